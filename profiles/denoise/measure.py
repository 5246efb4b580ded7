#!/usr/bin/env python3
"""What the film's denoiser costs, and which form of its level kernel is faster: python3 profiles/denoise/measure.py [repeats per side, default 5] [out.json] [scene,scene,...]

big-scene and soft-shadows at 1920x1080, flat_scene traversal, PT_SAMPLE_RNG: a film with moments that holds 8 samples per pixel, guides from pt_aov_device
(they never leave the device), then pt_film_denoise_device with the default parameters of Film.denoise (sigma_color 2, no plane weight, normal power 32) at
1 .. 5 levels, in the direct (PORTRAYER_DENOISE_TILE=0) and the tiled (=1) form, and once with the plane weight on (5 levels) - all sides alternating in ONE
process after a warm-up of each. Every denoise / resolve figure is device time between two HIP events on the null stream around the call's kernels (seed,
levels, finish); `add8` is pt_film_add's own kernel_ms. A level's time is the difference of the medians at k and k - 1 levels; `1 level` carries the seed and
finish kernels. For scale, not as a gate: pt_film_resolve_device and add(8) of the same build.
The two forms' outputs are compared once per scene (they must be identical). The rule for the default: the form that is faster at 5 levels by more than three
spreads (p90 - p10) of the other form's repeats; otherwise the direct form.
Prints one line per side with medians [p10 .. p90], then one JSON line."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from portrayer_amd import _hip as H  # noqa: E402
from portrayer_amd import host  # noqa: E402
from scene_dsl import ASSETS, default_background  # noqa: E402

SCENES = {"big-scene": (1920, 1080), "soft-shadows": (1920, 1080)}
SEED, MODE = 0, H.SAMPLE_RNG
LEVELS = (1, 2, 3, 4, 5)


def stats(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return dict(median=float(np.median(v)), p10=float(v[len(v) // 10]), p90=float(v[(9 * len(v)) // 10]), min=float(v[0]), max=float(v[-1]))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
    scenes = tuple(sys.argv[3].split(",")) if len(sys.argv) > 3 else tuple(SCENES)
    lib = H.lib()
    hip = C.CDLL("libamdhip64.so")  # (already loaded: the library links against it) - events only
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    result = {"repeats_per_side": n, "runs": {}}
    for scene in scenes:
        w, h = SCENES[scene]
        px = w * h
        bg = default_background(w, h)
        rows = 1 if bg.shape == (h, 3) else 0
        sc = host.Scene.example(scene, assets=ASSETS)
        r = host.Renderer(sc, H.TRAVERSE_FLAT)
        c = r.context
        cam = host.camera(sc.camera, w, h)
        ev0, ev1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0

        def alloc(nbytes):
            p = C.c_void_p()
            assert lib.pt_device_alloc(c, nbytes, C.byref(p)) == 0, lib.pt_last_error(c)
            return p
        d_pos, d_nrm, d_node, d_rgb, d_lin = alloc(px * 24), alloc(px * 24), alloc(px * 4), alloc(px * 3), alloc(px * 24)
        full = H.PtRect(0, 0, w - 1, h - 1)
        ap = H.PtAovParams(w, h, full, (C.c_double * 2)(0.5, 0.5))
        ab = H.PtAovBuffers()
        ab.position, ab.normal, ab.node = C.cast(d_pos, H._dp), C.cast(d_nrm, H._dp), C.cast(d_node, H._ip)
        assert lib.pt_aov_device(c, C.byref(cam), C.byref(ap), C.byref(ab), None) == 0, lib.pt_last_error(c)
        aov_ms = C.c_double(0.0)
        assert lib.pt_aov_finish(c, C.byref(aov_ms)) == 0, lib.pt_last_error(c)
        guides = H.PtDenoiseGuides(d_pos.value, d_nrm.value, d_node.value)
        film, plain = C.c_void_p(), C.c_void_p()
        assert lib.pt_film_create_moments(c, w, h, C.byref(film)) == 0 and lib.pt_film_create(c, w, h, C.byref(plain)) == 0, lib.pt_last_error(c)
        fp = H.PtFilmParams(full, 8, SEED, MODE, rows)
        ms = C.c_double(0.0)
        assert lib.pt_film_add(c, film, C.byref(cam), bg.ctypes.data_as(H._dp), C.byref(fp), C.byref(ms)) == 0, lib.pt_last_error(c)

        def timed(call):
            assert hip.hipEventRecord(ev0, None) == 0
            assert call() == 0, lib.pt_last_error(c)
            assert hip.hipEventRecord(ev1, None) == 0 and hip.hipEventSynchronize(ev1) == 0
            t = C.c_float(0.0)
            assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
            return float(t.value)

        def denoise(tile, levels, sigma_plane=0.0):
            os.environ["PORTRAYER_DENOISE_TILE"] = str(tile)  # (read per call)
            p = H.PtDenoiseParams(levels, 0, 2.0, sigma_plane, 5)
            return timed(lambda: lib.pt_film_denoise_device(c, film, C.byref(p), C.byref(guides), d_rgb, d_lin, None, None))

        def add8():
            assert lib.pt_film_reset(c, plain) == 0
            assert lib.pt_film_add(c, plain, C.byref(cam), bg.ctypes.data_as(H._dp), C.byref(fp), C.byref(ms)) == 0, lib.pt_last_error(c)
            return ms.value

        # the two forms compute the same bits at this size too
        outs = []
        for tile in (0, 1):
            denoise(tile, 5, 0.05)
            o = np.empty((h, w, 3))
            assert lib.pt_copy_from_device(c, o.ctypes.data_as(C.c_void_p), d_lin, o.nbytes) == 0
            outs.append(o)
        identical = outs[0].tobytes() == outs[1].tobytes()

        sides = {"resolve": lambda: timed(lambda: lib.pt_film_resolve_device(c, film, d_rgb, d_lin, None)), "add8": add8}
        for tile, tag in ((0, "direct"), (1, "tiled")):
            for k in LEVELS:
                sides["%s_%d" % (tag, k)] = (lambda tile=tile, k=k: denoise(tile, k))
            sides["%s_5_plane" % tag] = (lambda tile=tile: denoise(tile, 5, 0.05))
        for f in sides.values():  # warm-up of each side
            f()
        t = {k: [] for k in sides}
        for _ in range(n):
            for k, f in sides.items():
                t[k].append(f())
        m = {k: stats(v) for k, v in t.items()}
        m["aov_ms"], m["forms_identical"] = aov_ms.value, identical
        d5, t5 = m["direct_5"], m["tiled_5"]
        if t5["median"] < d5["median"] - 3.0 * (d5["p90"] - d5["p10"]):
            m["faster_at_5_levels"] = "tiled"
        elif d5["median"] < t5["median"] - 3.0 * (t5["p90"] - t5["p10"]):
            m["faster_at_5_levels"] = "direct"
        else:
            m["faster_at_5_levels"] = "neither by three spreads"
        result["runs"][scene] = m
        print("%-16s %dx%d   aov %.3f ms   forms identical: %s" % (scene, w, h, aov_ms.value, identical), flush=True)
        for k in sides:
            print("    %-16s %9.3f ms [%9.3f .. %9.3f]" % (k, m[k]["median"], m[k]["p10"], m[k]["p90"]), flush=True)
        for tag in ("direct", "tiled"):
            per = [m["%s_1" % tag]["median"]] + [m["%s_%d" % (tag, k)]["median"] - m["%s_%d" % (tag, k - 1)]["median"] for k in LEVELS[1:]]
            print("    %-7s seed + level 0 + finish %.3f ms, levels 1 .. 4: %s ms" % (tag, per[0], ", ".join("%.3f" % v for v in per[1:])), flush=True)
        print("    faster at 5 levels: %s (tiled / direct %.3f)" % (m["faster_at_5_levels"], t5["median"] / d5["median"]), flush=True)
        assert lib.pt_film_destroy(c, film) == 0 and lib.pt_film_destroy(c, plain) == 0
        for p in (d_pos, d_nrm, d_node, d_rgb, d_lin):
            lib.pt_device_free(c, p)
        r.close()
        assert identical, "the direct and the tiled form differ"
    print(json.dumps(result))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
