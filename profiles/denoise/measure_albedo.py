#!/usr/bin/env python3
"""What the guides pass and the demodulated denoise cost and buy: python3 profiles/denoise/measure_albedo.py [repeats per side, default 5] [out.json] [cost|quality|both]

cost     big-scene (untextured) and transmission-refraction (textured) at 1920x1080, flat_scene traversal: the guides pass with all four buffers
         (pt_guides_device) beside the aov pass of the same build asking for position, normal and node (pt_aov_device), and a 5-level denoise of a film with
         moments that holds 8 samples per pixel, with and without albedo (pt_film_denoise_albedo_device / pt_film_denoise_device, default parameters of
         Film.denoise) - all sides alternating in ONE process after a warm-up of each. Every figure is device time between two HIP events on the null
         stream around the call. Medians [p10 .. p90] of the repeats.
quality  texture-mapping and transmission-refraction at 268 x 148 after add(8), seed 7, PT_SAMPLE_RNG: the RMS difference (over all values of `linear`) to
         render(samples=512) of resolve(), denoise() and denoise(albedo=True), at 1 and 5 levels; and, as a diagnostic, of the demodulated filter fed
         with the mean albedo of 16 guides passes on a 4 x 4 grid of offsets inside the pixel.
texture-mapping opens assets/earth_cube.png, which the reference repository lacks: a seeded random stand-in is made in a temporary directory, as the tests do.
For the record, not gates. Prints one line per figure, then one JSON line."""
import ctypes as C
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from portrayer_amd import _hip as H  # noqa: E402
from portrayer_amd import host  # noqa: E402
from scene_dsl import ASSETS, default_background  # noqa: E402

COST_SCENES = ("big-scene", "transmission-refraction")
QUALITY_SCENES = ("texture-mapping", "transmission-refraction")
SEED = 7


def stats(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return dict(median=float(np.median(v)), p10=float(v[len(v) // 10]), p90=float(v[(9 * len(v)) // 10]), min=float(v[0]), max=float(v[-1]))


def assets_with_stand_in():
    from PIL import Image
    d = tempfile.mkdtemp(prefix="assets")
    for f in os.listdir(ASSETS):
        os.symlink(os.path.join(ASSETS, f), os.path.join(d, f))
    Image.fromarray(np.random.default_rng(3).integers(0, 256, size=(48, 64, 3), dtype=np.uint8)).save(os.path.join(d, "earth_cube.png"))
    return d


def cost(n, assets):
    lib = H.lib()
    hip = C.CDLL("libamdhip64.so")  # (already loaded: the library links against it) - events only
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    w, h = 1920, 1080
    px = w * h
    out = {}
    for scene in COST_SCENES:
        bg = default_background(w, h)
        rows = 1 if bg.shape == (h, 3) else 0
        sc = host.Scene.example(scene, assets=assets)
        r = host.Renderer(sc, H.TRAVERSE_FLAT)
        c = r.context
        cam = host.camera(sc.camera, w, h)
        ev0, ev1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0

        def alloc(nbytes):
            p = C.c_void_p()
            assert lib.pt_device_alloc(c, nbytes, C.byref(p)) == 0, lib.pt_last_error(c)
            return p
        d_alb, d_pos, d_nrm, d_node, d_rgb, d_lin = alloc(px * 24), alloc(px * 24), alloc(px * 24), alloc(px * 4), alloc(px * 3), alloc(px * 24)
        full = H.PtRect(0, 0, w - 1, h - 1)
        ap = H.PtAovParams(w, h, full, (C.c_double * 2)(0.5, 0.5))
        ab = H.PtAovBuffers()
        ab.position, ab.normal, ab.node = C.cast(d_pos, H._dp), C.cast(d_nrm, H._dp), C.cast(d_node, H._ip)
        gb = H.PtGuidesBuffers()
        gb.albedo, gb.position, gb.normal, gb.node = C.cast(d_alb, H._dp), C.cast(d_pos, H._dp), C.cast(d_nrm, H._dp), C.cast(d_node, H._ip)
        guides = H.PtDenoiseGuides(d_pos.value, d_nrm.value, d_node.value)
        film = C.c_void_p()
        assert lib.pt_film_create_moments(c, w, h, C.byref(film)) == 0, lib.pt_last_error(c)
        fp = H.PtFilmParams(full, 8, SEED, H.SAMPLE_RNG, rows)
        assert lib.pt_film_add(c, film, C.byref(cam), bg.ctypes.data_as(H._dp), C.byref(fp), None) == 0, lib.pt_last_error(c)
        p5 = H.PtDenoiseParams(5, 0, 2.0, 0.0, 5)

        def timed(call, finish=None):
            assert hip.hipEventRecord(ev0, None) == 0
            assert call() == 0, lib.pt_last_error(c)
            assert hip.hipEventRecord(ev1, None) == 0 and hip.hipEventSynchronize(ev1) == 0
            if finish:
                assert finish(c, None) == 0, lib.pt_last_error(c)
            t = C.c_float(0.0)
            assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
            return float(t.value)

        sides = {
            "aov_position_normal_node": lambda: timed(lambda: lib.pt_aov_device(c, C.byref(cam), C.byref(ap), C.byref(ab), None), lib.pt_aov_finish),
            "guides_all_four": lambda: timed(lambda: lib.pt_guides_device(c, C.byref(cam), C.byref(ap), C.byref(gb), None), lib.pt_guides_finish),
            "denoise_5": lambda: timed(lambda: lib.pt_film_denoise_device(c, film, C.byref(p5), C.byref(guides), d_rgb, d_lin, None, None)),
            "denoise_5_albedo": lambda: timed(lambda: lib.pt_film_denoise_albedo_device(c, film, C.byref(p5), C.byref(guides), C.cast(d_alb, H._dp), d_rgb, d_lin, None, None)),
        }
        for f in sides.values():  # warm-up of each side
            f()
        t = {k: [] for k in sides}
        for _ in range(n):
            for k, f in sides.items():
                t[k].append(f())
        m = {k: stats(v) for k, v in t.items()}
        out[scene] = m
        print("%-24s %dx%d" % (scene, w, h), flush=True)
        for k in sides:
            print("    %-26s %9.3f ms [%9.3f .. %9.3f]" % (k, m[k]["median"], m[k]["p10"], m[k]["p90"]), flush=True)
        print("    guides / aov %.2f, denoise with / without albedo %.3f" % (m["guides_all_four"]["median"] / m["aov_position_normal_node"]["median"],
                                                                            m["denoise_5_albedo"]["median"] / m["denoise_5"]["median"]), flush=True)
        assert lib.pt_film_destroy(c, film) == 0
        for p in (d_alb, d_pos, d_nrm, d_node, d_rgb, d_lin):
            lib.pt_device_free(c, p)
        r.close()
    return out


def quality(assets):
    w, h = 268, 148
    out = {}
    for scene in QUALITY_SCENES:
        sc = host.Scene.example(scene, assets=assets)
        r = host.Renderer(sc, H.TRAVERSE_FLAT)
        bg = default_background(w, h)
        film = r.film(w, h, moments=True)
        film.add(sc.camera, bg, samples=8, seed=SEED, sample_mode=H.SAMPLE_RNG)
        _, ref, _ = r.render(sc.camera, w, h, bg, samples=512, seed=SEED, sample_mode=H.SAMPLE_RNG)
        rms = lambda c: float(np.sqrt(np.mean((c - ref) ** 2)))
        m = {"resolve": rms(film.resolve()[1])}
        # a diagnostic beside the product's path: the caller's albedo as the mean of 16 guides passes on a 4 x 4 grid of offsets inside the pixel - what an
        # antialiased albedo guide would give, against the one centre sample of albedo=True
        g = r.guides(sc.camera, w, h)
        grid = [(i + 0.5) / 4.0 for i in range(4)]
        mean_albedo = sum(r.guides(sc.camera, w, h, offset=(ox, oy), want=("albedo",))["albedo"] for oy in grid for ox in grid) / 16.0
        for levels in (1, 5):
            m["denoise_%d" % levels] = rms(film.denoise(sc.camera, iterations=levels, sigma_color=2.0)[1])
            m["denoise_%d_albedo" % levels] = rms(film.denoise(sc.camera, iterations=levels, sigma_color=2.0, albedo=True)[1])
            m["denoise_%d_albedo_mean16" % levels] = rms(film.denoise(None, iterations=levels, sigma_color=2.0, guides=g, albedo=mean_albedo)[1])
        out[scene] = m
        print("%-24s %dx%d after add(8): rms to render(samples=512)" % (scene, w, h), flush=True)
        for k, v in m.items():
            print("    %-26s %.5f (%.3f x resolve)" % (k, v, v / m["resolve"]), flush=True)
        film.close()
        r.close()
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
    what = sys.argv[3] if len(sys.argv) > 3 else "both"
    assets = assets_with_stand_in()
    result = {"repeats_per_side": n}
    if what in ("quality", "both"):
        result["quality"] = quality(assets)
    if what in ("cost", "both"):
        result["cost"] = cost(n, assets)
    print(json.dumps(result))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
