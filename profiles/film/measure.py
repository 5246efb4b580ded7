#!/usr/bin/env python3
"""What a film costs, against its yardstick: python3 profiles/film/measure.py [repeats per side, default 7] [out.json] [scene,scene,...]

big-scene, entering-the-mirror-dimension and transmission-refraction at 1920x1080 and macho-cows at its bench size (1280x720), 64 samples per pixel in
total, flat_scene traversal, everything resident on the GPU, the sides alternating in ONE process after a warm-up of each:
  render        pt_render_device + pt_render_finish, samples = 64, PT_SAMPLE_RNG, collect_stats = 0   -> pt_stats.kernel_ms (render + finishing kernel)
  film 1 x 64   pt_film_reset, then ONE pt_film_add_device of 64 samples + pt_radiance_finish -> kernel_ms (sampling launches and their folds), one resolve
  film 8 x 8    ... eight adds of 8, a pt_film_resolve_device after each (the preview that sharpens)
  film 64 x 1   ... 64 adds of 1, a resolve after each
each film side once with launches of at most 8 samples per pixel (PORTRAYER_FILM_LW=8, the default) and once with 64. Per side: the sum of the adds' kernel_ms,
and separately the host's wall time of one resolve (launch + pt_synchronize, device buffers). The render kernels are byte-identical to the parent commit's
(tools/compare_render_objects.py), so `render` is the parent's number. Prints one line per scene with medians [p10 .. p90] and the ratios to `render`, then one
JSON line."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from portrayer_amd import _hip as H  # noqa: E402
from portrayer_amd import host  # noqa: E402
from scene_dsl import ASSETS, default_background  # noqa: E402

SAMPLES = 64
SCENES = {"big-scene": (1920, 1080), "entering-the-mirror-dimension": (1920, 1080), "transmission-refraction": (1920, 1080), "macho-cows": (1280, 720)}
PLANS = {"1x64": (64,), "8x8": (8,) * 8, "64x1": (1,) * 64}


def stats(v):
    v = np.sort(np.asarray(v))
    return dict(median=float(np.median(v)), p10=float(v[len(v) // 10]), p90=float(v[(9 * len(v)) // 10]), min=float(v[0]), max=float(v[-1]))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
    scenes = tuple(sys.argv[3].split(",")) if len(sys.argv) > 3 else tuple(SCENES)
    lib = H.lib()
    result = {"samples": SAMPLES, "repeats_per_side": n, "runs": {}}
    for scene in scenes:
        w, h = SCENES[scene]
        px = w * h
        bg = default_background(w, h)
        rows = 1 if bg.shape == (h, 3) else 0
        sc = host.Scene.example(scene, assets=ASSETS)
        r = host.Renderer(sc, H.TRAVERSE_FLAT)
        c = r.context
        cam = host.camera(sc.camera, w, h)

        def alloc(nbytes, src=None):
            p = C.c_void_p()
            assert lib.pt_device_alloc(c, nbytes, C.byref(p)) == 0, lib.pt_last_error(c)
            if src is not None:
                assert lib.pt_copy_to_device(c, p, src.ctypes.data_as(C.c_void_p), src.nbytes) == 0
            return p
        d_bg, d_rgb, d_lin = alloc(bg.nbytes, bg), alloc(px * 3), alloc(px * 24)
        full = H.PtRect(0, 0, w - 1, h - 1)
        rp = H.PtRenderParams(w, h, full, SAMPLES, 0, H.SAMPLE_RNG, rows, 0, 1, 0)
        st, ms = H.PtStats(), C.c_double(0.0)
        film = C.c_void_p()
        assert lib.pt_film_create(c, w, h, C.byref(film)) == 0, lib.pt_last_error(c)

        def render():
            assert lib.pt_render_device(c, C.byref(cam), d_bg, C.byref(rp), 0, d_rgb, None) == 0, lib.pt_last_error(c)
            assert lib.pt_render_finish(c, C.byref(st)) == 0, lib.pt_last_error(c)
            return st.kernel_ms, 0.0

        def film_side(plan, lw):
            os.environ["PORTRAYER_FILM_LW"] = str(lw)
            assert lib.pt_film_reset(c, film) == 0, lib.pt_last_error(c)
            kernel, resolve = 0.0, []
            for k in plan:
                p = H.PtFilmParams(full, k, 0, H.SAMPLE_RNG, rows)
                assert lib.pt_film_add_device(c, film, C.byref(cam), d_bg, C.byref(p), None) == 0, lib.pt_last_error(c)
                assert lib.pt_radiance_finish(c, C.byref(ms)) == 0, lib.pt_last_error(c)
                kernel += ms.value
                t0 = time.perf_counter()
                assert lib.pt_film_resolve_device(c, film, d_rgb, d_lin, None) == 0, lib.pt_last_error(c)
                assert lib.pt_synchronize(c) == 0
                resolve.append((time.perf_counter() - t0) * 1e3)
            return kernel, float(np.median(resolve))
        sides = {"render": render}
        for lw in (8, 64):
            for name, plan in PLANS.items():
                sides["film_%s_lw%d" % (name, lw)] = (lambda plan=plan, lw=lw: film_side(plan, lw))
        for f in sides.values():  # warm-up of each side
            f()
        t = {k: [] for k in sides}
        res = {k: [] for k in sides}
        for _ in range(n):
            for k, f in sides.items():
                a, b = f()
                t[k].append(a)
                res[k].append(b)
        m = {k: stats(v) for k, v in t.items()}
        m["resolve_wall_ms"] = {k: stats(v) for k, v in res.items() if k != "render"}
        m["kernel_mode"], m["kernel_variant"] = int(st.kernel_mode), int(st.kernel_variant)
        m["ratio_to_render"] = {k: m[k]["median"] / m["render"]["median"] for k in sides if k != "render"}
        result["runs"][scene] = m
        print("%-30s %dx%d render %.2f ms [%.2f .. %.2f]" % (scene, w, h, m["render"]["median"], m["render"]["p10"], m["render"]["p90"]), flush=True)
        for k in sides:
            if k != "render":
                print("    %-16s %.2f ms [%.2f .. %.2f]  x%.2f of render   resolve %.3f ms wall" % (
                    k, m[k]["median"], m[k]["p10"], m[k]["p90"], m["ratio_to_render"][k], m["resolve_wall_ms"][k]["median"]), flush=True)
        assert lib.pt_film_destroy(c, film) == 0
        for p in (d_bg, d_rgb, d_lin):
            lib.pt_device_free(c, p)
        r.close()
    os.environ.pop("PORTRAYER_FILM_LW", None)
    print(json.dumps(result))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
