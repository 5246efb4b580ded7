#!/usr/bin/env python3
"""How long the radiance pass takes, against its yardstick: python3 profiles/radiance/measure.py [passes per side, default 20] [out.json] [scene,scene,...]

big-scene, entering-the-mirror-dimension, macho-cows and transmission-refraction at 1920x1080, flat_scene and hierarchical traversal, everything resident on the
GPU and alternating in ONE process after a warm-up of each side:
  render      pt_render_device + pt_render_finish, samples = 1, PT_SAMPLE_CENTRE, collect_stats = 0   -> pt_stats.kernel_ms (render + finishing kernel)
  radiance    pt_radiance_device + pt_radiance_finish over the 2,073,600 pixel-centre rays in pixel order, the render's background row per ray -> kernel_ms
  shuffled 0  the same batch in a seeded random order, reorder = 0
  shuffled 1  ... reorder = 1 (kernel_ms includes keying and sort)
The render kernels are byte-identical to the parent commit's (tools/compare_render_objects.py), so `render` is the parent's number. The pass is expected to be
slower: 64 pixels of a row per wavefront and not an 8x8 tile, no occluder table, the interpreter where the render runs its straight-line kernel. Prints one
line per (scene, traversal) with medians [p10 .. p90], Mray/s of primary rays and the ratios, then one JSON line."""
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

W, HT = 1920, 1080
SCENES = ("big-scene", "entering-the-mirror-dimension", "macho-cows", "transmission-refraction")


def stats(v):
    v = np.sort(np.asarray(v))
    return dict(median=float(np.median(v)), p10=float(v[len(v) // 10]), p90=float(v[(9 * len(v)) // 10]), min=float(v[0]), max=float(v[-1]))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
    scenes = tuple(sys.argv[3].split(",")) if len(sys.argv) > 3 else SCENES
    import oracle_lib as O
    O.build()
    lib = H.lib()
    bg = default_background(W, HT)
    px = W * HT
    ys, xs = np.mgrid[0:HT, 0:W]
    order = np.random.default_rng(1).permutation(px)
    result = {"size": [W, HT], "passes_per_side": n, "runs": {}}
    for scene in scenes:
        sc = host.Scene.example(scene, assets=ASSETS)
        o, d = O.camera_rays(sc.camera, W, HT, np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float64))
        bg_rays = np.ascontiguousarray(np.repeat(bg, W, axis=0)) if bg.shape == (HT, 3) else np.ascontiguousarray(bg.reshape(-1, 3))
        for name, tr in (("flat", H.TRAVERSE_FLAT), ("hier", H.TRAVERSE_HIER)):
            r = host.Renderer(sc, tr)
            c = r.context
            cam = host.camera(sc.camera, W, HT)

            def alloc(nbytes, src=None):
                p = C.c_void_p()
                assert lib.pt_device_alloc(c, nbytes, C.byref(p)) == 0, lib.pt_last_error(c)
                if src is not None:
                    assert lib.pt_copy_to_device(c, p, src.ctypes.data_as(C.c_void_p), src.nbytes) == 0
                return p
            d_bg, d_rgb, d_out = alloc(bg.nbytes, bg), alloc(px * 3), alloc(px * 24)
            inorder = [alloc(px * 24, a) for a in (o, d, bg_rays)]
            shuffled = [alloc(px * 24, np.ascontiguousarray(a[order])) for a in (o, d, bg_rays)]
            rp = H.PtRenderParams(W, HT, H.PtRect(0, 0, W - 1, HT - 1), 1, 0, H.SAMPLE_CENTRE, 1 if bg.shape == (HT, 3) else 0, 0, 1, 0)
            st, ms = H.PtStats(), C.c_double(0.0)

            def render():
                assert lib.pt_render_device(c, C.byref(cam), d_bg, C.byref(rp), 0, d_rgb, None) == 0, lib.pt_last_error(c)
                assert lib.pt_render_finish(c, C.byref(st)) == 0, lib.pt_last_error(c)
                return st.kernel_ms

            def radiance(arrays, reorder):
                p = H.PtRadianceParams(px, reorder, 1, 0, 0, 0)
                assert lib.pt_radiance_device(c, C.byref(p), arrays[0], arrays[1], arrays[2], d_out, None) == 0, lib.pt_last_error(c)
                assert lib.pt_radiance_finish(c, C.byref(ms)) == 0, lib.pt_last_error(c)
                return ms.value
            sides = {"render": render, "radiance": lambda: radiance(inorder, 0), "shuffled_0": lambda: radiance(shuffled, 0), "shuffled_1": lambda: radiance(shuffled, 1)}
            for _ in range(3):  # warm-up of each side
                for f in sides.values():
                    f()
            t = {k: [] for k in sides}
            for _ in range(n):
                for k, f in sides.items():
                    t[k].append(f())
            m = {k: stats(v) for k, v in t.items()}
            m["kernel_mode"], m["kernel_variant"] = int(st.kernel_mode), int(st.kernel_variant)
            m["mray_s"] = {k: px / m[k]["median"] / 1e3 for k in sides}
            m["ratio_to_render"] = {k: m[k]["median"] / m["render"]["median"] for k in sides if k != "render"}
            result["runs"]["%s/%s" % (scene, name)] = m
            print("%-30s %-4s " % (scene, name) + "   ".join("%s %.3f ms [%.3f .. %.3f] %.0f Mray/s" % (k, m[k]["median"], m[k]["p10"], m[k]["p90"], m["mray_s"][k]) for k in sides) +
                  "   radiance / render %.2f, shuffled %.2f, shuffled + reorder %.2f  (median [p10 .. p90] of %d)" % (
                      m["ratio_to_render"]["radiance"], m["ratio_to_render"]["shuffled_0"], m["ratio_to_render"]["shuffled_1"], n), flush=True)
            for p in [d_bg, d_rgb, d_out] + inorder + shuffled:
                lib.pt_device_free(c, p)
            r.close()
    print(json.dumps(result))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
