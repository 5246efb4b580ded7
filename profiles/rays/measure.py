#!/usr/bin/env python3
"""How long the ray-query pass takes, against its two yardsticks: python3 profiles/rays/measure.py [passes per variant, default 30] [out.json] [--trace]

big-scene and macho-cows, the 1920x1080 camera rays, in each of the three traversals; rays and results resident on the GPU, every variant warmed
first, the variants alternating inside one loop of ONE process, kernel times from the passes' own HIP events:
  aov          pt_aov_device, six buffers: the same rays built from the camera, one 8x8 tile per wavefront             (yardstick a)
  pixel r0     pt_rays_device, the rays in pixel order (row-major: a wavefront = 64 pixels of a row), six buffers, reorder = 0
  pixel r1     ... reorder = 1: what the sort costs a batch that needs none
  shuffled r0  the same rays in seeded random order, reorder = 0
  shuffled r1  ... reorder = 1 (keying + sort + cast)
  any r0 / r1  the shuffled batch as an occlusion query
  cast wall    pt_test_cast_rays (one walk per LANE) on both orders: WALL time of the call, its five hipMallocs and copies included (yardstick b;
               its kernel alone: run this script with --trace under `rocprofv3 --kernel-trace --stats -- python3 ...` and read pt_cast_kernel's row,
               where the keying and sort kernels of reorder = 1 are listed too)
Then, flat_scene semantics only: reorder = 0 against 1 over batch sizes (the first n of the shuffled batch) and over degrees of disorder (pixel order
shuffled inside consecutive blocks of B rays). --trace: three passes per variant, no sweeps - for a profiler run."""
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

W, HT = 1920, 1080
SIX = ("t", "position", "normal", "node", "sub", "material")


def stats(v):
    v = np.sort(np.asarray(v))
    return dict(median=float(np.median(v)), p10=float(v[len(v) // 10]), p90=float(v[(9 * len(v)) // 10]), min=float(v[0]), max=float(v[-1]))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    trace = "--trace" in sys.argv
    n_pass = 3 if trace else (int(args[0]) if args else 30)
    out_path = args[1] if len(args) > 1 else None
    import oracle_lib as O
    O.build()
    lib = H.lib()
    result = {"size": [W, HT], "passes_per_variant": n_pass, "scenes": {}}
    px = W * HT
    for scene_name in ("big-scene", "macho-cows"):
        sc = host.Scene.example(scene_name)
        ys, xs = np.mgrid[0:HT, 0:W]
        o_px, d_px = O.camera_rays(sc.camera, W, HT, np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float64))
        rng = np.random.default_rng(1)
        shuffle = rng.permutation(px)
        result["scenes"][scene_name] = {}
        for name, tr in (("flat", H.TRAVERSE_FLAT), ("kd", H.TRAVERSE_KD), ("hier", H.TRAVERSE_HIER)):
            r = host.Renderer(sc, tr)
            c = r.context
            cam = host.camera(sc.camera, W, HT)

            def alloc(nbytes):
                p = C.c_void_p()
                assert lib.pt_device_alloc(c, nbytes, C.byref(p)) == 0, lib.pt_last_error(c)
                return p

            def upload(a):
                a = np.ascontiguousarray(a)
                p = alloc(a.nbytes)
                assert lib.pt_copy_to_device(c, p, a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
                return p
            bufs = {k: alloc(px * comps * np.dtype(dt).itemsize) for k, (dt, comps) in H.RAYS_BUFFERS.items()}
            ptr = {np.float64: H._dp, np.int32: H._ip, np.uint8: H._u8p}
            six, occ, aovb = H.PtRaysBuffers(), H.PtRaysBuffers(), H.PtAovBuffers()
            for k in SIX:
                setattr(six, k, C.cast(bufs[k], ptr[H.RAYS_BUFFERS[k][0]]))
                setattr(aovb, "depth" if k == "t" else k, C.cast(bufs[k], ptr[H.RAYS_BUFFERS[k][0]]))
            occ.occluded = C.cast(bufs["occluded"], H._u8p)
            ap = H.PtAovParams(W, HT, H.PtRect(0, 0, W - 1, HT - 1), (C.c_double * 2)(0.5, 0.5))
            ms = C.c_double(0.0)
            rays_dev = {"pixel": (upload(o_px), upload(d_px)), "shuffled": (upload(o_px[shuffle]), upload(d_px[shuffle]))}
            frees = list(bufs.values()) + [p for pair in rays_dev.values() for p in pair]

            def aov():
                assert lib.pt_aov_device(c, C.byref(cam), C.byref(ap), C.byref(aovb), None) == 0, lib.pt_last_error(c)
                assert lib.pt_aov_finish(c, C.byref(ms)) == 0, lib.pt_last_error(c)
                return ms.value

            def rays(pair, n, any_hit, reorder):
                p = H.PtRaysParams(n, any_hit, reorder)
                assert lib.pt_rays_device(c, C.byref(p), pair[0], pair[1], C.byref(occ if any_hit else six), None) == 0, lib.pt_last_error(c)
                assert lib.pt_rays_finish(c, C.byref(ms)) == 0, lib.pt_last_error(c)
                return ms.value
            variants = {"aov": aov,
                        "pixel r0": lambda: rays(rays_dev["pixel"], px, 0, 0), "pixel r1": lambda: rays(rays_dev["pixel"], px, 0, 1),
                        "shuffled r0": lambda: rays(rays_dev["shuffled"], px, 0, 0), "shuffled r1": lambda: rays(rays_dev["shuffled"], px, 0, 1),
                        "any r0": lambda: rays(rays_dev["shuffled"], px, 1, 0), "any r1": lambda: rays(rays_dev["shuffled"], px, 1, 1)}
            for _ in range(3):  # warm-up of every variant
                for f in variants.values():
                    f()
            t = {k: [] for k in variants}
            for _ in range(n_pass):
                for k, f in variants.items():
                    t[k].append(f())
            m = {k: stats(v) for k, v in t.items()}
            tt, nn, ss = np.zeros(px), np.zeros(px, dtype=np.int32), np.zeros(px, dtype=np.int32)
            for label, (oo, dd) in (("cast wall pixel", (o_px, d_px)), ("cast wall shuffled", (np.ascontiguousarray(o_px[shuffle]), np.ascontiguousarray(d_px[shuffle])))):
                best = 1e30
                for _ in range(3):
                    t0 = time.perf_counter()
                    rc = lib.pt_test_cast_rays(c, px, oo.ctypes.data_as(H._dp), dd.ctypes.data_as(H._dp), 0, tt.ctypes.data_as(H._dp), nn.ctypes.data_as(H._ip), ss.ctypes.data_as(H._ip))
                    best = min(best, (time.perf_counter() - t0) * 1e3)
                m[label] = best if rc == 0 else "refused: %d" % rc
            print("%-10s %-4s " % (scene_name, name) + "  ".join("%s %.3f [%.3f .. %.3f]" % (k, m[k]["median"], m[k]["p10"], m[k]["p90"]) for k in variants) +
                  "  cast wall pixel / shuffled %s / %s   (ms: median [p10 .. p90] of %d)" % (m["cast wall pixel"], m["cast wall shuffled"], n_pass), flush=True)
            if name == "flat" and not trace:
                sweep = {"batch": {}, "disorder": {}}
                for n in (1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20, px):
                    for _ in range(2):
                        rays(rays_dev["shuffled"], n, 0, 0); rays(rays_dev["shuffled"], n, 0, 1)
                    a, b = [], []
                    for _ in range(n_pass):
                        a.append(rays(rays_dev["shuffled"], n, 0, 0)); b.append(rays(rays_dev["shuffled"], n, 0, 1))
                    sweep["batch"][n] = {"r0": stats(a), "r1": stats(b)}
                    print("  shuffled, first %8d rays: r0 %.3f  r1 %.3f ms" % (n, np.median(a), np.median(b)), flush=True)
                for block in (64, 1024, 1 << 14, 1 << 17, 1 << 19):
                    idx = np.arange(px)
                    for s in range(0, px, block):
                        idx[s:s + block] = s + rng.permutation(min(block, px - s))
                    pair = (upload(o_px[idx]), upload(d_px[idx]))
                    for _ in range(2):
                        rays(pair, px, 0, 0); rays(pair, px, 0, 1)
                    a, b = [], []
                    for _ in range(n_pass):
                        a.append(rays(pair, px, 0, 0)); b.append(rays(pair, px, 0, 1))
                    sweep["disorder"][block] = {"r0": stats(a), "r1": stats(b)}
                    print("  pixel order shuffled inside blocks of %7d: r0 %.3f  r1 %.3f ms" % (block, np.median(a), np.median(b)), flush=True)
                    for p in pair:
                        lib.pt_device_free(c, p)
                m["sweep"] = sweep
            result["scenes"][scene_name][name] = m
            for p in frees:
                lib.pt_device_free(c, p)
            r.close()
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
