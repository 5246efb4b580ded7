#!/usr/bin/env python3
"""How long the primary-visibility pass takes, against its yardstick: python3 profiles/aov/measure.py [passes per side, default 200] [out.json]

big-scene, 1920x1080, in each of the three traversals, everything resident on the GPU and alternating in ONE process after a warm-up of each:
  render    pt_render_device + pt_render_finish, samples = 1, PT_SAMPLE_CENTRE, collect_stats = 0  -> pt_stats.kernel_ms (render + finishing kernel)
  aov all   pt_aov_device + pt_aov_finish, all six buffers                                         -> kernel_ms
  aov d+n   the same, depth + node only
The render traces the same 2.07 M primary rays at the same granularity and then shades every hit, so the pass must come in below it.
One line of context: the same rays through pt_test_cast_rays (wall time, copies included)."""
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
from scene_dsl import default_background  # noqa: E402

W, HT = 1920, 1080


def stats(v):
    v = np.sort(np.asarray(v))
    return dict(median=float(np.median(v)), p10=float(v[len(v) // 10]), p90=float(v[(9 * len(v)) // 10]), min=float(v[0]), max=float(v[-1]))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    lib = H.lib()
    sc = host.Scene.example("big-scene")
    bg = default_background(W, HT)
    result = {"scene": "big-scene", "size": [W, HT], "passes_per_side": n, "modes": {}}
    for name, tr in (("flat", H.TRAVERSE_FLAT), ("kd", H.TRAVERSE_KD), ("hier", H.TRAVERSE_HIER)):
        r = host.Renderer(sc, tr)
        c = r.context
        cam = host.camera(sc.camera, W, HT)

        def alloc(nbytes):
            p = C.c_void_p()
            assert lib.pt_device_alloc(c, nbytes, C.byref(p)) == 0, lib.pt_last_error(c)
            return p
        d_bg, d_rgb = alloc(bg.nbytes), alloc(W * HT * 3)
        assert lib.pt_copy_to_device(c, d_bg, bg.ctypes.data_as(C.c_void_p), bg.nbytes) == 0
        px = W * HT
        d = {k: alloc(px * comps * np.dtype(dt).itemsize) for k, (dt, comps) in H.AOV_BUFFERS.items()}
        every, two = H.PtAovBuffers(), H.PtAovBuffers()
        for k, (dt, _) in H.AOV_BUFFERS.items():
            ptr = C.cast(d[k], H._dp if dt is np.float64 else H._ip)
            setattr(every, k, ptr)
            if k in ("depth", "node"):
                setattr(two, k, ptr)
        rp = H.PtRenderParams(W, HT, H.PtRect(0, 0, W - 1, HT - 1), 1, 0, H.SAMPLE_CENTRE, 1 if bg.shape == (HT, 3) else 0, 0, 1, 0)
        ap = H.PtAovParams(W, HT, H.PtRect(0, 0, W - 1, HT - 1), (C.c_double * 2)(0.5, 0.5))
        st, ms = H.PtStats(), C.c_double(0.0)

        def render():
            assert lib.pt_render_device(c, C.byref(cam), d_bg, C.byref(rp), 0, d_rgb, None) == 0, lib.pt_last_error(c)
            assert lib.pt_render_finish(c, C.byref(st)) == 0, lib.pt_last_error(c)
            return st.kernel_ms

        def aov(b):
            assert lib.pt_aov_device(c, C.byref(cam), C.byref(ap), C.byref(b), None) == 0, lib.pt_last_error(c)
            assert lib.pt_aov_finish(c, C.byref(ms)) == 0, lib.pt_last_error(c)
            return ms.value
        for _ in range(10):  # warm-up of each side
            render(); aov(every); aov(two)
        t = {"render": [], "aov_all": [], "aov_depth_node": []}
        for _ in range(n):
            t["render"].append(render()); t["aov_all"].append(aov(every)); t["aov_depth_node"].append(aov(two))
        m = {k: stats(v) for k, v in t.items()}
        m["kernel_mode"], m["kernel_variant"] = int(st.kernel_mode), int(st.kernel_variant)
        if name == "flat":  # context only: the self-test's per-lane walkers on the same rays, host buffers
            try:
                import oracle_lib as O
                O.build()
                ys, xs = np.mgrid[0:HT, 0:W]
                o, dr = O.camera_rays(sc.camera, W, HT, np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1))
                tt, nn, ss = np.zeros(px), np.zeros(px, dtype=np.int32), np.zeros(px, dtype=np.int32)
                best = 1e30
                for _ in range(3):
                    t0 = time.perf_counter()
                    assert lib.pt_test_cast_rays(c, px, o.ctypes.data_as(H._dp), dr.ctypes.data_as(H._dp), 0, tt.ctypes.data_as(H._dp), nn.ctypes.data_as(H._ip), ss.ctypes.data_as(H._ip)) == 0
                    best = min(best, (time.perf_counter() - t0) * 1e3)
                m["pt_test_cast_rays_wall_ms"] = best
            except Exception as e:  # the figure is context, not a requirement
                m["pt_test_cast_rays_wall_ms"] = "not measured: %s" % e
        result["modes"][name] = m
        print("%-5s render(samples=1) %.3f ms [%.3f .. %.3f]   aov all %.3f ms [%.3f .. %.3f]   aov depth+node %.3f ms [%.3f .. %.3f]   (median [p10 .. p90] of %d)" % (
            name, m["render"]["median"], m["render"]["p10"], m["render"]["p90"], m["aov_all"]["median"], m["aov_all"]["p10"], m["aov_all"]["p90"],
            m["aov_depth_node"]["median"], m["aov_depth_node"]["p10"], m["aov_depth_node"]["p90"], n), flush=True)
        for p in [d_bg, d_rgb] + list(d.values()):
            lib.pt_device_free(c, p)
        r.close()
    print(json.dumps(result))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1)
    bad = [k for k, m in result["modes"].items() if not m["aov_all"]["median"] <= m["render"]["median"]]
    if bad:
        print("the pass is NOT below the samples = 1 render in: " + ", ".join(bad))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
