#!/usr/bin/env python3
"""What the direct-light pass costs, against the two ways there were before it: python3 profiles/direct/measure.py [--case NAME] [--reps 5] [--no-host] [--out F.json]

1920x1080, flat traversal. Cases: big-scene and macho-cows (point lights, S = 1), soft-shadows (a point light and an area light, S = 16). The points are the pixel
centres' first hits (Renderer.aov), the normals turned to the eye: what Renderer.direct_camera traces. Per case:
  a   pt_segments_device, any_hit = 1, on the very rays the pass makes (the host replay pt_test_direct_host writes them; a point light's ray once per point, as the
      pass traces it; point-major), resident in device memory with their bounds: 56 bytes of loads per ray. Kernel time (HIP events); the copy up is not timed.
  c   pt_direct_device: kernel time.
  d   Renderer.direct_camera: wall time (aov + direct on the device, the sums copied back).
  b   wall time of the host path: Renderer.aov, the contract's rays and terms in numpy (tests/direct_restate.py, in slabs of 2^17 points),
      Renderer.rays(any_hit=True, t_max=...), the sum in numpy.
Kernel variants alternate inside one loop of one process after two warm-up rounds; min / median / max of --reps repetitions each. While timing, the results are
compared: the pass's sum and lit equal the hook's terms added in contract order where (a)'s flags are 0, in every bit, and so does the host path's sum."""
import argparse
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
from direct_restate import accumulate, is_point_light, restate  # noqa: E402

W, HT, SEED = 1920, 1080, 7
CASES = {"big-scene": 1, "macho-cows": 1, "soft-shadows": 16}
SLAB = 1 << 17


def summary(v):
    v = np.asarray(v)
    return dict(min=float(v.min()), median=float(np.median(v)), max=float(v.max()), n=int(len(v)))


def columns(lights, S):
    """which (light, sample) columns of the hook's n x L x S arrays are rays of their own: a point light's first, an area light's all"""
    return [(li, k) for li, l in enumerate(lights) for k in range(1 if is_point_light(l) else S)]


def spread(occ_cols, cols, lights, n, S):
    """(a)'s flags per distinct ray -> n x L x S, a point light's one flag under all of its S samples"""
    occ = np.zeros((n, len(lights), S), dtype=np.uint8)
    for c, (li, k) in enumerate(cols):
        if is_point_light(lights[li]):
            occ[:, li, :] = occ_cols[:, c][:, None]
        else:
            occ[:, li, k] = occ_cols[:, c]
    return occ


def host_path(r, sc, lights, eye, S):
    """Today's way: everything per ray crosses the bus. Returns (sum, wall seconds)."""
    t0 = time.perf_counter()
    aov = r.aov(sc.camera, W, HT, want=("position", "normal"))
    P, N = aov["position"].reshape(-1, 3), aov["normal"].reshape(-1, 3)
    n, cols = len(P), columns(lights, S)
    total = np.zeros((n, 3))
    for k in range(0, n, SLAB):
        O, D, T, E, valid = restate(P[k:k + SLAB], N[k:k + SLAB], lights, S, SEED, 0, k, 0.0, eye)
        m = len(O)
        sel = np.array(cols)
        oo = np.ascontiguousarray(np.repeat(O, len(cols), axis=0))
        dd = np.ascontiguousarray(D[:, sel[:, 0], sel[:, 1]].reshape(-1, 3))
        tt = np.ascontiguousarray(T[:, sel[:, 0], sel[:, 1]].ravel())
        occ = r.rays(oo, dd, any_hit=True, t_max=tt)["occluded"].reshape(m, len(cols))
        total[k:k + SLAB] = accumulate(T, E, valid, spread(occ, cols, lights, m, S))[0]
    return total, time.perf_counter() - t0


def measure(case, reps, with_host):
    S = CASES[case]
    lib = H.lib()
    sc = host.Scene.example(case)
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    c = r.context
    ex = sc.export()
    lights = np.ascontiguousarray(np.asarray(ex["lights"], dtype=np.float64).reshape(-1, 15)[:int(ex["n_lights"])])
    L, cols = len(lights), columns(lights, S)
    eye = np.array(list(host.camera(sc.camera, W, HT).eye))
    aov = r.aov(sc.camera, W, HT, want=("position", "normal"))
    P, N = np.ascontiguousarray(aov["position"].reshape(-1, 3)), np.ascontiguousarray(aov["normal"].reshape(-1, 3))
    n = len(P)
    p = H.PtDirectParams(n, S, 0, SEED, 0, 0.0, H.AO_FACE_EYE, (C.c_double * 3)(*eye))
    # the pass's rays and terms by the host replay, in slabs; the distinct rays point-major for (a)
    sel = np.array(cols)
    RO, RD, RT = np.zeros((n, len(cols), 3)), np.zeros((n, len(cols), 3)), np.zeros((n, len(cols)))
    T_all, E_all, valid = np.zeros((n, L, S)), np.zeros((n, L, S, 3)), np.zeros(n, dtype=np.uint8)
    dp = H._dp
    for k in range(0, n, SLAB):
        m = min(SLAB, n - k)
        ps = H.PtDirectParams(m, S, 0, SEED, k, 0.0, H.AO_FACE_EYE, (C.c_double * 3)(*eye))
        O, D, T, E, v = np.zeros((m, 3)), np.zeros((m, L, S, 3)), np.zeros((m, L, S)), np.zeros((m, L, S, 3)), np.zeros(m, dtype=np.uint8)
        assert lib.pt_test_direct_host(m, C.byref(ps), P[k:k + m].ctypes.data_as(dp), N[k:k + m].ctypes.data_as(dp), L, lights.ctypes.data_as(dp), O.ctypes.data_as(dp),
                                       D.ctypes.data_as(dp), T.ctypes.data_as(dp), E.ctypes.data_as(dp), v.ctypes.data_as(H._u8p)) == 0
        RO[k:k + m] = O[:, None, :]
        RD[k:k + m] = D[:, sel[:, 0], sel[:, 1]]
        RT[k:k + m] = T[:, sel[:, 0], sel[:, 1]]
        T_all[k:k + m], E_all[k:k + m], valid[k:k + m] = T, E, v
    n_rays = n * len(cols)

    def alloc(nbytes):
        ptr = C.c_void_p()
        assert lib.pt_device_alloc(c, nbytes, C.byref(ptr)) == 0, lib.pt_last_error(c)
        return ptr

    def upload(a):
        a = np.ascontiguousarray(a)
        ptr = alloc(a.nbytes)
        assert lib.pt_copy_to_device(c, ptr, a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
        return ptr

    def download(ptr, a):
        assert lib.pt_copy_from_device(c, a.ctypes.data_as(C.c_void_p), ptr, a.nbytes) == 0
        return a
    d_O, d_D, d_tm, d_flags = upload(RO), upload(RD), upload(RT), alloc(n_rays)
    d_P, d_N, d_sum, d_lit = upload(P), upload(N), alloc(n * 24), alloc(n * 4)
    del RO, RD
    ms = C.c_double(0.0)

    def segments():
        rp, rb = H.PtRaysParams(n_rays, 1, 0), H.PtRaysBuffers(occluded=C.cast(d_flags, H._u8p))
        assert lib.pt_segments_device(c, C.byref(rp), d_O, d_D, d_tm, C.byref(rb), None) == 0 and lib.pt_rays_finish(c, C.byref(ms)) == 0, lib.pt_last_error(c)
        return ms.value

    def direct():
        b = H.PtDirectBuffers(sum=C.cast(d_sum, dp), lit=C.cast(d_lit, H._up))
        assert lib.pt_direct_device(c, C.byref(p), d_P, d_N, C.byref(b), None) == 0 and lib.pt_direct_finish(c, C.byref(ms)) == 0, lib.pt_last_error(c)
        return ms.value
    variants = {"a": segments, "c": direct}
    segments()
    occ = spread(download(d_flags, np.zeros(n_rays, dtype=np.uint8)).reshape(n, len(cols)), cols, lights, n, S)
    want_sum, want_lit = accumulate(T_all, E_all, valid, occ)
    direct()
    assert download(d_sum, np.zeros((n, 3))).tobytes() == want_sum.tobytes(), "pt_direct's sum != the hook's terms where pt_segments sees the light"
    assert np.array_equal(download(d_lit, np.zeros(n, dtype=np.uint32)), want_lit)
    for _ in range(2):
        for fn in variants.values():
            fn()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t[k].append(fn())
    m = {k: summary(v) for k, v in t.items()}
    cast = int((RT > 0.0).sum())
    print("%s S=%d: %d points (%d valid), %d lights, %d distinct rays of which %d are cast, %d samples lit of %d" % (
        case, S, n, int(valid.sum()), L, n_rays, cast, int(want_lit.sum()), int(valid.sum()) * L * S))
    for k in variants:
        print("  %-14s %9.3f ms  [%.3f .. %.3f]   kernel" % (k, m[k]["median"], m[k]["min"], m[k]["max"]), flush=True)
    for ptr in (d_O, d_D, d_tm, d_flags, d_P, d_N, d_sum, d_lit):
        lib.pt_device_free(c, ptr)
    del T_all, E_all, occ
    if with_host:
        t0 = time.perf_counter()
        got = r.direct_camera(sc.camera, W, HT, samples=S, seed=SEED)
        m["d wall"] = dict(first_call_ms=(time.perf_counter() - t0) * 1e3)
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            got = r.direct_camera(sc.camera, W, HT, samples=S, seed=SEED)
            walls.append((time.perf_counter() - t0) * 1e3)
        assert got["sum"].reshape(-1, 3).tobytes() == want_sum.tobytes()
        m["d wall"].update(summary(walls))
        print("  %-14s %9.3f ms  [%.3f .. %.3f]   wall: aov + direct on the device, the sums copied back" % ("d direct_camera", m["d wall"]["median"], m["d wall"]["min"], m["d wall"]["max"]), flush=True)
        wall = []
        for _ in range(reps):
            total, sec = host_path(r, sc, lights, eye, S)
            assert total.tobytes() == want_sum.tobytes(), "the host path != pt_direct"
            wall.append(sec * 1e3)
        m["b wall"] = summary(wall)
        print("  %-14s %9.1f ms  [%.1f .. %.1f]   wall" % ("b host path", m["b wall"]["median"], m["b wall"]["min"], m["b wall"]["max"]), flush=True)
    r.close()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=list(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    result = {"width": W, "height": HT, "repetitions": a.reps, "cases": {}}
    for case in a.case or list(CASES):
        result["cases"][case] = measure(case, a.reps, not a.no_host)
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(result, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
