#!/usr/bin/env python3
"""What the ambient-occlusion pass costs, against the two ways there were before it: python3 profiles/ao/measure.py [--case NAME] [--reps 5] [--no-host] [--out F.json]

1920x1080, 16 rays per pixel, flat traversal. Cases: big-scene with radius inf, macho-cows with radius inf and with radius 1 (--case big-scene:inf, macho-cows:inf,
macho-cows:1; default all three). The points are the pixel centres' first hits (Renderer.aov), the normals turned to the eye: what Renderer.ao_camera traces. Per case:
  a          pt_segments_device, any_hit = 1, on the very rays the pass makes (the host replay pt_test_ao_rays_host writes them, point-major = the pass's point-major
             order), resident in device memory with their bounds: 56 bytes of loads per ray. Kernel time (HIP events); the copy up is not timed.
  a r1       the same with reorder = 1 (keying and sort inside the kernel time).
  c point    pt_ao_device, PORTRAYER_AO_LAYOUT=point: kernel time.
  c sample   pt_ao_device, PORTRAYER_AO_LAYOUT=sample.
  c +bent    the two layouts again with the bent normal asked for beside the count.
  b r0 / r1  wall time of the host path: Renderer.aov, the contract's rays in numpy (the restatement of tests/test_ao_contract.py, in slabs of 2^17 points),
             Renderer.rays(any_hit=True, t_max=radius, reorder=0 / 1), the count in numpy. Its kernel_ms is reported beside the wall time.
Kernel variants alternate inside one loop of one process after two warm-up rounds; min / median / max of --reps repetitions each. While timing, the results are
compared: the pass's counts equal the sums of (a)'s flags in both layouts, and the host path's."""
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
from test_ao_contract import restate  # noqa: E402

W, HT, S, SEED = 1920, 1080, 16, 7
CASES = ("big-scene:inf", "macho-cows:inf", "macho-cows:1")


def summary(v):
    v = np.asarray(v)
    return dict(min=float(v.min()), median=float(np.median(v)), max=float(v.max()), n=int(len(v)))


def host_path(r, sc, eye, radius, reorder):
    """Today's way: everything per ray crosses the bus. Returns (counts, wall seconds, the ray pass's kernel ms)."""
    t0 = time.perf_counter()
    aov = r.aov(sc.camera, W, HT, want=("position", "normal"))
    P, N = aov["position"].reshape(-1, 3), aov["normal"].reshape(-1, 3)
    n = len(P)
    O, D = np.empty((n, S, 3)), np.empty((n, S, 3))
    for k in range(0, n, 1 << 17):
        O[k:k + (1 << 17)], D[k:k + (1 << 17)], _ = restate(P[k:k + (1 << 17)], N[k:k + (1 << 17)], S, SEED, 0, k, 0.0, eye)
    got = r.rays(O.reshape(-1, 3), D.reshape(-1, 3), any_hit=True, reorder=reorder, t_max=float(radius))
    counts = got["occluded"].reshape(n, S).sum(axis=1, dtype=np.uint32)
    return counts, time.perf_counter() - t0, got["kernel_ms"]


def measure(case, reps, with_host):
    scene_name, radius = case.split(":")
    radius = float(radius)
    lib = H.lib()
    sc = host.Scene.example(scene_name)
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    c = r.context
    eye = np.array(list(host.camera(sc.camera, W, HT).eye))
    aov = r.aov(sc.camera, W, HT, want=("position", "normal"))
    P, N = np.ascontiguousarray(aov["position"].reshape(-1, 3)), np.ascontiguousarray(aov["normal"].reshape(-1, 3))
    n = len(P)
    p = H.PtAoParams(n, S, 0, SEED, 0, radius, 0.0, H.AO_FACE_EYE, (C.c_double * 3)(*eye))
    O, D, valid = np.zeros((n, S, 3)), np.zeros((n, S, 3)), np.zeros(n, dtype=np.uint8)
    assert lib.pt_test_ao_rays_host(n, C.byref(p), P.ctypes.data_as(H._dp), N.ctypes.data_as(H._dp), O.ctypes.data_as(H._dp), D.ctypes.data_as(H._dp), valid.ctypes.data_as(H._u8p)) == 0

    def alloc(nbytes):
        ptr = C.c_void_p()
        assert lib.pt_device_alloc(c, nbytes, C.byref(ptr)) == 0, lib.pt_last_error(c)
        return ptr

    def upload(a):
        ptr = alloc(a.nbytes)
        assert lib.pt_copy_to_device(c, ptr, a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
        return ptr

    def download(ptr, a):
        assert lib.pt_copy_from_device(c, a.ctypes.data_as(C.c_void_p), ptr, a.nbytes) == 0
        return a
    d_O, d_D, d_tm, d_flags = upload(O), upload(D), upload(np.full(n * S, radius)), alloc(n * S)
    d_P, d_N, d_occ, d_bent = upload(P), upload(N), alloc(n * 4), alloc(n * 24)
    del O, D
    ms = C.c_double(0.0)

    def segments(reorder):
        rp, rb = H.PtRaysParams(n * S, 1, reorder), H.PtRaysBuffers(occluded=C.cast(d_flags, H._u8p))
        assert lib.pt_segments_device(c, C.byref(rp), d_O, d_D, d_tm, C.byref(rb), None) == 0 and lib.pt_rays_finish(c, C.byref(ms)) == 0, lib.pt_last_error(c)
        return ms.value

    def ao(layout, bent):
        os.environ["PORTRAYER_AO_LAYOUT"] = layout
        b = H.PtAoBuffers(occluded=C.cast(d_occ, H._up), bent=C.cast(d_bent, H._dp) if bent else None)
        assert lib.pt_ao_device(c, C.byref(p), d_P, d_N, C.byref(b), None) == 0 and lib.pt_ao_finish(c, C.byref(ms)) == 0, lib.pt_last_error(c)
        return ms.value
    variants = {"a": lambda: segments(0), "a r1": lambda: segments(1), "c point": lambda: ao("point", False), "c sample": lambda: ao("sample", False),
                "c point +bent": lambda: ao("point", True), "c sample +bent": lambda: ao("sample", True)}
    segments(0)
    want = download(d_flags, np.zeros(n * S, dtype=np.uint8)).reshape(n, S).sum(axis=1, dtype=np.uint32)
    for layout in ("point", "sample"):
        ao(layout, True)
        assert np.array_equal(download(d_occ, np.zeros(n, dtype=np.uint32)), want), "pt_ao (%s) != pt_segments on the same rays" % layout
    for _ in range(2):
        for fn in variants.values():
            fn()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t[k].append(fn())
    m = {k: summary(v) for k, v in t.items()}
    part = int(((want > 0) & (want < S) & (valid == 1)).sum())
    print("%s radius %g: %d points (%d valid, %d with 0 < occluded < %d), %d rays, occluded share %.3f" % (scene_name, radius, n, int(valid.sum()), part, S, n * S, want.sum() / (S * max(int(valid.sum()), 1))))
    for k in variants:
        print("  %-15s %9.3f ms  [%.3f .. %.3f]   kernel" % (k, m[k]["median"], m[k]["min"], m[k]["max"]), flush=True)
    for ptr in (d_O, d_D, d_tm, d_flags, d_P, d_N, d_occ, d_bent):
        lib.pt_device_free(c, ptr)
    if with_host:
        os.environ.pop("PORTRAYER_AO_LAYOUT", None)
        t0 = time.perf_counter()
        got = r.ao_camera(sc.camera, W, HT, samples=S, radius=radius, seed=SEED)
        m["ao_camera wall"] = dict(first_call_ms=(time.perf_counter() - t0) * 1e3)
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            got = r.ao_camera(sc.camera, W, HT, samples=S, radius=radius, seed=SEED)
            walls.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(got["occluded"].ravel(), want)
        m["ao_camera wall"].update(summary(walls))
        print("  %-15s %9.3f ms  [%.3f .. %.3f]   wall: aov + ao on the device, the counts copied back" % ("ao_camera", m["ao_camera wall"]["median"], m["ao_camera wall"]["min"], m["ao_camera wall"]["max"]), flush=True)
        for ro in (0, 1):
            wall, kern = [], []
            for _ in range(reps):
                counts, sec, kms = host_path(r, sc, eye, radius, bool(ro))
                assert np.array_equal(counts, want), "the host path != pt_segments on the same rays"
                wall.append(sec * 1e3)
                kern.append(kms)
            m["b r%d wall" % ro], m["b r%d kernel" % ro] = summary(wall), summary(kern)
            print("  %-15s %9.1f ms  [%.1f .. %.1f]   wall; its ray pass's kernel %.3f ms [%.3f .. %.3f]" % (
                "b r%d" % ro, m["b r%d wall" % ro]["median"], m["b r%d wall" % ro]["min"], m["b r%d wall" % ro]["max"], m["b r%d kernel" % ro]["median"], m["b r%d kernel" % ro]["min"],
                m["b r%d kernel" % ro]["max"]), flush=True)
    r.close()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=CASES)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    result = {"width": W, "height": HT, "samples": S, "repetitions": a.reps, "cases": {}}
    for case in a.case or CASES:
        result["cases"][case] = measure(case, a.reps, not a.no_host)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
