#!/usr/bin/env python3
"""What the gather pass costs, against the two ways there were before it: python3 profiles/gather/measure.py [--case NAME] [--reps 5] [--no-host] [--out F.json]

1920x1080, 16 rays per pixel, flat traversal, background (0.25, 0.5, 1). Cases: big-scene, macho-cows, transmission-refraction (default all three). The points are
the pixel centres' first hits (Renderer.aov), the normals turned to the eye: what Renderer.gather_camera shades. Per case:
  a r0 / r1  pt_radiance_device on the very rays the pass makes (the host replay pt_test_ao_rays_host writes them, point-major = the pass's order), resident in
             device memory, stream_base 0, reorder 0 and 1: 48 bytes of loads and 24 of stores per ray. Kernel time (HIP events; with reorder = 1 keying and sort
             are inside it); the copy up is not timed.
  c          pt_gather_device: kernel time.
  d          Renderer.gather_camera: wall time (aov + gather on the device, the sums copied back).
  b          wall time of the host path: Renderer.aov, the contract's rays in numpy (the restatement of tests/test_ao_contract.py, in slabs of 2^17 points),
             Renderer.radiance, the sum per channel in numpy. Its radiance pass's kernel_ms is reported beside the wall time.
Kernel variants alternate inside one loop of one process after two warm-up rounds; median [min .. max] of --reps repetitions each. While timing, the results are
compared: the pass's sums equal (a)'s colours added in order, in every bit, and so do gather_camera's and the host path's."""
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
from scene_dsl import ASSETS  # noqa: E402
from test_ao_contract import restate  # noqa: E402

W, HT, S, SEED = 1920, 1080, 16, 7
BG = np.array([0.25, 0.5, 1.0])
CASES = ("big-scene", "macho-cows", "transmission-refraction")


def summary(v):
    v = np.asarray(v)
    return dict(min=float(v.min()), median=float(np.median(v)), max=float(v.max()), n=int(len(v)))


def add_in_order(rgb, valid):
    """(n, S, 3) colours -> (n, 3): from zero, ascending k, per channel; zeros at invalid points"""
    total = np.zeros((rgb.shape[0], 3))
    for k in range(rgb.shape[1]):
        total += rgb[:, k, :]
    total[valid == 0] = 0.0
    return total


def host_path(r, sc, eye):
    """Today's way: everything per ray crosses the bus. Returns (sums, wall seconds, the radiance pass's kernel ms)."""
    t0 = time.perf_counter()
    aov = r.aov(sc.camera, W, HT, want=("position", "normal"))
    P, N = aov["position"].reshape(-1, 3), aov["normal"].reshape(-1, 3)
    n = len(P)
    O, D, valid = np.empty((n, S, 3)), np.empty((n, S, 3)), np.empty(n, dtype=bool)
    for k in range(0, n, 1 << 17):
        O[k:k + (1 << 17)], D[k:k + (1 << 17)], valid[k:k + (1 << 17)] = restate(P[k:k + (1 << 17)], N[k:k + (1 << 17)], S, SEED, 0, k, 0.0, eye)
    got = r.radiance(O.reshape(-1, 3), D.reshape(-1, 3), BG, seed=SEED, sample=0, stream_base=0)
    total = add_in_order(got["rgb"].reshape(n, S, 3), valid)
    return total, time.perf_counter() - t0, got["kernel_ms"]


def measure(scene_name, reps, with_host):
    lib = H.lib()
    sc = host.Scene.example(scene_name, assets=ASSETS)
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    c = r.context
    eye = np.array(list(host.camera(sc.camera, W, HT).eye))
    aov = r.aov(sc.camera, W, HT, want=("position", "normal"))
    P, N = np.ascontiguousarray(aov["position"].reshape(-1, 3)), np.ascontiguousarray(aov["normal"].reshape(-1, 3))
    n = len(P)
    ap = H.PtAoParams(n, S, 0, SEED, 0, float("inf"), 0.0, H.AO_FACE_EYE, (C.c_double * 3)(*eye))
    O, D, valid = np.zeros((n, S, 3)), np.zeros((n, S, 3)), np.zeros(n, dtype=np.uint8)
    assert lib.pt_test_ao_rays_host(n, C.byref(ap), P.ctypes.data_as(H._dp), N.ctypes.data_as(H._dp), O.ctypes.data_as(H._dp), D.ctypes.data_as(H._dp), valid.ctypes.data_as(H._u8p)) == 0

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
    d_O, d_D, d_rgb, d_bg = upload(O), upload(D), alloc(n * S * 24), upload(BG)
    d_P, d_N, d_sum = upload(P), upload(N), alloc(n * 24)
    del O, D
    ms = C.c_double(0.0)
    gp = H.PtGatherParams(n, S, 0, SEED, 0, 0.0, H.AO_FACE_EYE, (C.c_double * 3)(*eye))

    def radiance(reorder):
        rp = H.PtRadianceParams(n * S, reorder, 0, SEED, 0, 0)
        assert lib.pt_radiance_device(c, C.byref(rp), d_O, d_D, d_bg, d_rgb, None) == 0 and lib.pt_radiance_finish(c, C.byref(ms)) == 0, lib.pt_last_error(c)
        return ms.value

    def gather():
        b = H.PtGatherBuffers(sum=C.cast(d_sum, H._dp))
        assert lib.pt_gather_device(c, C.byref(gp), d_P, d_N, BG.ctypes.data_as(H._dp), C.byref(b), None) == 0 and lib.pt_gather_finish(c, C.byref(ms)) == 0, lib.pt_last_error(c)
        return ms.value
    variants = {"a r0": lambda: radiance(0), "a r1": lambda: radiance(1), "c": gather}
    radiance(0)
    want = add_in_order(download(d_rgb, np.zeros((n, S, 3))), valid)
    gather()
    assert download(d_sum, np.zeros((n, 3))).tobytes() == want.tobytes(), "pt_gather != pt_radiance on the same rays, added in order"
    for _ in range(2):
        for fn in variants.values():
            fn()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t[k].append(fn())
    m = {k: summary(v) for k, v in t.items()}
    shaded = int(((want != (BG * S)[None, :]).any(axis=1) & (valid == 1)).sum())
    print("%s: %d points (%d valid, %d with a sum other than %d x background), %d rays" % (scene_name, n, int(valid.sum()), shaded, S, n * S))
    for k in variants:
        print("  %-15s %9.3f ms  [%.3f .. %.3f]   kernel" % (k, m[k]["median"], m[k]["min"], m[k]["max"]), flush=True)
    for ptr in (d_O, d_D, d_rgb, d_bg, d_P, d_N, d_sum):
        lib.pt_device_free(c, ptr)
    if with_host:
        t0 = time.perf_counter()
        got = r.gather_camera(sc.camera, W, HT, BG, samples=S, seed=SEED)
        m["d wall"] = dict(first_call_ms=(time.perf_counter() - t0) * 1e3)
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            got = r.gather_camera(sc.camera, W, HT, BG, samples=S, seed=SEED)
            walls.append((time.perf_counter() - t0) * 1e3)
        assert got["sum"].tobytes() == want.tobytes()
        m["d wall"].update(summary(walls))
        print("  %-15s %9.3f ms  [%.3f .. %.3f]   wall: aov + gather on the device, the sums copied back" % ("d gather_camera", m["d wall"]["median"], m["d wall"]["min"], m["d wall"]["max"]), flush=True)
        wall, kern = [], []
        for _ in range(reps):
            total, sec, kms = host_path(r, sc, eye)
            assert total.tobytes() == want.tobytes(), "the host path != pt_radiance on the same rays"
            wall.append(sec * 1e3)
            kern.append(kms)
        m["b wall"], m["b kernel"] = summary(wall), summary(kern)
        print("  %-15s %9.1f ms  [%.1f .. %.1f]   wall; its radiance pass's kernel %.3f ms [%.3f .. %.3f]" % (
            "b host path", m["b wall"]["median"], m["b wall"]["min"], m["b wall"]["max"], m["b kernel"]["median"], m["b kernel"]["min"], m["b kernel"]["max"]), flush=True)
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
