#!/usr/bin/env python3
"""What the probe pass costs, against the two ways there were before it: python3 profiles/probe/measure.py [--case NAME] [--samples S] [--reps 5] [--no-host] [--out F.json]

4,096 probes at S = 256 and at S = 1024 rays each, flat traversal, background (0.25, 0.5, 1). Cases: big-scene, macho-cows, transmission-refraction (default all
three). The probes are first hits under a 128 x 128 image (Renderer.aov), 4,096 taken evenly, each lifted 0.25 along its normal into free space. Per case and S:
  a r0 / r1  pt_radiance_device on the very rays the pass makes (the host replay pt_test_probe_host writes them, probe-major = the pass's order), resident in
             device memory, stream_base 0, reorder 0 and 1: 48 bytes of loads and 24 of stores per ray. Kernel time (HIP events; with reorder = 1 keying and sort
             are inside it); the copy up is not timed.
  c          pt_probe_device: kernel time, the fold over the rounds inside it.
  c valid    pt_probe_device asked for `valid` alone: nothing is traced, no tail and no fold - what the pass costs before its first ray.
  d          Renderer.probe: wall time (24 bytes per probe up, 216 down, coeffs = sh * 4 pi / S in numpy).
  b          wall time of the host path: the contract's rays and basis values in numpy (tests/probe_restate.py), Renderer.radiance, the projection in numpy in the
             contract's order. Its radiance pass's kernel_ms is reported beside the wall time.
Kernel variants alternate inside one loop of one process after two warm-up rounds; median [min .. max] of --reps repetitions each. While timing, the results are
compared on every probe: the pass's sums equal (a)'s colours weighted and added in the contract's order, in every bit, and so do Renderer.probe's and the host
path's. The fold kernel's own time is not between events of its own: run this script under a kernel trace (rocprofv3 --kernel-trace --stats) to read it."""
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
from probe_restate import project, restate  # noqa: E402
from scene_dsl import ASSETS  # noqa: E402

NPROBES, SEED = 4096, 7
BG = np.array([0.25, 0.5, 1.0])
CASES = ("big-scene", "macho-cows", "transmission-refraction")


def summary(v):
    v = np.asarray(v)
    return dict(min=float(v.min()), median=float(np.median(v)), max=float(v.max()), n=int(len(v)))


def probes_of(r, sc):
    aov = r.aov(sc.camera, 128, 128, want=("position", "normal", "node"))
    hit = np.flatnonzero(aov["node"].ravel() >= 0)
    assert len(hit) >= NPROBES, "the image has fewer than %d hits" % NPROBES
    take = hit[np.linspace(0, len(hit) - 1, NPROBES).astype(int)]
    return np.ascontiguousarray(aov["position"].reshape(-1, 3)[take] + 0.25 * aov["normal"].reshape(-1, 3)[take])


def host_path(r, P, S):
    """Today's way: everything per ray crosses the bus. Returns (sh, wall seconds, the radiance pass's kernel ms)."""
    t0 = time.perf_counter()
    O, D, Y, valid = restate(P, S, SEED, 0, 0)
    n = len(P)
    got = r.radiance(O.reshape(-1, 3), D.reshape(-1, 3), BG, seed=SEED, sample=0, stream_base=0)
    sh = project(Y, got["rgb"].reshape(n, S, 3), valid)
    return sh, time.perf_counter() - t0, got["kernel_ms"]


def measure(scene_name, S, reps, with_host):
    lib = H.lib()
    sc = host.Scene.example(scene_name, assets=ASSETS)
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    c = r.context
    P = probes_of(r, sc)
    n = len(P)
    pp = H.PtProbeParams(n, S, 0, SEED, 0)
    O, D, Y, valid = np.zeros((n, S, 3)), np.zeros((n, S, 3)), np.zeros((n, S, 9)), np.zeros(n, dtype=np.uint8)
    dp = lambda a: a.ctypes.data_as(H._dp)
    assert lib.pt_test_probe_host(n, C.byref(pp), dp(P), dp(O), dp(D), dp(Y), valid.ctypes.data_as(H._u8p)) == 0

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
    d_P, d_sh, d_valid = upload(P), alloc(n * 216), alloc(n)
    del O, D
    ms = C.c_double(0.0)

    def radiance(reorder):
        rp = H.PtRadianceParams(n * S, reorder, 0, SEED, 0, 0)
        assert lib.pt_radiance_device(c, C.byref(rp), d_O, d_D, d_bg, d_rgb, None) == 0 and lib.pt_radiance_finish(c, C.byref(ms)) == 0, lib.pt_last_error(c)
        return ms.value

    def probe(want_sh=True):
        b = H.PtProbeBuffers(sh=C.cast(d_sh, H._dp)) if want_sh else H.PtProbeBuffers(valid=C.cast(d_valid, H._u8p))
        assert lib.pt_probe_device(c, C.byref(pp), d_P, dp(BG), C.byref(b), None) == 0 and lib.pt_probe_finish(c, C.byref(ms)) == 0, lib.pt_last_error(c)
        return ms.value
    variants = {"a r0": lambda: radiance(0), "a r1": lambda: radiance(1), "c": probe, "c valid": lambda: probe(False)}
    radiance(0)
    want = project(Y, download(d_rgb, np.zeros((n, S, 3))), valid)
    probe()
    assert download(d_sh, np.zeros((n, 9, 3))).tobytes() == want.tobytes(), "pt_probe != pt_radiance on the same rays, weighted and added in order"
    for _ in range(2):
        for fn in variants.values():
            fn()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t[k].append(fn())
    m = {k: summary(v) for k, v in t.items()}
    sky = project(Y, np.broadcast_to(BG, (n, S, 3)), valid)
    shaded = int((want != sky).reshape(n, -1).any(axis=1).sum())
    print("%s S=%d: %d probes (%d valid, %d with sums other than the all-background answer), %d rays" % (scene_name, S, n, int(valid.sum()), shaded, n * S))
    for k in variants:
        print("  %-15s %9.3f ms  [%.3f .. %.3f]   kernel" % (k, m[k]["median"], m[k]["min"], m[k]["max"]), flush=True)
    for ptr in (d_O, d_D, d_rgb, d_bg, d_P, d_sh, d_valid):
        lib.pt_device_free(c, ptr)
    if with_host:
        t0 = time.perf_counter()
        got = r.probe(P, BG, samples=S, seed=SEED)
        m["d wall"] = dict(first_call_ms=(time.perf_counter() - t0) * 1e3)
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            got = r.probe(P, BG, samples=S, seed=SEED)
            walls.append((time.perf_counter() - t0) * 1e3)
        assert got["sh"].tobytes() == want.tobytes()
        m["d wall"].update(summary(walls))
        print("  %-15s %9.3f ms  [%.3f .. %.3f]   wall: positions up, the pass, 216 bytes per probe back" % ("d Renderer.probe", m["d wall"]["median"], m["d wall"]["min"], m["d wall"]["max"]), flush=True)
        wall, kern = [], []
        for _ in range(min(reps, 3)):
            sh, sec, kms = host_path(r, P, S)
            assert sh.tobytes() == want.tobytes(), "the host path != pt_radiance on the same rays"
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
    ap.add_argument("--samples", action="append", type=int, choices=H.PROBE_SAMPLES)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    result = {"probes": NPROBES, "repetitions": a.reps, "cases": {}}
    for case in a.case or CASES:
        for S in a.samples or (256, 1024):
            result["cases"]["%s S=%d" % (case, S)] = measure(case, S, a.reps, not a.no_host)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
