"""A numpy restatement of the probe pass's contract (portrayer_amd/csrc/pt_probe.h): steps 1 to 5 - which rays a probe casts and the nine basis
values of each - and step 6's order of summation. numpy's elementwise operations are separate correctly rounded f64 operations, nothing is contracted, so this
text and the functions the kernel compiles must agree in every bit (tests/test_probe_contract.py compares it with the host replay pt_test_probe_host); the GPU
tests shade these rays with Renderer.radiance and sum with project()."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_ao_contract import ROT, rng_f64  # noqa: E402  (PT_AO_ROT is reused as it is; pt_rng_f64 over arrays)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = (64, 128, 256, 512, 1024)


def header_tables():
    text = open(os.path.join(ROOT, "portrayer_amd", "csrc", "pt_probe_tables.h")).read()
    v = np.array([float.fromhex(x) for x in re.findall(r"-?0x[0-9a-f.]+p[+-]\d+", text)])
    assert v.size == 1024 * 3 + 5
    return v[:3072].reshape(1024, 3), v[3072:]


DIRS, SH = header_tables()


def stream_indices(n, first):
    """q = first_index + i modulo 2^64"""
    with np.errstate(over="ignore"):
        return np.uint64(first) + np.arange(n, dtype=np.uint64)


def restate(P, S, seed=0, pas=0, first=0):
    """Steps 1 to 5 in numpy: (origins (n, S, 3), directions (n, S, 3), basis (n, S, 9), valid (n,) u8); zeros at invalid probes."""
    P = np.asarray(P, dtype=np.float64)
    n = len(P)
    with np.errstate(all="ignore"):
        valid = np.all(np.abs(P) <= 1e18, axis=1)
        q = stream_indices(n, first)
        j = (rng_f64(seed, q, pas, 0) * 256.0).astype(np.uint32)
        m = (rng_f64(seed, q, pas, 1) * 1024.0).astype(np.uint32)
        c, s = ROT[j, 0][:, None], ROT[j, 1][:, None]
        N = DIRS[m]
        nn = N / np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])[:, None]
        x, y, z = DIRS[None, :S, 0], DIRS[None, :S, 1], DIRS[None, :S, 2]
        lx = c * x - s * y
        ly = s * x + c * y
        nx, ny, nz = nn[:, 0], nn[:, 1], nn[:, 2]
        sg = np.copysign(1.0, nz)
        a = -1.0 / (sg + nz)
        b = (nx * ny) * a
        T = np.stack([1.0 + ((sg * nx) * nx) * a, sg * b, -(sg * nx)], axis=1)
        B = np.stack([b, sg + (ny * ny) * a, -ny], axis=1)
        D = (T[:, None, :] * lx[:, :, None] + B[:, None, :] * ly[:, :, None]) + nn[:, None, :] * z[:, :, None]
        O = np.broadcast_to(P[:, None, :], D.shape).copy()
        dx, dy, dz = D[..., 0], D[..., 1], D[..., 2]
        c0, c1, c2, c3, c4 = SH
        Y = np.stack([np.full_like(dx, c0), c1 * dy, c1 * dz, c1 * dx, (c2 * dx) * dy, (c2 * dy) * dz, c3 * ((3.0 * dz) * dz - 1.0), (c2 * dx) * dz,
                      c4 * (dx * dx - dy * dy)], axis=-1)
    D[~valid] = 0.0
    O[~valid] = 0.0
    Y[~valid] = 0.0
    return O, D, Y, valid.astype(np.uint8)


def project(Y, rgb, valid):
    """Step 6 in numpy: Y (n, S, 9), rgb (n, S, 3) -> sh (n, 9, 3). Per round of 64 samples a partial from 0 in ascending k; round 0's partial plus the later
    rounds' in ascending round, left to right. Zeros at invalid probes."""
    n, S = Y.shape[:2]
    sh = None
    with np.errstate(all="ignore"):
        for r in range(S // 64):
            part = np.zeros((n, 9, 3))
            for k in range(64 * r, 64 * r + 64):
                part = part + Y[:, k, :, None] * rgb[:, k, None, :]
            sh = part if sh is None else sh + part
    sh[np.asarray(valid) == 0] = 0.0
    return sh
