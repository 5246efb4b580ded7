"""The contract of the direct-light pass (pt_direct, include/portrayer_hip.h) in numpy, written from the header's comments: numpy's elementwise
operations are separate correctly rounded f64 operations and nothing is contracted. tests/test_direct_contract.py compares it with the host replay of the
functions the kernel compiles; tests/test_gpu_direct.py adds its terms in contract order, with visibility from Renderer.rays, as the oracle of the kernel."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_ao_contract import rng_f64  # noqa: E402

EPSILON = 0.00001  # PT_EPSILON


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def is_point_light(light):
    """Step 5: an area vector that is all zero (either sign)."""
    return bool(np.all(light[9:12] == 0.0) or np.all(light[12:15] == 0.0))


def restate(P, N, lights, S, seed=0, pas=0, first=0, bias=0.0, eye=None, to_light=False, normalise=True):
    """Steps 1 to 7 and 9, and step 8's rule for which rays are traced: (origins (n, 3), directions (n, L, S, 3), t_max (n, L, S), terms (n, L, S, 3), valid (n,)).
    A sample that casts no ray has direction, t_max and term 0. normalise=False leaves step 3 out (for normals that are unit already)."""
    P, N = np.asarray(P, dtype=np.float64), np.asarray(N, dtype=np.float64)
    lights = np.asarray(lights, dtype=np.float64).reshape(-1, 15)
    n, L = len(P), len(lights)
    D, T, E = np.zeros((n, L, S, 3)), np.zeros((n, L, S)), np.zeros((n, L, S, 3))
    with np.errstate(all="ignore"):
        valid = np.all(np.abs(P) <= 1e18, axis=1) & np.all(np.abs(N) <= 1e18, axis=1) & ~np.all(N == 0.0, axis=1)  # 1
        if eye is not None:  # 2
            v = P - np.asarray(eye, dtype=np.float64)[None, :]
            N = np.where((dot(N, v) > 0.0)[:, None], -N, N)
        nrm = N / np.sqrt(dot(N, N))[:, None] if normalise else N  # 3
        O = P + nrm * bias  # 4
        q = np.uint64(first) + np.arange(n, dtype=np.uint64)
        j = 0
        for li, light in enumerate(lights):
            pos, colour, (c0, c1, c2), a, b = light[0:3], light[3:6], light[6:9], light[9:12], light[12:15]
            for k in range(S):
                if is_point_light(light):  # 5
                    lpos = np.broadcast_to(pos, (n, 3))
                else:
                    stream = q * np.uint64(S) + np.uint64(k)  # modulo 2^64
                    ca = 2.0 * rng_f64(seed, stream, pas, 2 * j) - 1.0
                    cb = 2.0 * rng_f64(seed, stream, pas, 2 * j + 1) - 1.0
                    lpos = pos[None, :] + (a[None, :] * ca[:, None] + b[None, :] * cb[:, None])
                v = lpos - O  # 6
                dist = np.sqrt(dot(v, v))
                d = v / dist[:, None]
                tm = dist if to_light else np.full(n, np.inf)
                c = np.fmax(dot(nrm, d), 0.0)  # 7
                traced = np.all(np.abs(O) <= 1e18, axis=1) & np.all(np.abs(d) <= 1e18, axis=1) & (tm > EPSILON)  # 8: pt_segments' rule
                casts = valid & (c > 0.0) & traced
                att = (c0 + c1 * dist) + (c2 * dist) * dist  # 9
                term = (colour[None, :] * c[:, None]) / att[:, None]
                D[casts, li, k] = d[casts]
                T[casts, li, k] = tm[casts]
                E[casts, li, k] = term[casts]
            if not is_point_light(light):
                j += 1
    O = np.where(valid[:, None], O, 0.0)
    return O, D, T, E, valid.astype(np.uint8)


def accumulate(T, E, valid, occluded):
    """Step 10: (sum (n, 3), lit (n,)) from the restatement's t_max and terms and `occluded` (n, L, S), a ray query's answer for the restatement's rays. A
    point light's S samples are equal, so adding them one by one is adding the one S times."""
    n, L, S = T.shape
    total, lit = np.zeros((n, 3)), np.zeros(n, dtype=np.uint32)
    for li in range(L):
        for k in range(S):
            add = (T[:, li, k] > 0.0) & (np.asarray(occluded)[:, li, k] == 0) & (np.asarray(valid) != 0)
            total = np.where(add[:, None], total + E[:, li, k], total)
            lit += add.astype(np.uint32)
    return total, lit
