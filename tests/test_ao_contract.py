"""The contract of the ambient-occlusion pass without a GPU (portrayer_amd/csrc/pt_ao.h): a numpy restatement of its steps 1 to 8 - numpy's
elementwise operations are separate correctly rounded f64 operations, nothing is contracted - against the host replay pt_test_ao_rays_host, which compiles the
functions the kernel compiles, in every bit; the tables against the header and their generator; and the properties the tables and the frame are chosen for."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = (1, 2, 4, 8, 16, 32, 64)
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def header_tables():
    text = open(os.path.join(ROOT, "portrayer_amd", "csrc", "pt_ao_tables.h")).read()
    v = np.array([float.fromhex(x) for x in re.findall(r"-?0x[0-9a-f.]+p[+-]\d+", text)])
    assert v.size == 64 * 3 + 256 * 2
    return v[:192].reshape(64, 3), v[192:].reshape(256, 2)


DIRS, ROT = header_tables()


def mix64(z):
    z = z ^ (z >> np.uint64(30)); z = z * np.uint64(0xbf58476d1ce4e5b9)
    z = z ^ (z >> np.uint64(27)); z = z * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def rng_f64(seed, index, sample, draw):
    """pt_rng_f64 (csrc/pt_math.h) over an array of stream indices; uint64 arithmetic wraps"""
    with np.errstate(over="ignore"):
        k = mix64(np.array([seed], dtype=np.uint64) + np.uint64(0x9e3779b97f4a7c15))
        key = mix64(k ^ (index.astype(np.uint64) * np.uint64(0xd1342543de82ef95) + np.uint64(0x632be59bd9b4e019)))
        r = mix64(key ^ np.uint64((sample << 32) | draw))
    return (r >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def restate(P, N, S, seed=0, pas=0, first=0, bias=0.0, eye=None):
    """Steps 1 to 8 in numpy: (origins (n, S, 3), directions (n, S, 3), valid (n,)); zeros at invalid points."""
    n = len(P)
    with np.errstate(all="ignore"):
        valid = np.all(np.abs(P) <= 1e18, axis=1) & np.all(np.abs(N) <= 1e18, axis=1) & ~np.all(N == 0.0, axis=1)
        if eye is not None:
            v = P - np.asarray(eye, dtype=np.float64)[None, :]
            dot = (N[:, 0] * v[:, 0] + N[:, 1] * v[:, 1]) + N[:, 2] * v[:, 2]
            N = np.where((dot > 0.0)[:, None], -N, N)
        nn = N / np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])[:, None]
        j = (rng_f64(seed, first + np.arange(n, dtype=np.uint64), pas, 0) * 256.0).astype(np.uint32)
        c, s = ROT[j, 0][:, None], ROT[j, 1][:, None]
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
        O = np.broadcast_to((P + nn * bias)[:, None, :], D.shape).copy()
    D[~valid] = 0.0
    O[~valid] = 0.0
    return O, D, valid.astype(np.uint8)


def replay(H, P, N, S, seed=0, pas=0, first=0, bias=0.0, eye=None):
    n = len(P)
    P, N = np.ascontiguousarray(P), np.ascontiguousarray(N)
    e = (0.0, 0.0, 0.0) if eye is None else tuple(float(v) for v in eye)
    p = H.PtAoParams(n, S, pas, seed, first, float("inf"), bias, H.AO_FACE_EYE if eye is not None else 0, (C.c_double * 3)(*e))
    O, D, valid = np.full((n, S, 3), 7.0), np.full((n, S, 3), 7.0), np.full(n, 7, dtype=np.uint8)
    rc = H.lib().pt_test_ao_rays_host(n, C.byref(p), P.ctypes.data_as(H._dp), N.ctypes.data_as(H._dp), O.ctypes.data_as(H._dp), D.ctypes.data_as(H._dp), valid.ctypes.data_as(H._u8p))
    assert rc == 0
    return O, D, valid


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.fixture(scope="module")
def points():
    """4,096 random points and normals of any length, then the corners of the frame and of the validity rule"""
    rng = np.random.default_rng(20261)
    P = rng.uniform(-50.0, 50.0, (4096, 3))
    N = rng.normal(size=(4096, 3)) * np.exp(rng.uniform(-3.0, 3.0, (4096, 1)))
    special = [(0.6, 0.8, 0.0), (0.6, 0.8, -0.0), (-0.6, -0.8, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (-0.0, -0.0, 1.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0),
               (0.0, -1.0, 0.0), (1.0, 0.0, -0.0), (3e-5, -8e-5, 5e-5), (6e5, 3e5, -7e5), (1e-4, 0.0, 0.0), (0.0, 0.0, -1e6), (1e-9, 1e-9, -1.0), (1e-9, -1e-9, 1.0),
               (0.0, 0.0, 0.0), (np.nan, 0.0, 1.0), (0.0, np.inf, 1.0), (0.0, 1.0, -np.inf), (2e18, 0.0, 1.0), (0.0, 1.0, -2e18), (1e18, 0.0, 0.0), (-0.0, 0.0, -0.0)]
    sp = np.array(special)
    P = np.vstack([P, rng.uniform(-5.0, 5.0, (len(sp), 3)), [[np.nan, 0.0, 0.0], [0.0, -np.inf, 0.0], [0.0, 0.0, 2e18], [1e18, -1e18, 1e18]]])
    N = np.vstack([N, sp, [[0.0, 0.0, 1.0]] * 4])
    return P, N


def test_the_librarys_tables_are_the_headers_and_the_generator_agrees(H):
    dirs, rot = np.zeros((64, 3)), np.zeros((256, 2))
    assert H.lib().pt_test_ao_tables(dirs.ctypes.data_as(H._dp), rot.ctypes.data_as(H._dp)) == 0
    assert same_bits(dirs, DIRS) and same_bits(rot, ROT)
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ao_tables.py"), "--check"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr


def test_the_directions_are_unit_above_the_plane_cosine_weighted_and_stratified_in_every_prefix():
    assert np.abs(np.sqrt((DIRS * DIRS).sum(1)) - 1.0).max() <= 1e-15 and np.abs(np.sqrt((ROT * ROT).sum(1)) - 1.0).max() <= 1e-15
    assert DIRS[:, 2].min() > 0.0
    assert abs(DIRS[:, 2].mean() - 2.0 / 3.0) < 1e-3, "the mean of cos(theta) under a cosine-weighted density is 2/3"
    for S in SAMPLES:
        u = 1.0 - DIRS[:S, 2] * DIRS[:S, 2]
        assert sorted(np.floor(u * S).astype(int)) == list(range(S)), "one direction per stratum [m/S, (m+1)/S) of u at S = %d" % S
        phi = np.arctan2(DIRS[:S, 1], DIRS[:S, 0]) / (2.0 * np.pi) % 1.0
        assert sorted(np.floor(phi * S).astype(int)) == list(range(S)), "and of the azimuth"


@pytest.mark.parametrize("S", SAMPLES)
def test_the_restatement_equals_the_host_replay_in_every_bit(H, points, S):
    P, N = points
    for seed, pas, bias, eye in ((0, 0, 0.0, None), (7, 1, 1e-3, None), (7, 0, 0.0, (0.5, -60.0, 2.0)), (0x9e3779b97f4a7c15, 3, 0.25, (0.0, 60.0, -1.0))):
        O, D, valid = restate(P, N, S, seed, pas, 0, bias, eye)
        O2, D2, valid2 = replay(H, P, N, S, seed, pas, 0, bias, eye)
        assert np.array_equal(valid, valid2)
        assert same_bits(D, D2), (S, seed, pas, eye)
        assert same_bits(O, O2), (S, seed, pas, eye)


def test_validity_is_the_ray_queries_rule_and_a_zero_normal(H, points):
    P, N = points
    O, D, valid = replay(H, P, N, 4)
    assert valid[:4096].all()
    tail = valid[4096:]
    want = np.ones(len(tail), dtype=np.uint8)
    want[[17, 18, 19, 20, 21, 22, 24, 25, 26, 27]] = 0  # the zero normals, NaN, inf, 2e18; then the three bad positions (1e18 itself is in range)
    assert np.array_equal(tail, want), tail
    assert not O[valid == 0].any() and not D[valid == 0].any()


def test_face_eye_turns_exactly_the_normals_that_look_away(H, points):
    P, N = points
    P, N = P[:4096], N[:4096]
    eye = np.array([0.5, -60.0, 2.0])
    _, D, _ = replay(H, P, N, 1, eye=eye)
    away = ((N * (P - eye)).sum(1) > 0.0)
    assert 1000 < away.sum() < 3000, "both sides are exercised"
    _, D_turned, _ = replay(H, P, np.where(away[:, None], -N, N), 1)
    assert same_bits(D, D_turned)


def test_a_slice_with_its_first_index_is_that_slice_of_the_whole_and_passes_and_seeds_differ(H, points):
    P, N = points
    P, N = P[:512], N[:512]
    O, D, _ = replay(H, P, N, 16, seed=3, pas=2, first=1000)
    for k, m in ((0, 1), (1, 63), (64, 65), (300, 212)):
        O2, D2, _ = replay(H, P[k:k + m], N[k:k + m], 16, seed=3, pas=2, first=1000 + k)
        assert same_bits(O[k:k + m], O2) and same_bits(D[k:k + m], D2)
    assert not same_bits(D, replay(H, P, N, 16, seed=3, pas=1, first=1000)[1]) and not same_bits(D, replay(H, P, N, 16, seed=4, pas=2, first=1000)[1])
    assert same_bits(replay(H, P, N, 64, seed=3, pas=2, first=1000)[1][:, :16], D), "S samples are the first S of 64"


def test_every_ray_is_unit_and_above_its_points_plane(H, points):
    P, N = points
    P, N = P[:4096], N[:4096]
    O, D, _ = replay(H, P, N, 64, seed=11, bias=0.5)
    nn = N / np.sqrt((N * N).sum(1))[:, None]
    assert (np.sqrt((D * D).sum(2)) - 1.0).max() <= 1e-15 and (1.0 - np.sqrt((D * D).sum(2))).max() <= 1e-15
    assert (D * nn[:, None, :]).sum(2).min() >= 0.08, "sqrt(1/128) = 0.088 is the lowest direction of the table"
    assert np.abs(O[:, 0, :] - (P + nn * 0.5)).max() <= 1e-13 and same_bits(O, np.broadcast_to(O[:, :1, :], O.shape).copy())
    rot = (rng_f64(11, np.arange(4096, dtype=np.uint64), 0, 0) * 256.0).astype(int)
    assert len(set(rot.tolist())) == 256, "every rotation of the table is drawn"


def test_the_hook_refuses_what_the_pass_refuses(H):
    P = np.zeros((1, 3)); N = np.array([[0.0, 0.0, 1.0]])
    O, D, valid = np.zeros((1, 64, 3)), np.zeros((1, 64, 3)), np.zeros(1, dtype=np.uint8)
    args = (P.ctypes.data_as(H._dp), N.ctypes.data_as(H._dp), O.ctypes.data_as(H._dp), D.ctypes.data_as(H._dp), valid.ctypes.data_as(H._u8p))
    ok = dict(n=1, samples=16, pass_index=0, seed=0, first_index=0, radius=1.0, bias=0.0, flags=0)
    for change in (dict(samples=0), dict(samples=3), dict(samples=128), dict(radius=float("nan")), dict(radius=1e-5), dict(radius=-1.0), dict(bias=-1e-9), dict(bias=float("inf")),
                   dict(bias=float("nan")), dict(flags=2), dict(flags=3)):
        p = H.PtAoParams(**dict(ok, **change))
        assert H.lib().pt_test_ao_rays_host(1, C.byref(p), *args) == H.ERR_ARGUMENT, change
    p = H.PtAoParams(**dict(ok, flags=H.AO_FACE_EYE))
    p.eye[1] = float("nan")
    assert H.lib().pt_test_ao_rays_host(1, C.byref(p), *args) == H.ERR_ARGUMENT
    assert H.lib().pt_test_ao_rays_host(1, C.byref(H.PtAoParams(**dict(ok, radius=float("inf")))), *args) == 0
    assert H.lib().pt_test_ao_rays_host(1, None, *args) == H.ERR_ARGUMENT
