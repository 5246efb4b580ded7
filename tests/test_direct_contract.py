"""The contract of the direct-light pass without a GPU (portrayer_amd/csrc/pt_direct.h): the numpy restatement of its steps (tests/direct_restate.py)
against the host replay pt_test_direct_host, which compiles the functions the kernel compiles, in every bit of every output."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from direct_restate import accumulate, restate  # noqa: E402
from test_ao_contract import same_bits  # noqa: E402


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def light(pos, colour=(0.9, 0.8, 0.7), falloff=(1.0, 0.05, 0.002), a=(0.0, 0.0, 0.0), b=(0.0, 0.0, 0.0)):
    return list(pos) + list(colour) + list(falloff) + list(a) + list(b)


POINT_A = light((3.0, 40.0, -2.0))
POINT_B = light((-30.0, 25.0, 10.0), (0.2, 0.3, 1.0), (0.5, 0.0, 0.01))
AREA_A = light((0.0, 35.0, 0.0), (1.0, 1.0, 1.0), (1.0, 0.0, 0.0), (4.0, 0.0, 0.5), (0.0, 0.25, 3.0))
AREA_B = light((20.0, 20.0, 20.0), (0.5, 0.6, 0.7), (0.0, 0.1, 0.0), (0.0, 2.0, 0.0), (1.0, 0.0, -1.0))
HALF_AREA = light((5.0, 30.0, 5.0), a=(1.0, 2.0, 3.0), b=(0.0, -0.0, 0.0))  # exactly one zero vector: a point light
LIGHT_LISTS = {
    "point only": [POINT_A, POINT_B],
    "area only": [AREA_A, AREA_B],
    "area, point, area": [AREA_A, POINT_A, AREA_B],  # draws 0, 1 and 2, 3
    "one zero vector": [HALF_AREA, AREA_B],          # draws 0, 1 go to the second
    "no lights": [],
    "65 lights": [light((np.cos(i) * 30.0, 20.0 + i, np.sin(i) * 30.0), a=(1.0, 0.0, 0.0) if i % 3 == 0 else (0.0, 0.0, 0.0), b=(0.0, 0.0, 1.0)) for i in range(65)],
}


def replay(H, P, N, lights, S, seed=0, pas=0, first=0, bias=0.0, eye=None, to_light=False):
    n = len(P)
    P, N = np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(N, dtype=np.float64)
    Lt = np.ascontiguousarray(np.asarray(lights, dtype=np.float64).reshape(-1, 15))
    L = len(Lt)
    e = (0.0, 0.0, 0.0) if eye is None else tuple(float(v) for v in eye)
    flags = (H.AO_FACE_EYE if eye is not None else 0) | (H.DIRECT_TO_LIGHT if to_light else 0)
    p = H.PtDirectParams(n, S, pas, seed, first, bias, flags, (C.c_double * 3)(*e))
    O, D, T, E, valid = np.full((n, 3), 7.0), np.full((n, L, S, 3), 7.0), np.full((n, L, S), 7.0), np.full((n, L, S, 3), 7.0), np.full(n, 7, dtype=np.uint8)
    dp = H._dp
    rc = H.lib().pt_test_direct_host(n, C.byref(p), P.ctypes.data_as(dp), N.ctypes.data_as(dp), L, Lt.ctypes.data_as(dp) if L else None, O.ctypes.data_as(dp),
                                     D.ctypes.data_as(dp), T.ctypes.data_as(dp), E.ctypes.data_as(dp), valid.ctypes.data_as(H._u8p))
    assert rc == 0
    return O, D, T, E, valid


def same(a, b):
    return all(same_bits(x, y) for x, y in zip(a[:4], b[:4])) and np.array_equal(a[4], b[4])


@pytest.fixture(scope="module")
def points():
    """512 random points below the lights with normals of any length and direction, then the corners: a point exactly at a light, one with the light in its
    tangent plane and one with it below, and the validity rule's among good points."""
    rng = np.random.default_rng(20262)
    P = rng.uniform(-15.0, 15.0, (512, 3))
    N = rng.normal(size=(512, 3)) * np.exp(rng.uniform(-3.0, 3.0, (512, 1)))
    N[:150, 1] = np.abs(N[:150, 1])  # many of them look up, where the lights are
    sp_P = [POINT_A[0:3], (3.0, 40.0, 5.0), (3.0, 45.0, -2.0), (0.0, 0.0, 0.0), (1.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (np.nan, 0.0, 0.0),
            (0.0, -np.inf, 0.0), (0.0, 0.0, 2e18), (1.0, 1.0, 1.0), (1e18, -1e18, 1e18)]
    sp_N = [(0.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 0.0), (np.nan, 0.0, 1.0), (0.0, np.inf, 1.0), (2e18, 1.0, 0.0), (-0.0, 0.0, -0.0), (0.0, 1.0, 0.0),
            (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.0, 3.0, 0.0), (0.0, 1.0, 0.0)]
    P = np.vstack([P[:300], np.array(sp_P), P[300:]])
    N = np.vstack([N[:300], np.array(sp_N), N[300:]])
    return P, N


@pytest.mark.parametrize("name", sorted(LIGHT_LISTS))
@pytest.mark.parametrize("S", (1, 4, 64))
def test_the_restatement_equals_the_host_replay_in_every_bit(H, points, name, S):
    P, N = points
    if name == "65 lights" and S == 64:
        P, N = P[250:350], N[250:350]  # (the corners among them; 65 x 64 samples of 100 points)
    lights = LIGHT_LISTS[name]
    for seed, pas, first, bias, eye, to_light in ((0, 0, 0, 0.0, None, False), (7, 1, 5, 1e-3, None, True), (7, 0, 1 << 60, 0.0, (0.5, -60.0, 2.0), False),
                                                  (0x9e3779b97f4a7c15, 3, 1000, 0.25, (0.0, 60.0, -1.0), True)):
        a = restate(P, N, lights, S, seed, pas, first, bias, eye, to_light)
        b = replay(H, P, N, lights, S, seed, pas, first, bias, eye, to_light)
        assert np.array_equal(a[4], b[4])
        for what, x, y in zip(("origins", "directions", "t_max", "terms"), a, b):
            assert same_bits(x, y), (what, name, S, seed, pas, first, bias, eye, to_light)


def test_the_corners_cast_no_ray_and_invalid_points_report_zeros(H, points):
    P, N = points
    O, D, T, E, valid = replay(H, P, N, [POINT_A], 1)
    assert valid[:300].all() and valid[313:].all()
    assert valid[300:313].tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1]
    # the light at the point (c NaN), in its tangent plane (c = 0) and below it (c = 0): t_max 0, term 0, though the points are valid
    assert not T[300:303].any() and not E[300:303].any() and not D[300:303].any()
    assert not O[valid == 0].any() and not D[valid == 0].any() and not T[valid == 0].any() and not E[valid == 0].any()
    assert T[311, 0, 0] == np.inf and (E[311] > 0.0).all(), "an unnormalised normal that looks at the light"
    assert (T[:300] > 0.0).sum() > 100 and (T[:300] == 0.0).sum() > 40, "both sides of the cosine are exercised"
    # to_light: the bound is the distance, and the direction is unit
    O2, D2, T2, E2, _ = replay(H, P, N, [POINT_A], 1, to_light=True)
    cast = T2[:, 0, 0] > 0.0
    assert np.array_equal(cast, T[:, 0, 0] > 0.0) and same_bits(D, D2) and same_bits(E, E2)
    assert np.abs(T2[cast, 0, 0] - np.sqrt(((np.array(POINT_A[0:3]) - O2[cast]) ** 2).sum(1))).max() < 1e-12
    assert np.abs(np.sqrt((D2[cast, 0, 0] ** 2).sum(1)) - 1.0).max() < 1e-15


def test_a_bias_beyond_the_ray_queries_range_casts_nothing(H, points):
    P, N = points
    O, D, T, E, valid = replay(H, P[:300], N[:300], [POINT_A, AREA_A], 4, bias=1e19)
    assert valid.all() and not T.any() and not E.any() and not D.any()
    assert same((O, D, T, E, valid), restate(P[:300], N[:300], [POINT_A, AREA_A], 4, bias=1e19))


def test_face_eye_turns_exactly_the_normals_that_look_away(H, points):
    P, N = points
    P, N = P[:300], N[:300]
    eye = np.array([0.5, -60.0, 2.0])
    away = ((N * (P - eye)).sum(1) > 0.0)
    assert 50 < away.sum() < 250, "both sides are exercised"
    assert same(replay(H, P, N, [AREA_A, POINT_B], 4, eye=eye), replay(H, P, np.where(away[:, None], -N, N), [AREA_A, POINT_B], 4))


def test_a_slice_with_its_first_index_is_that_slice_of_the_whole(H, points):
    P, N = points
    lights = LIGHT_LISTS["area, point, area"]
    for first in (1000, 1 << 60, (1 << 64) - 100):
        whole = replay(H, P, N, lights, 4, seed=3, pas=2, first=first)
        for k, m in ((0, 1), (1, 63), (64, 65), (290, 212)):
            part = replay(H, P[k:k + m], N[k:k + m], lights, 4, seed=3, pas=2, first=(first + k) % (1 << 64))
            assert same(tuple(x[k:k + m] for x in whole), part), (first, k, m)


def test_another_pass_and_another_seed_move_area_samples_and_nothing_else(H, points):
    P, N = points
    lights = LIGHT_LISTS["area, point, area"]
    base = replay(H, P, N, lights, 4, seed=3, pas=2, first=9)
    for other in (replay(H, P, N, lights, 4, seed=3, pas=1, first=9), replay(H, P, N, lights, 4, seed=4, pas=2, first=9)):
        assert same_bits(base[0], other[0]) and np.array_equal(base[4], other[4])
        for x, y in zip(base[1:4], other[1:4]):
            assert same_bits(x[:, 1], y[:, 1]), "the point light's samples stay"
            assert not same_bits(x[:, 0], y[:, 0]) and not same_bits(x[:, 2], y[:, 2]), "the area lights' move"
    # a point light's S samples are one sample
    assert same_bits(base[1][:, 1], np.broadcast_to(base[1][:, 1, :1], base[1][:, 1].shape).copy())
    # the two area lights draw from different numbers: equal lights at different places in the list sample differently
    twice = replay(H, P, N, [AREA_A, AREA_A], 4, seed=3, pas=2, first=9)
    assert not same_bits(twice[1][:, 0], twice[1][:, 1])
    # ... and a point light in front of an area light consumes no draws
    assert same_bits(replay(H, P, N, [POINT_A, AREA_A], 4, seed=3)[1][:, 1], replay(H, P, N, [AREA_A], 4, seed=3)[1][:, 0])


def test_the_sum_adds_a_point_lights_sample_S_times_in_order(points):
    P, N = points
    O, D, T, E, valid = restate(P[:300], N[:300], [POINT_A, AREA_A], 4)
    occ = np.zeros(T.shape, dtype=np.uint8)
    occ[::2, 1, 1] = 1
    total, lit = accumulate(T, E, valid, occ)
    i = int(np.argmax((T[:, 0, 0] > 0.0) & (T[:, 1] > 0.0).all(1) & (np.arange(300) % 2 == 0)))
    want = np.zeros(3)
    for li, k in ((0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 2), (1, 3)):
        want = want + E[i, li, k]
    assert same_bits(total[i], want) and lit[i] == 7


def test_the_hook_refuses_what_the_pass_refuses(H):
    P = np.zeros((1, 3)); N = np.array([[0.0, 0.0, 1.0]]); Lt = np.array(POINT_A)
    O, D, T, E, valid = np.zeros((1, 3)), np.zeros((1, 1, 64, 3)), np.zeros((1, 1, 64)), np.zeros((1, 1, 64, 3)), np.zeros(1, dtype=np.uint8)
    dp = H._dp
    args = (P.ctypes.data_as(dp), N.ctypes.data_as(dp), 1, Lt.ctypes.data_as(dp), O.ctypes.data_as(dp), D.ctypes.data_as(dp), T.ctypes.data_as(dp), E.ctypes.data_as(dp),
            valid.ctypes.data_as(H._u8p))
    ok = dict(n=1, samples=16, pass_index=0, seed=0, first_index=0, bias=0.0, flags=0)
    for change in (dict(samples=0), dict(samples=3), dict(samples=128), dict(bias=-1e-9), dict(bias=float("inf")), dict(bias=float("nan")), dict(flags=4), dict(flags=7),
                   dict(n=(1 << 24) + 1)):
        assert H.lib().pt_test_direct_host(1, C.byref(H.PtDirectParams(**dict(ok, **change))), *args) == H.ERR_ARGUMENT, change
    p = H.PtDirectParams(**dict(ok, flags=H.AO_FACE_EYE))
    p.eye[1] = float("nan")
    assert H.lib().pt_test_direct_host(1, C.byref(p), *args) == H.ERR_ARGUMENT
    for flags in (0, H.AO_FACE_EYE, H.DIRECT_TO_LIGHT, H.AO_FACE_EYE | H.DIRECT_TO_LIGHT):
        assert H.lib().pt_test_direct_host(1, C.byref(H.PtDirectParams(**dict(ok, flags=flags))), *args) == 0
    assert H.lib().pt_test_direct_host(1, None, *args) == H.ERR_ARGUMENT
