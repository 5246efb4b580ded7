"""The contract of the probe pass without a GPU (portrayer_amd/csrc/pt_probe.h): the numpy restatement of its steps 1 to 5 (tests/probe_restate.py)
against the host replay pt_test_probe_host, which compiles the functions the kernel compiles, in every bit; the tables against the header and their generator;
and the properties the tables are chosen for."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from probe_restate import DIRS, ROOT, SAMPLES, SH, project, restate, stream_indices  # noqa: E402
from test_ao_contract import rng_f64, same_bits  # noqa: E402


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def replay(H, P, S, seed=0, pas=0, first=0):
    n = len(P)
    P = np.ascontiguousarray(P)
    p = H.PtProbeParams(n, S, pas, seed, first)
    O, D, Y, valid = np.full((n, S, 3), 7.0), np.full((n, S, 3), 7.0), np.full((n, S, 9), 7.0), np.full(n, 7, dtype=np.uint8)
    dp = lambda a: a.ctypes.data_as(H._dp)
    assert H.lib().pt_test_probe_host(n, C.byref(p), dp(P), dp(O), dp(D), dp(Y), valid.ctypes.data_as(H._u8p)) == 0
    return O, D, Y, valid


@pytest.fixture(scope="module")
def probes():
    """200 random positions, then the corners of the validity rule between valid ones"""
    rng = np.random.default_rng(20262)
    P = rng.uniform(-50.0, 50.0, (200, 3))
    odd = [[np.nan, 0.0, 0.0], [1.0, 2.0, 3.0], [0.0, -np.inf, 0.0], [0.0, np.inf, 1.0], [0.0, 0.0, 2e18], [-2e18, 0.0, 0.0], [1e18, -1e18, 1e18], [0.0, 0.0, 0.0], [-0.0, 1e-300, 5.0]]
    return np.vstack([P[:100], odd, P[100:]])


def test_the_librarys_tables_are_the_headers_and_the_generator_agrees(H):
    dirs, sh = np.zeros((1024, 3)), np.zeros(5)
    assert H.lib().pt_test_probe_tables(dirs.ctypes.data_as(H._dp), sh.ctypes.data_as(H._dp)) == 0
    assert same_bits(dirs, DIRS) and same_bits(sh, SH)
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_probe_tables.py"), "--check"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    pi = np.pi
    want = [1.0 / (2.0 * np.sqrt(pi)), np.sqrt(3.0 / (4.0 * pi)), np.sqrt(15.0 / (4.0 * pi)), np.sqrt(5.0 / (16.0 * pi)), np.sqrt(15.0 / (16.0 * pi))]
    assert np.abs(SH / np.array(want) - 1.0).max() <= 4 * 2.0 ** -53, "libm's values are within a few roundings of the nearest doubles"


def test_every_prefix_is_stratified_in_u_and_in_v():
    """u = (1 - z) / 2 and the azimuth v: each of the S strata [m / S, (m + 1) / S) holds one of the first S directions, for every S the pass takes - so any
    coarser power-of-two partition holds equally many."""
    for S in SAMPLES:
        u = (1.0 - DIRS[:S, 2]) / 2.0  # (exact: z = 1 - 2 u with u a multiple of 1/2048)
        assert sorted(np.floor(u * S).astype(int)) == list(range(S)), "one direction per stratum of u at S = %d" % S
        v = np.arctan2(DIRS[:S, 1], DIRS[:S, 0]) / (2.0 * np.pi) % 1.0
        assert sorted(np.floor(v * S).astype(int)) == list(range(S)), "and of v at S = %d" % S
        for coarse in (2, 8, 64):
            assert np.all(np.bincount(np.floor(u * coarse).astype(int), minlength=coarse) == S // coarse)
            assert np.all(np.bincount(np.floor(v * coarse).astype(int), minlength=coarse) == S // coarse)
    assert np.array_equal(((1.0 - DIRS[:, 2]) / 2.0 * 2048.0) % 2.0, np.ones(1024)), "u is an odd multiple of 1/2048"


def test_every_table_direction_is_a_unit_vector_to_one_rounding_per_component():
    """Each component is the exact value rounded once: three errors of at most 2^-53 each move the length by at most sqrt(3) 2^-53 < 2^-52. Measured without a
    rounding of its own: the squared length in exact rational arithmetic."""
    from fractions import Fraction
    worst = Fraction(0)
    for d in DIRS:
        sq = sum(Fraction(float(c)) ** 2 for c in d)
        worst = max(worst, abs(sq - 1))
    # | |d| - 1 | = | |d|^2 - 1 | / (|d| + 1); |d| + 1 >= 2 - 2^-52
    assert worst / (2 - Fraction(1, 2 ** 52)) <= Fraction(1, 2 ** 52), float(worst)


@pytest.mark.parametrize("S", [64, 1024])
def test_the_restatement_equals_the_host_replay_in_every_bit(H, probes, S):
    for seed in (0, 0x9e3779b97f4a7c15):
        for pas in (0, 3):
            for first in (0, 1 << 60):
                O, D, Y, valid = restate(probes, S, seed, pas, first)
                O2, D2, Y2, valid2 = replay(H, probes, S, seed, pas, first)
                tag = (S, seed, pas, first)
                assert np.array_equal(valid, valid2), tag
                assert same_bits(O, O2), tag
                assert same_bits(D, D2), tag
                assert same_bits(Y, Y2), tag
    assert list(valid[100:109]) == [0, 1, 0, 0, 0, 0, 1, 1, 1], "NaN, inf and 2e18 are invalid; 1e18 is the last valid magnitude"
    assert not O[valid == 0].any() and not D[valid == 0].any() and not Y[valid == 0].any(), "an invalid probe's rays and basis values are zeros"
    assert same_bits(O[valid == 1], np.broadcast_to(probes[valid == 1][:, None, :], (int(valid.sum()), S, 3)).copy()), "the origin is the position itself"
    assert np.abs(np.sqrt((D * D).sum(-1))[valid == 1] - 1.0).max() < 1e-15


def test_a_slice_with_its_first_index_is_that_slice_of_the_whole_and_passes_and_seeds_differ(H, probes):
    whole = replay(H, probes, 64, 7, 1, 1000)
    part = replay(H, probes[40:90], 64, 7, 1, 1040)
    for a, b in zip(whole, part):
        assert np.array_equal(a[40:90].view(np.uint8), b.view(np.uint8))
    for other in (replay(H, probes, 64, 8, 1, 1000), replay(H, probes, 64, 7, 2, 1000), replay(H, probes, 64, 7, 1, 1001)):
        assert not same_bits(whole[1], other[1])
    # neighbouring probes do not share directions: the axis and the rotation are the probe's own draws
    assert len({whole[1][i].tobytes() for i in range(100)}) > 90


def test_the_hook_refuses_what_the_pass_refuses(H):
    P = np.zeros((1, 3))
    dp = lambda a: a.ctypes.data_as(H._dp)
    for S in (0, 32, 96, 2048):
        O, D, Y, v = np.zeros((1, 2048, 3)), np.zeros((1, 2048, 3)), np.zeros((1, 2048, 9)), np.zeros(1, dtype=np.uint8)
        assert H.lib().pt_test_probe_host(1, C.byref(H.PtProbeParams(1, S, 0, 0, 0)), dp(P), dp(O), dp(D), dp(Y), v.ctypes.data_as(H._u8p)) == H.ERR_ARGUMENT
    assert H.lib().pt_test_probe_host(1, None, dp(P), None, None, None, None) == H.ERR_ARGUMENT


def test_the_stream_product_wraps_modulo_two_to_the_64():
    """Sample k of probe i draws from the stream (first_index + i) * S + k, a 64-bit product reduced modulo 2^64 only - the same value as pt_radiance's
    stream_base + (i * S + k) with stream_base = first_index * S reduced the same way. At first_index = 2^60 and S = 1024 the product is 2^70."""
    M = 1 << 64
    for first, S in ((1 << 60, 1024), (1 << 60, 64), ((1 << 64) - 3, 128), (0x9e3779b97f4a7c15, 512)):
        q = stream_indices(5, first)
        assert [int(v) for v in q] == [(first + i) % M for i in range(5)]
        with np.errstate(over="ignore"):
            stream = q[:, None] * np.uint64(S) + np.arange(S, dtype=np.uint64)[None, :]
            base = np.uint64(first) * np.uint64(S)
            radiance = base + np.arange(5 * S, dtype=np.uint64)
        assert [int(v) for v in stream.ravel()[[0, 1, S, 5 * S - 1]]] == [((first + i) * S + k) % M for i, k in ((0, 0), (0, 1), (1, 0), (4, S - 1))]
        assert np.array_equal(stream.ravel(), radiance)
    assert ((1 << 60) * 1024) % M == 0 and ((1 << 60) * 64) % M == 0  # 2^70 and 2^66 wrap to nothing: with first_index = 2^60 probe i has the streams of probe i with first_index = 0
    a = rng_f64(7, np.array([((1 << 60) + 1) * 1024 % M], dtype=np.uint64), 0, 2)
    b = rng_f64(7, np.array([1024], dtype=np.uint64), 0, 2)
    assert a[0] == b[0]


def test_the_projection_of_a_constant_is_the_sum_of_the_basis_and_its_order_is_per_round():
    P = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0]])
    _, D, Y, valid = restate(P, 256, 3, 0, 5)
    sh = project(Y, np.ones((2, 256, 3)), valid)
    assert not sh[1].any()
    # Monte Carlo: 4 pi / S x the sums estimates the coefficients of L = 1: (2 sqrt(pi), 0, ...); the stratified set is far better than 1 / sqrt(S)
    est = sh[0, :, 0] * (4.0 * np.pi / 256.0)
    assert abs(est[0] - 2.0 * np.sqrt(np.pi)) < 1e-12 and np.abs(est[1:]).max() < 0.05
    rounds = [Y[0, 64 * r:64 * r + 64] for r in range(4)]
    by_hand = None
    for part in rounds:
        acc = np.zeros(9)
        for k in range(64):
            acc = acc + part[k] * 1.0
        by_hand = acc if by_hand is None else by_hand + acc
    assert same_bits(sh[0, :, 1], by_hand)
