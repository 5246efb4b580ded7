"""The film's running sum without a GPU: pt_test_film_fold_host runs the two functions the fold and resolve kernels call (pt_film_fold, pt_film_sum) over one
pixel's samples, cut into consecutive adds. Whatever the cuts, the result carries the bits of DESIGN section 2's summation contract, restated here in numpy:
chunks of 8 summed left to right, then the chunk sums summed left to right - the first operand of either sum taken as it is, not added to zero."""
import ctypes as C
import itertools

import numpy as np
import pytest


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def contract_sum(samples):
    """(n, 3) -> (3,): the render's association."""
    chunks = []
    for k in range(0, len(samples), 8):
        c = samples[k].copy()
        for v in samples[k + 1:k + 8]:
            c = c + v
        chunks.append(c)
    total = chunks[0]
    for c in chunks[1:]:
        total = total + c
    return total


def fold(H, samples, cuts):
    s = np.ascontiguousarray(samples, dtype=np.float64)
    cu = (C.c_uint32 * len(cuts))(*cuts)
    out = np.full(3, np.nan)
    rc = H.lib().pt_test_film_fold_host(len(s), s.ctypes.data_as(H._dp), cu, len(cuts), out.ctypes.data_as(H._dp))
    assert rc == H.OK, (rc, cuts)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def every_cut(n):
    """Every way of cutting n samples into 1, 2 and 3 consecutive adds."""
    yield (n,)
    for a in range(1, n):
        yield (a, n - a)
    for a, b in itertools.combinations(range(1, n), 2):
        yield (a, b - a, n - b)


@pytest.mark.parametrize("n", range(1, 41))
def test_every_cut_carries_the_contracts_bits(H, n):
    rng = np.random.default_rng(n)
    # magnitudes spread over many binades, both signs: a different association shows in the last bits
    samples = rng.uniform(-1.0, 1.0, size=(n, 3)) * 10.0 ** rng.integers(-6, 7, size=(n, 3))
    samples[0] = (-0.0, 0.0, -0.0)  # a leading -0.0 survives only if the first sample is assigned: 0.0 + -0.0 is +0.0
    if n > 8:
        samples[8, 0] = -0.0
    want = contract_sum(samples)
    single = fold(H, samples, (n,))
    assert np.array_equal(bits(single), bits(want)), (n, single, want)
    cuts = list(every_cut(n))
    assert len(cuts) == 1 + (n - 1) + (n - 1) * (n - 2) // 2
    for cut in cuts:
        got = fold(H, samples, cut)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got), bits(single)), (n, cut, got, want)


def test_a_leading_negative_zero_stays_negative(H):
    for n in (1, 8):
        s = np.zeros((n, 3))
        s[:] = -0.0
        got = fold(H, s, (n,))
        assert np.all(np.signbit(got)), (n, got)
    s = np.full((9, 3), -0.0)
    s[8] = 0.0  # chunk 0 sums to -0.0, chunk 1 is +0.0: -0.0 + 0.0 = +0.0, as the render has it
    assert not np.any(np.signbit(fold(H, s, (4, 5))))
    assert np.array_equal(bits(fold(H, s, (4, 5))), bits(contract_sum(s)))


def test_the_association_is_not_a_plain_running_sum(H):
    """The samples are chosen so that the contract's association and a left-to-right sum of all samples differ: the test above would pass for neither otherwise."""
    s = np.zeros((16, 3))
    s[0] = 1e16
    s[1:] = 1.0
    plain = s[0].copy()
    for v in s[1:]:
        plain = plain + v
    want = contract_sum(s)
    assert not np.array_equal(bits(plain), bits(want))
    for cut in ((16,), (7, 9), (8, 8), (1, 14, 1)):
        assert np.array_equal(bits(fold(H, s, cut)), bits(want)), cut


def test_bad_requests(H):
    lib = H.lib()
    s = np.zeros((4, 3))
    out = np.zeros(3)
    dp = lambda a: a.ctypes.data_as(H._dp)
    cuts = (C.c_uint32 * 2)(1, 3)
    assert lib.pt_test_film_fold_host(4, dp(s), cuts, 2, dp(out)) == H.OK
    assert lib.pt_test_film_fold_host(4, None, cuts, 2, dp(out)) == H.ERR_ARGUMENT
    assert lib.pt_test_film_fold_host(4, dp(s), None, 2, dp(out)) == H.ERR_ARGUMENT
    assert lib.pt_test_film_fold_host(4, dp(s), cuts, 2, None) == H.ERR_ARGUMENT
    assert lib.pt_test_film_fold_host(0, dp(s), cuts, 2, dp(out)) == H.ERR_ARGUMENT
    assert lib.pt_test_film_fold_host(4, dp(s), cuts, 0, dp(out)) == H.ERR_ARGUMENT
    assert lib.pt_test_film_fold_host(3, dp(s), cuts, 2, dp(out)) == H.ERR_ARGUMENT  # the cuts do not add up
