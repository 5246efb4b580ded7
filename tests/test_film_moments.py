"""A film with moments without a GPU: pt_test_film_moments_host runs the functions the fold and error kernels call (pt_film_fold, pt_film_moment, pt_film_sum,
pt_film_error_of) over one pixel's samples, cut into consecutive adds. Whatever the cuts: the sum carries the bits of DESIGN section 2's summation contract, q
those of a plain left-to-right sum of y * y with y = (v.x + v.y) + v.z, and err those of the header's order of operations - every step a correctly rounded
IEEE operation, restated here in numpy."""
import ctypes as C

import numpy as np
import pytest

from test_film_fold import bits, contract_sum, every_cut


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def moments(H, samples, cuts):
    s = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1, 3)
    cu = (C.c_uint32 * max(len(cuts), 1))(*cuts)
    out, q, err = np.full(3, np.nan), C.c_double(np.nan), C.c_double(np.nan)
    rc = H.lib().pt_test_film_moments_host(len(s), s.ctypes.data_as(H._dp), cu, len(cuts), out.ctypes.data_as(H._dp), C.byref(q), C.byref(err))
    assert rc == H.OK, (rc, cuts)
    return out, np.float64(q.value), np.float64(err.value)


def want_q(samples):
    q = None
    for v in samples:
        y = (v[0] + v[1]) + v[2]
        q = y * y if q is None else q + y * y
    return np.float64(q)


def want_err(S, q, n):
    """include/portrayer_hip.h, pt_film_error, operation for operation (numpy float64 scalars: one rounding each)."""
    if n < 2:
        return np.float64(np.inf)
    dn = np.float64(n)
    mean = S / dn
    my = (mean[0] + mean[1]) + mean[2]
    var = (q - (dn * my) * my) / np.float64(n - 1)
    if not var > 0.0:
        var = np.float64(0.0)
    return np.sqrt(var / dn)


@pytest.mark.parametrize("n", range(1, 41))
def test_every_cut_carries_the_bits_of_the_restatement(H, n):
    rng = np.random.default_rng(100 + n)
    samples = rng.uniform(-1.0, 1.0, size=(n, 3)) * 10.0 ** rng.integers(-3, 4, size=(n, 3))
    samples[0] = (-0.0, 0.0, -0.0)  # a leading -0.0 survives in the sum only if the first sample is assigned
    S, q = contract_sum(samples), want_q(samples)
    e = want_err(S, q, n)
    assert (n == 1) == bool(np.isinf(e)) and (n == 1 or e > 0.0)
    for cut in every_cut(n):
        got_S, got_q, got_e = moments(H, samples, cut)
        assert np.array_equal(bits(got_S), bits(S)), (n, cut, got_S, S)
        assert bits(got_q) == bits(q), (n, cut, got_q, q)
        assert bits(got_e) == bits(e), (n, cut, got_e, e)


def test_fewer_than_two_samples_have_no_estimate(H):
    _, _, e = moments(H, np.zeros((0, 3)), ())
    assert np.isposinf(e)
    _, q, e = moments(H, np.array([[0.25, 0.5, 0.125]]), (1,))
    assert np.isposinf(e) and q == 0.875 * 0.875


@pytest.mark.parametrize("value", [(0.1, 0.2, 0.3), (1e-3, 7.0, 0.25), (0.0, 0.0, 0.0), (1 / 3, 1 / 3, 1 / 3)])
def test_a_constant_pixel_has_error_zero_not_a_negative_variance(H, value):
    """With equal samples q - n my^2 is rounding noise of either sign: a var that is not > 0 becomes 0, so the error is +0.0 and never the root of a negative."""
    seen_clamp = False
    for n in range(2, 41):
        s = np.tile(np.array(value), (n, 1))
        S, q, e = moments(H, s, (n,))
        assert bits(e) == bits(want_err(contract_sum(s), want_q(s), n)) and not np.isnan(e) and e >= 0.0, (n, e)
        dn = np.float64(n)
        my = ((S / dn)[0] + (S / dn)[1]) + (S / dn)[2]
        if not (q - (dn * my) * my) > 0.0:
            seen_clamp = True
            assert bits(e) == bits(np.float64(0.0)), (n, e)
    assert seen_clamp, "no count at which the variance of a constant pixel came out as zero or negative: the case is not covered"


def test_bad_requests(H):
    lib = H.lib()
    s, out, q, e = np.zeros((4, 3)), np.zeros(3), C.c_double(), C.c_double()
    dp = lambda a: a.ctypes.data_as(H._dp)
    cuts = (C.c_uint32 * 2)(1, 3)
    assert lib.pt_test_film_moments_host(4, dp(s), cuts, 2, dp(out), C.byref(q), C.byref(e)) == H.OK
    assert lib.pt_test_film_moments_host(4, None, cuts, 2, dp(out), C.byref(q), C.byref(e)) == H.ERR_ARGUMENT
    assert lib.pt_test_film_moments_host(4, dp(s), None, 2, dp(out), C.byref(q), C.byref(e)) == H.ERR_ARGUMENT
    assert lib.pt_test_film_moments_host(4, dp(s), cuts, 2, None, C.byref(q), C.byref(e)) == H.ERR_ARGUMENT
    assert lib.pt_test_film_moments_host(4, dp(s), cuts, 2, dp(out), None, C.byref(e)) == H.ERR_ARGUMENT
    assert lib.pt_test_film_moments_host(4, dp(s), cuts, 2, dp(out), C.byref(q), None) == H.ERR_ARGUMENT
    assert lib.pt_test_film_moments_host(4, dp(s), cuts, 0, dp(out), C.byref(q), C.byref(e)) == H.ERR_ARGUMENT
    assert lib.pt_test_film_moments_host(3, dp(s), cuts, 2, dp(out), C.byref(q), C.byref(e)) == H.ERR_ARGUMENT  # the cuts do not add up
