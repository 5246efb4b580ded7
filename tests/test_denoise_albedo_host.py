"""The demodulated denoise's contract without a GPU (pt_film_denoise_albedo): the division by the pixel's modulation after the level-0 seed and the
products after the last level, restated in numpy around tests/test_denoise_host.py's numpy_denoise, must equal pt_test_denoise_albedo_host in every bit.
Every comparison here is exact (view(np.uint64)) except the no-leak bound, whose reasoning stands beside it, and the one quality condition at the end."""
import ctypes as C

import numpy as np
import pytest

from test_denoise_host import ITERATIONS, SIZES, bits, host_denoise, numpy_denoise, prototype_image, synthetic

ALBEDO_EPS = 0.0078125  # PT_DENOISE_ALBEDO_EPS, 2^-7
# (sigma_color, sigma_plane, normal_power_log2, same_node): everything on, SAME_NODE, everything off
PARAMS = [(2.0, 0.05, 5, False), (2.0, 0.05, 5, True), (0.0, 0.0, -1, False)]
QUALITY = (2.0, 0.05, 5, False)  # the parameters of test_denoise_host.py's quality test


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def modulation(node, albedo):
    """(m, mm) of every pixel: m = a + EPS per channel of a hit's albedo that is >= 0 and < inf, 1 otherwise and on a miss; mm = ((m.x + m.y) + m.z) / 3."""
    with np.errstate(all="ignore"):
        ok = (albedo >= 0.0) & (albedo < np.inf)  # (False for NaN)
        m = np.where(ok & (node >= 0)[..., None], albedo + ALBEDO_EPS, 1.0)
    return m, ((m[..., 0] + m[..., 1]) + m[..., 2]) / 3.0


def numpy_denoise_albedo(linear, variance, counts, node, normal, position, albedo, iterations, sigma_color, sigma_plane, normal_power_log2, same_node):
    """DESIGN 4.16's steps around numpy_denoise. Pixels with count 0 keep their input."""
    valid = counts > 0
    m, mm = modulation(node, albedo)
    with np.errstate(all="ignore"):
        c = np.where(valid[..., None], linear / m, linear)
        v = np.where(valid, variance / (mm * mm), variance)
        c, v = numpy_denoise(c, v, counts, node, normal, position, iterations, sigma_color, sigma_plane, normal_power_log2, same_node)
        return np.where(valid[..., None], c * m, c), np.where(valid, v * (mm * mm), v)


def host_denoise_albedo(H, linear, variance, counts, node, normal, position, albedo, iterations, sigma_color, sigma_plane, normal_power_log2, same_node, fill=-7.25):
    """pt_test_denoise_albedo_host into buffers pre-filled with `fill`."""
    h, w = counts.shape
    lin, var, cnt = np.ascontiguousarray(linear, dtype=np.float64), np.ascontiguousarray(variance, dtype=np.float64), np.ascontiguousarray(counts, dtype=np.uint32)
    nd, nr, ps = np.ascontiguousarray(node, dtype=np.int32), np.ascontiguousarray(normal, dtype=np.float64), np.ascontiguousarray(position, dtype=np.float64)
    al = np.ascontiguousarray(albedo, dtype=np.float64)
    p = H.PtDenoiseParams(iterations, H.DENOISE_SAME_NODE if same_node else 0, sigma_color, sigma_plane, normal_power_log2)
    g = H.PtDenoiseGuides(ps.ctypes.data, nr.ctypes.data, nd.ctypes.data)
    out_c, out_v = np.full((h, w, 3), fill), np.full((h, w), fill)
    rc = H.lib().pt_test_denoise_albedo_host(w, h, C.byref(p), lin.ctypes.data_as(H._dp), var.ctypes.data_as(H._dp), cnt.ctypes.data_as(H._up), C.byref(g), al.ctypes.data_as(H._dp),
                                             out_c.ctypes.data_as(H._dp), out_v.ctypes.data_as(H._dp))
    assert rc == H.OK, rc
    return out_c, out_v


def synthetic_albedo(s, seed):
    """A seeded albedo for synthetic()'s inputs with, where the size has room, a black pixel, a -0.0, and NaN, negative and +inf channels on hits with samples
    (the m = 1 rule); something arbitrary (never read) on the misses."""
    h, w = s["counts"].shape
    rng = np.random.default_rng(seed)
    albedo = rng.uniform(0.05, 0.95, size=(h, w, 3))
    albedo[s["node"] < 0] = -3.0
    hits = np.flatnonzero((s["node"] >= 0) & (s["counts"] > 0))
    if len(hits) >= 5:
        flat = albedo.reshape(-1, 3)
        at = hits[np.linspace(0, len(hits) - 1, 7).astype(int)[1:6]]
        flat[at[0]] = (0.0, 0.0, 0.0)
        flat[at[1], 1] = -0.0
        flat[at[2], 0] = np.nan
        flat[at[3], 2] = -0.25
        flat[at[4], 1] = np.inf
    return albedo


def test_the_synthetic_albedo_holds_every_case():
    s = synthetic(67, 37, 5)
    a = synthetic_albedo(s, 6)
    live = ((s["node"] >= 0) & (s["counts"] > 0))[..., None] & np.ones(3, dtype=bool)
    assert np.all(a[live[..., 0]] == 0, axis=-1).any(), "a black albedo"
    assert (np.signbit(a) & (a == 0) & live).any() and (np.isnan(a) & live).any() and ((a < 0) & live).any() and (np.isposinf(a) & live).any()
    assert (s["node"] < 0).any() and (s["counts"] == 0).any() and (s["counts"] == 1).any()
    m, mm = modulation(s["node"], a)
    assert np.isfinite(m).all() and (m > 0).all() and np.all(m[s["node"] < 0] == 1.0) and (m[np.isnan(a) & live] == 1.0).all() and (m[np.isposinf(a) & live] == 1.0).all()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("iterations", ITERATIONS)
def test_the_host_replay_is_the_numpy_restatement_bit_for_bit(H, size, iterations):
    w, h = size
    s = synthetic(w, h, 100 + w)
    albedo = synthetic_albedo(s, 200 + w)
    guides = (s["node"], s["normal"], s["position"])
    valid = s["counts"] > 0
    for sc, sp, npl2, same in PARAMS:
        got_c, got_v = host_denoise_albedo(H, s["linear"], s["variance"], s["counts"], *guides, albedo, iterations, sc, sp, npl2, same)
        pre_c, pre_v = np.where(valid[..., None], s["linear"], -7.25), np.where(valid, s["variance"], -7.25)
        want_c, want_v = numpy_denoise_albedo(pre_c, pre_v, s["counts"], *guides, albedo, iterations, sc, sp, npl2, same)
        what = "%dx%d, %d levels, %r" % (w, h, iterations, (sc, sp, npl2, same))
        assert np.array_equal(bits(got_c), bits(want_c)), what
        assert np.array_equal(bits(got_v), bits(want_v)), what
        assert np.all(got_c[~valid] == -7.25) and np.all(got_v[~valid] == -7.25), "pixels without samples are not written"
        assert np.isfinite(got_c).all() and np.isfinite(got_v).all(), what + ": a NaN, negative or infinite albedo channel makes no NaN"


@pytest.mark.parametrize("iterations", [1, 5])
def test_an_albedo_of_one_minus_eps_is_the_plain_filter_in_every_bit(H, iterations):
    """m = (1 - 2^-7) + 2^-7 = 1 and mm = 3 / 3 = 1 exactly: every division and product is by 1."""
    s = synthetic(67, 37, 167)
    guides = (s["node"], s["normal"], s["position"])
    albedo = np.full((37, 67, 3), 1.0 - ALBEDO_EPS)
    for sc, sp, npl2, same in PARAMS:
        got = host_denoise_albedo(H, s["linear"], s["variance"], s["counts"], *guides, albedo, iterations, sc, sp, npl2, same)
        want = host_denoise(H, s["linear"], s["variance"], s["counts"], *guides, iterations, sc, sp, npl2, same)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), (iterations, sc, sp, npl2, same)


@pytest.mark.parametrize("iterations", [1, 5])
def test_grey_power_of_two_albedos_scale_the_plain_filters_result_exactly(H, iterations):
    """m in {1/2, 1/4, 1/8} per pixel, the same in three channels: mm = (3 m) / 3 = m, and every step the albedo adds is a scaling by a power of two. So the
    demodulated filter on (c m, v mm mm) is the plain filter on (c, v), times m (for v: times mm mm), bit for bit."""
    s = synthetic(67, 37, 168)
    guides = (s["node"], s["normal"], s["position"])
    rng = np.random.default_rng(9)
    m1 = np.array([0.5, 0.25, 0.125])[rng.integers(0, 3, size=(37, 67))]
    m1 = np.where(s["node"] >= 0, m1, 1.0)  # (a miss is not modulated, whatever its albedo says)
    albedo = np.repeat((m1 - ALBEDO_EPS)[..., None], 3, axis=-1)
    albedo[s["node"] < 0] = 0.375
    m, mm = modulation(s["node"], albedo)
    assert np.array_equal(m[..., 0], m1) and np.array_equal(mm, m1)
    for sc, sp, npl2, same in PARAMS:
        got_c, got_v = host_denoise_albedo(H, s["linear"] * m, s["variance"] * (mm * mm), s["counts"], *guides, albedo, iterations, sc, sp, npl2, same)
        want_c, want_v = host_denoise(H, s["linear"], s["variance"], s["counts"], *guides, iterations, sc, sp, npl2, same)
        valid = s["counts"] > 0
        assert np.array_equal(bits(got_c[valid]), bits((want_c * m)[valid])), (iterations, sc, sp, npl2, same)
        assert np.array_equal(bits(got_v[valid]), bits((want_v * (mm * mm))[valid])), (iterations, sc, sp, npl2, same)


def test_nothing_leaks_across_the_miss_boundary(H):
    """test_denoise_host.py's no-leak condition on a modulated film: every hit pixel is truth * m (m random per pixel and channel, albedo = m - EPS), every miss
    its truth, v = 0, colour and plane weights off. Demodulated, green is 0.45 or 0.5 on every hit and 0.3 on every miss, each within one rounding ((x m) / m);
    the 5 levels add at most 26 roundings each, the final product and this test's division two more: 134 roundings of values below 1, 134 x 2^-53 < 1e-13."""
    s = prototype_image()
    guides = (s["node"], s["normal"], s["position"])
    valid = s["counts"] > 0
    albedo = np.random.default_rng(11).uniform(0.1, 0.9, size=s["truth"].shape) - ALBEDO_EPS
    m, _ = modulation(s["node"], albedo)
    clean_c, _ = host_denoise_albedo(H, s["truth"] * m, np.zeros_like(s["variance"]), s["counts"], *guides, albedo, 5, 0.0, 0.0, 5, False)
    green = clean_c[..., 1] / m[..., 1]
    hits, misses = (s["node"] >= 0) & valid, (s["node"] < 0) & valid
    assert green[hits].min() >= 0.45 - 1e-13 and green[hits].max() <= 0.5 + 1e-13, "a hit pixel took colour from the miss region"
    assert np.abs(green[misses] - 0.3).max() <= 1e-13, "a miss pixel took colour from a hit"


def test_argument_errors_of_the_host_replay(H):
    w, h = 5, 3
    s = synthetic(w, h, 1)
    albedo = synthetic_albedo(s, 2)
    out_c = np.full((h, w, 3), 7.0)
    dp = lambda a: a.ctypes.data_as(H._dp)
    g = H.PtDenoiseGuides(s["position"].ctypes.data, s["normal"].ctypes.data, s["node"].ctypes.data)
    call = lambda p, al: H.lib().pt_test_denoise_albedo_host(w, h, C.byref(p), dp(s["linear"]), dp(s["variance"]), s["counts"].ctypes.data_as(H._up), C.byref(g), al, dp(out_c), None)
    assert call(H.PtDenoiseParams(3, 0, 2.0, 0.05, 5), None) == H.ERR_ARGUMENT, "a NULL albedo"
    assert call(H.PtDenoiseParams(3, 2, 2.0, 0.05, 5), dp(albedo)) == H.ERR_ARGUMENT, "flags = 2 stays refused: no new bit"
    assert call(H.PtDenoiseParams(9, 0, 2.0, 0.05, 5), dp(albedo)) == H.ERR_ARGUMENT
    assert np.all(out_c == 7.0), "a refused call writes nothing"
    assert call(H.PtDenoiseParams(3, 0, 2.0, 0.05, 5), dp(albedo)) == H.OK
    assert H.DENOISE_ALBEDO_EPS == ALBEDO_EPS == 2.0 ** -7


def textured_prototype(seed):
    """The image the demodulated filter was tried on: prototype_image(seed) with every hit pixel's truth and mean multiplied, per channel, by a random albedo and
    its variance by the square of the albedo's mean over the channels; misses are unmodulated."""
    s = prototype_image(seed)
    albedo = np.random.default_rng(seed + 1).uniform(0.05, 0.95, s["truth"].shape)
    hit = s["node"] >= 0
    scale = np.where(hit[..., None], albedo, 1.0)
    mean_scale = scale.mean(axis=-1)
    s["truth"], s["linear"], s["variance"] = s["truth"] * scale, s["linear"] * scale, s["variance"] * mean_scale * mean_scale
    s["albedo"] = albedo
    return s


def test_on_a_fine_texture_the_demodulated_filter_beats_the_plain_one(H):
    """The one quality condition, seed 2010, 5 levels, the quality test's parameters: the demodulated RMS error to the truth is below the plain filter's and at
    most 0.6 x the input's (it measured 0.46 x; the bound is loose because the image is random, not because the filter is)."""
    s = textured_prototype(2010)
    guides = (s["node"], s["normal"], s["position"])
    valid = s["counts"] > 0
    rms = lambda c: float(np.sqrt(np.mean((c[valid] - s["truth"][valid]) ** 2)))
    before = rms(s["linear"])
    plain, _ = host_denoise(H, s["linear"], s["variance"], s["counts"], *guides, 5, *QUALITY)
    demod, demod_v = host_denoise_albedo(H, s["linear"], s["variance"], s["counts"], *guides, s["albedo"], 5, *QUALITY)
    print("rms to the truth: input %.4f, plain filter %.4f, demodulated filter %.4f (%.2f x the input)" % (before, rms(plain), rms(demod), rms(demod) / before))
    assert np.isfinite(demod[valid]).all() and np.isfinite(demod_v[valid]).all()
    assert rms(demod) < rms(plain)
    assert rms(demod) <= 0.6 * before, (before, rms(demod))
