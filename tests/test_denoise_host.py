"""The denoiser's contract without a GPU (pt_film_denoise): the filter is DEFINED as a fixed sequence of correctly rounded IEEE f64 operations, so
pt_test_denoise_host - the plain loop over the functions the kernels call (portrayer_amd/csrc/pt_denoise.h) - and the vectorised numpy restatement below, one
array operation per tap, must agree in every bit. Every comparison here is exact (view(np.uint64)) except the one quality condition at the end."""
import ctypes as C
import itertools

import numpy as np
import pytest

SIZES = [(1, 1), (5, 3), (16, 16), (17, 33), (67, 37)]  # (width, height)
ITERATIONS = [1, 3, 5, 8]
H5 = [1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0]
EPS = 1e-12  # PT_DENOISE_EPS
# (sigma_color, sigma_plane, normal_power_log2, same_node): everything on, each weight switched off in turn, SAME_NODE, everything off, power 1
PARAMS = [(2.0, 0.05, 5, False), (0.0, 0.05, 5, False), (2.0, 0.0, 5, False), (2.0, 0.05, -1, False), (2.0, 0.05, 5, True), (0.0, 0.0, -1, False), (1.5, 0.0, 0, False)]


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def numpy_denoise(linear, variance, counts, node, normal, position, iterations, sigma_color, sigma_plane, normal_power_log2, same_node):
    """Section 1 of the contract, restated: returns (c, v) after `iterations` levels. Pixels with count 0 keep their input."""
    h, w = counts.shape
    c, v = np.array(linear, dtype=np.float64), np.array(variance, dtype=np.float64)
    valid = counts > 0
    kc = np.float64(sigma_color) * np.float64(sigma_color)
    kp = np.float64(1.0) / (np.float64(sigma_plane) * np.float64(sigma_plane)) if sigma_plane > 0 else np.float64(0.0)
    with np.errstate(all="ignore"):
        for level in range(iterations):
            s = 1 << level
            cs, vs, ws = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
            for j, i in itertools.product(range(-2, 3), range(-2, 3)):  # j outer, i inner
                x0, x1, y0, y1 = max(0, -s * i), min(w, w - s * i), max(0, -s * j), min(h, h - s * j)
                if x0 >= x1 or y0 >= y1:
                    continue  # every tap (i, j) of this level falls outside the film
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + s * j, y1 + s * j), slice(x0 + s * i, x1 + s * i))
                take = valid[P] & valid[Q]
                miss_p, miss_q = node[P] < 0, node[Q] < 0
                take &= miss_p == miss_q
                if same_node:
                    take &= node[P] == node[Q]
                wgt = np.full(take.shape, H5[j + 2] * H5[i + 2])
                if normal_power_log2 >= 0:
                    a = (normal[P][..., 0] * normal[Q][..., 0] + normal[P][..., 1] * normal[Q][..., 1]) + normal[P][..., 2] * normal[Q][..., 2]
                    a = np.where(a > 0, a, 0.0)
                    for _ in range(normal_power_log2):
                        a = a * a
                    wgt = np.where(miss_p, wgt, wgt * a)
                if sigma_plane > 0:
                    e = position[Q] - position[P]
                    d = (normal[P][..., 0] * e[..., 0] + normal[P][..., 1] * e[..., 1]) + normal[P][..., 2] * e[..., 2]
                    t = 1.0 - (d * d) * kp
                    wgt = np.where(miss_p, wgt, wgt * np.where(t > 0, t * t, 0.0))
                if sigma_color > 0:
                    yp, yq = (c[P][..., 0] + c[P][..., 1]) + c[P][..., 2], (c[Q][..., 0] + c[Q][..., 1]) + c[Q][..., 2]
                    dy = yp - yq
                    t = 1.0 - (dy * dy) / (kc * (v[P] + v[Q]) + EPS)
                    wgt = wgt * np.where(t > 0, t * t, 0.0)
                take &= wgt > 0  # (False for a NaN weight)
                cs[P] = np.where(take[..., None], cs[P] + c[Q] * wgt[..., None], cs[P])
                vs[P] = np.where(take, vs[P] + (wgt * wgt) * v[Q], vs[P])
                ws[P] = np.where(take, ws[P] + wgt, ws[P])
            degenerate = ws == 0
            c_new = np.where(degenerate[..., None], c, cs / ws[..., None])
            v_new = np.where(degenerate, v, vs / (ws * ws))
            c, v = np.where(valid[..., None], c_new, c), np.where(valid, v_new, v)
    return c, v


def host_denoise(H, linear, variance, counts, node, normal, position, iterations, sigma_color, sigma_plane, normal_power_log2, same_node, fill=-7.25):
    """pt_test_denoise_host into buffers pre-filled with `fill`."""
    h, w = counts.shape
    lin, var, cnt = np.ascontiguousarray(linear, dtype=np.float64), np.ascontiguousarray(variance, dtype=np.float64), np.ascontiguousarray(counts, dtype=np.uint32)
    nd, nr, ps = np.ascontiguousarray(node, dtype=np.int32), np.ascontiguousarray(normal, dtype=np.float64), np.ascontiguousarray(position, dtype=np.float64)
    p = H.PtDenoiseParams(iterations, H.DENOISE_SAME_NODE if same_node else 0, sigma_color, sigma_plane, normal_power_log2)
    g = H.PtDenoiseGuides(ps.ctypes.data, nr.ctypes.data, nd.ctypes.data)
    out_c, out_v = np.full((h, w, 3), fill), np.full((h, w), fill)
    rc = H.lib().pt_test_denoise_host(w, h, C.byref(p), lin.ctypes.data_as(H._dp), var.ctypes.data_as(H._dp), cnt.ctypes.data_as(H._up), C.byref(g),
                                      out_c.ctypes.data_as(H._dp), out_v.ctypes.data_as(H._dp))
    assert rc == H.OK, rc
    return out_c, out_v


def synthetic(w, h, seed):
    """Seeded inputs that hold every case of the contract where the size has room for it: two planes with different (slightly perturbed) normals and a patch of
    a third node on the first, a miss region, counts of 0 and 1, a leading -0.0 colour, a clean v = 0 region, a zero normal on a hit (the ws == 0 path, with the
    -0.0 colour on it), a NaN position."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    node = np.where(xs < (w + 1) // 2, 0, 1).astype(np.int32)
    node[(ys >= h // 4) & (ys < h // 2) & (xs < w // 4)] = 2
    node[ys >= h - max(h // 4, 1) if h > 2 else ys > h] = -1  # the bottom rows miss (not at 1 x 1)
    hit = node >= 0
    normal = np.zeros((h, w, 3))
    normal[node == 1] = (0.6, 0.0, 0.8)
    normal[(node == 0) | (node == 2)] = (0.0, 0.0, 1.0)
    normal += np.where(hit[..., None], rng.normal(0.0, 0.02, size=(h, w, 3)), 0.0)
    position = np.zeros((h, w, 3))
    position[..., 0], position[..., 1] = xs * 0.1, ys * 0.1
    position[..., 2] = np.where(node == 1, -0.75 * xs * 0.1 + 2.0, 0.0) + rng.normal(0.0, 0.005, size=(h, w))
    position[~hit] = 0.0
    truth = np.where((node == 1)[..., None], (0.2, 0.5, 0.7), (0.6, 0.45, 0.3)) + np.zeros((h, w, 3))
    truth[~hit] = np.stack([xs / max(w, 1), ys / max(h, 1), 0.5 + 0.0 * xs], axis=-1)[~hit]
    counts = np.full((h, w), 8, dtype=np.uint32)
    variance = rng.uniform(0.001, 0.01, size=(h, w))
    linear = truth + rng.normal(0.0, 1.0, size=(h, w, 3)) * np.sqrt(variance / 3.0)[..., None]
    if w * h >= 15:
        pick = rng.permutation(w * h)
        counts.flat[pick[:max(w * h // 16, 1)]] = 0
        ones = pick[max(w * h // 16, 1):max(w * h // 8, 2)]
        counts.flat[ones] = 1
        my = (linear[..., 0] + linear[..., 1]) + linear[..., 2]
        variance.flat[ones] = (my * my).flat[ones]
        clean = (ys < max(h // 5, 1)) & (xs >= w // 2)  # a noise-free region: v = 0 and the exact colour
        variance[clean] = 0.0
        linear[clean] = truth[clean]
        hits = np.flatnonzero(hit & (counts > 0))
        zero_n, nan_p, neg0 = hits[len(hits) // 3], hits[len(hits) // 2], hits[(2 * len(hits)) // 3]
        normal.reshape(-1, 3)[zero_n] = 0.0
        linear.reshape(-1, 3)[zero_n, 0] = -0.0
        position.reshape(-1, 3)[nan_p, 1] = np.nan
        linear.reshape(-1, 3)[neg0, 0] = -0.0
    else:
        linear[0, 0, 0] = -0.0
    return {"linear": linear, "variance": variance, "counts": counts, "node": node, "normal": normal, "position": position, "truth": truth}


def test_the_synthetic_inputs_hold_every_case():
    s = synthetic(67, 37, 5)
    cnt, node = s["counts"], s["node"]
    assert (cnt == 0).any() and (cnt == 1).any() and (cnt == 8).any()
    assert (node < 0).any() and set(np.unique(node)) == {-1, 0, 1, 2}
    assert np.signbit(s["linear"][..., 0][s["linear"][..., 0] == 0]).any(), "a -0.0 colour"
    assert (s["variance"] == 0).any() and np.isnan(s["position"]).any()
    assert (np.all(s["normal"] == 0, axis=-1) & (node >= 0)).any(), "a zero normal on a hit"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("iterations", ITERATIONS)
def test_the_host_replay_is_the_numpy_restatement_bit_for_bit(H, size, iterations):
    w, h = size
    s = synthetic(w, h, 100 + w)
    guides = (s["node"], s["normal"], s["position"])
    for sc, sp, npl2, same in PARAMS:
        got_c, got_v = host_denoise(H, s["linear"], s["variance"], s["counts"], *guides, iterations, sc, sp, npl2, same)
        pre_c, pre_v = np.where((s["counts"] > 0)[..., None], s["linear"], -7.25), np.where(s["counts"] > 0, s["variance"], -7.25)
        want_c, want_v = numpy_denoise(pre_c, pre_v, s["counts"], *guides, iterations, sc, sp, npl2, same)
        what = "%dx%d, %d levels, %r" % (w, h, iterations, (sc, sp, npl2, same))
        assert np.array_equal(bits(got_c), bits(want_c)), what
        assert np.array_equal(bits(got_v), bits(want_v)), what
        untouched = s["counts"] == 0
        assert np.all(got_c[untouched] == -7.25) and np.all(got_v[untouched] == -7.25), "pixels without samples are not written"
        assert np.isfinite(got_c).all() and np.isfinite(got_v).all(), what
        if w * h >= 15 and npl2 >= 0:  # the zero normal on a hit: ws == 0, the input passes through, the sign of its -0.0 included
            at = np.argwhere(np.all(s["normal"] == 0, axis=-1) & (s["node"] >= 0) & (s["counts"] > 0))[0]
            assert np.array_equal(bits(got_c[at[0], at[1]]), bits(s["linear"][at[0], at[1]])) and np.signbit(got_c[at[0], at[1], 0])
            assert bits(got_v[at[0], at[1]]) == bits(s["variance"][at[0], at[1]])


def test_at_eight_levels_only_the_centre_tap_is_left(H):
    """Step 128 is wider than 67 x 37: level 7 averages a pixel with itself, so 8 levels differ from 7 only by (c w) / w and (w w v) / (w w)."""
    s = synthetic(67, 37, 167)
    guides = (s["node"], s["normal"], s["position"])
    c7, v7 = host_denoise(H, s["linear"], s["variance"], s["counts"], *guides, 7, 2.0, 0.0, -1, False)
    c8, v8 = host_denoise(H, s["linear"], s["variance"], s["counts"], *guides, 8, 2.0, 0.0, -1, False)
    w0 = np.float64(0.375) * np.float64(0.375)
    valid = s["counts"] > 0
    assert np.array_equal(bits(c8[valid]), bits((c7[valid] * w0) / w0)) and np.array_equal(bits(v8[valid]), bits(((w0 * w0) * v7[valid]) / (w0 * w0)))


def test_a_clean_gradient_is_not_blurred(H):
    """v = 0 on both sides and different colours: weight 0 - every pixel of a noise-free ramp keeps its exact value (only the centre tap, (c w) / w, is left)."""
    w, h = 17, 9
    ys, xs = np.mgrid[0:h, 0:w]
    lin = np.stack([xs / 64.0, 5.0 * ys / 64.0, 0.25 + 0.0 * xs], axis=-1)  # (i + 5 j != 0 for every other tap: no two taps of a centre share a channel sum)
    node = np.zeros((h, w), dtype=np.int32)
    got_c, got_v = host_denoise(H, lin, np.zeros((h, w)), np.full((h, w), 8, dtype=np.uint32), node, np.zeros((h, w, 3)), np.zeros((h, w, 3)), 5, 2.0, 0.0, -1, False)
    assert np.array_equal(got_c, lin) and not got_v.any()


def test_argument_errors_of_the_host_replay(H):
    w, h = 5, 3
    s = synthetic(w, h, 1)
    lin, var, cnt = s["linear"], s["variance"], s["counts"]
    nd, nr, ps = s["node"], s["normal"], s["position"]
    out_c, out_v = np.full((h, w, 3), 7.0), np.full((h, w), 7.0)
    dp, up = (lambda a: a.ctypes.data_as(H._dp)), (lambda a: a.ctypes.data_as(H._up))
    full = H.PtDenoiseGuides(ps.ctypes.data, nr.ctypes.data, nd.ctypes.data)
    call = lambda p, g, wd=w, ht=h, l=lin, v=var, c=cnt, oc=out_c, ov=out_v: H.lib().pt_test_denoise_host(
        wd, ht, C.byref(p) if p is not None else None, dp(l) if l is not None else None, dp(v) if v is not None else None, up(c) if c is not None else None,
        C.byref(g) if g is not None else None, dp(oc) if oc is not None else None, dp(ov) if ov is not None else None)
    good = H.PtDenoiseParams(3, 0, 2.0, 0.05, 5)
    assert call(good, full) == H.OK
    out_c[:], out_v[:] = 7.0, 7.0
    nan, inf = float("nan"), float("inf")
    for bad in [H.PtDenoiseParams(0, 0, 2.0, 0.05, 5), H.PtDenoiseParams(9, 0, 2.0, 0.05, 5), H.PtDenoiseParams(-1, 0, 2.0, 0.05, 5), H.PtDenoiseParams(3, 2, 2.0, 0.05, 5),
                H.PtDenoiseParams(3, 0, -1.0, 0.05, 5), H.PtDenoiseParams(3, 0, nan, 0.05, 5), H.PtDenoiseParams(3, 0, inf, 0.05, 5), H.PtDenoiseParams(3, 0, 2.0, -0.5, 5),
                H.PtDenoiseParams(3, 0, 2.0, nan, 5), H.PtDenoiseParams(3, 0, 2.0, inf, 5), H.PtDenoiseParams(3, 0, 2.0, 0.05, -2), H.PtDenoiseParams(3, 0, 2.0, 0.05, 8)]:
        assert call(bad, full) == H.ERR_ARGUMENT
    assert call(None, full) == H.ERR_ARGUMENT and call(good, None) == H.ERR_ARGUMENT
    assert call(good, full, l=None) == H.ERR_ARGUMENT and call(good, full, c=None) == H.ERR_ARGUMENT and call(good, full, oc=None, ov=None) == H.ERR_ARGUMENT
    assert call(good, full, wd=0) == H.ERR_ARGUMENT and call(good, full, ht=0) == H.ERR_ARGUMENT
    assert call(good, full, v=None) == H.ERR_ARGUMENT, "no variance: a film without moments, accepted without a colour weight only"
    # the guides each weight needs
    assert call(good, H.PtDenoiseGuides(ps.ctypes.data, nr.ctypes.data, None)) == H.ERR_ARGUMENT
    assert call(good, H.PtDenoiseGuides(ps.ctypes.data, None, nd.ctypes.data)) == H.ERR_ARGUMENT
    assert call(good, H.PtDenoiseGuides(None, nr.ctypes.data, nd.ctypes.data)) == H.ERR_ARGUMENT
    assert call(H.PtDenoiseParams(3, 0, 2.0, 0.0, 5), H.PtDenoiseGuides(None, None, nd.ctypes.data)) == H.ERR_ARGUMENT
    assert call(H.PtDenoiseParams(3, 0, 2.0, 0.05, -1), H.PtDenoiseGuides(ps.ctypes.data, None, nd.ctypes.data)) == H.ERR_ARGUMENT
    assert np.all(out_c == 7.0) and np.all(out_v == 7.0), "a refused call writes nothing"
    assert call(H.PtDenoiseParams(3, 0, 2.0, 0.0, 5), H.PtDenoiseGuides(None, nr.ctypes.data, nd.ctypes.data)) == H.OK
    assert call(H.PtDenoiseParams(3, 0, 2.0, 0.0, -1), H.PtDenoiseGuides(None, None, nd.ctypes.data)) == H.OK
    assert call(H.PtDenoiseParams(3, 0, 0.0, 0.0, -1), H.PtDenoiseGuides(None, None, nd.ctypes.data), v=None) == H.OK
    assert call(good, full, oc=None) == H.OK and call(good, full, ov=None) == H.OK


def prototype_image(seed=2010, w=67, h=37, samples=8, sigma=0.28):
    """The image the filter was prototyped on: two planes with different normals, a miss region with a gradient, `samples` Gaussian samples per pixel, some
    pixels with count 1 and some with count 0. Returns the film a moments film would hold of it (mean, variance by the count-1 rule, counts), guides and truth."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    node = np.where(xs < 30, 0, 1).astype(np.int32)
    node[ys >= 28] = -1
    hit = node >= 0
    normal = np.zeros((h, w, 3))
    normal[node == 0], normal[node == 1] = (0.0, 0.0, 1.0), (0.6, 0.0, 0.8)
    position = np.zeros((h, w, 3))
    position[..., 0], position[..., 1] = xs * 0.1, ys * 0.1
    position[..., 2] = np.where(node == 1, -0.75 * xs * 0.1 + 2.25, 0.0)
    position[~hit] = 0.0
    truth = np.where((node == 1)[..., None], (0.2, 0.5, 0.7), (0.6, 0.45, 0.3)) + np.zeros((h, w, 3))
    truth[~hit] = np.stack([xs / w, 0.3 + 0.0 * xs, 1.0 - xs / w], axis=-1)[~hit]
    counts = np.full((h, w), samples, dtype=np.uint32)
    pick = rng.permutation(w * h)
    counts.flat[pick[:40]] = 0
    counts.flat[pick[40:100]] = 1
    draws = truth[None] + rng.normal(0.0, sigma, size=(samples, h, w, 3))
    n = counts.astype(np.float64)
    use = np.arange(samples)[:, None, None] < counts[None]
    mean = np.where(counts[..., None] > 0, (draws * use[..., None]).sum(axis=0) / np.maximum(n, 1.0)[..., None], 0.0)
    y = draws.sum(axis=-1)
    my = mean.sum(axis=-1)
    var_y = np.where(counts >= 2, ((y - my[None]) ** 2 * use).sum(axis=0) / np.maximum(n - 1.0, 1.0), 0.0)
    variance = np.where(counts >= 2, var_y / np.maximum(n, 1.0), my * my)  # (standard error of the mean)^2; at count 1 the sample's own magnitude
    return {"linear": mean, "variance": variance, "counts": counts, "node": node, "normal": normal, "position": position, "truth": truth}


def test_five_levels_at_least_halve_the_error_of_the_prototypes_image(H):
    """The one quality condition: sigma_color 2, sigma_plane 0.05, power 32, 5 levels - the RMS error to the truth is at most half of the input's (the numpy
    prototype measured 0.34 x), every value finite, and nothing leaks across the miss boundary (checked with the colour and plane weights off, where only the miss
    rule stands between the two)."""
    s = prototype_image()
    guides = (s["node"], s["normal"], s["position"])
    valid = s["counts"] > 0
    rms = lambda c: float(np.sqrt(np.mean((c[valid] - s["truth"][valid]) ** 2)))
    before = rms(s["linear"])
    got_c, got_v = host_denoise(H, s["linear"], s["variance"], s["counts"], *guides, 5, 2.0, 0.05, 5, False)
    after = rms(got_c)
    print("rms to the truth: input %.4f, after 5 levels %.4f (%.2f x)" % (before, after, after / before))
    assert np.isfinite(got_c[valid]).all() and np.isfinite(got_v[valid]).all()
    assert after <= 0.5 * before, (before, after)
    want_c, want_v = numpy_denoise(np.where(valid[..., None], s["linear"], -7.25), np.where(valid, s["variance"], -7.25), s["counts"], *guides, 5, 2.0, 0.05, 5, False)
    assert np.array_equal(bits(got_c), bits(want_c)) and np.array_equal(bits(got_v), bits(want_v))
    # no leak: a noise-free film (every pixel its truth, v = 0) filtered with the colour and plane weights off. Hits mix across the two planes a little
    # (0.8^32 of a weight) but green is 0.45 or 0.5 on every hit and 0.3 on every miss: any colour from the miss region would pull a hit's green below 0.45,
    # and any from a hit would lift a miss's above 0.3. A weighted mean of 25 values leaves their hull by at most 26 roundings per level: 5 x 26 x 2^-53 < 1e-13.
    clean_c, _ = host_denoise(H, s["truth"], np.zeros_like(s["variance"]), s["counts"], *guides, 5, 0.0, 0.0, 5, False)
    hits, misses = (s["node"] >= 0) & valid, (s["node"] < 0) & valid
    assert clean_c[hits][:, 1].min() >= 0.45 - 1e-13 and clean_c[hits][:, 1].max() <= 0.5 + 1e-13, "a hit pixel took colour from the miss region"
    assert np.abs(clean_c[misses][:, 1] - 0.3).max() <= 1e-13, "a miss pixel took colour from a hit"
