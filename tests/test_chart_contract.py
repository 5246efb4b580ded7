"""The contract of the chart pass without a GPU (portrayer_amd/csrc/pt_chart.h): the numpy restatement tests/chart_restate.py - written from the
header's comments - against the host replay pt_test_chart_host, which compiles the functions the kernels compile, in every bit of every output; and the
properties the contract is chosen for: inclusive coverage, the lowest index owns, a triangle that does not take part changes nothing, and no texel centre
falls between two triangles that share an edge."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import chart_restate as R  # noqa: E402

CASES = R.cases()
(FWD, NRM), (IFWD, INRM) = R.node_matrices()
SEEDS = range(20)
GRID_SIZES = [(64, 64), (67, 37)]


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def both(H, fwd, nrm, v, n, uv, w, h, flags=0):
    a = R.chart(fwd, nrm, v, n, uv, w, h, flags)
    b = R.host(H.lib(), H, fwd, nrm, v, n, uv, w, h, flags)
    for k in ("position", "normal", "tri", "covered"):
        assert R.same_bits(a[k], b[k]), "%s differs at %d of %d texels" % (k, int(np.sum(np.any((a[k] != b[k]).reshape(w * h, -1), axis=1))), w * h)
    return a


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("smooth", [False, True])
def test_host_replay_equals_the_restatement_in_every_bit(H, name, smooth):
    """every case at every size, on a rotated, non-uniformly scaled node, flat and smooth, with and without PT_CHART_FLIP_NORMAL"""
    v, n, uv, sizes = CASES[name]
    for (w, h) in sizes:
        plain = both(H, FWD, NRM, v, n if smooth else None, uv, w, h)
        flipped = both(H, FWD, NRM, v, n if smooth else None, uv, w, h, R.FLIP_NORMAL)
        assert R.same_bits(flipped["normal"][plain["covered"] == 1], -plain["normal"][plain["covered"] == 1])
        assert R.same_bits(flipped["position"], plain["position"]) and R.same_bits(flipped["tri"], plain["tri"])
        own = plain["covered"] == 1
        assert np.all(plain["tri"][~own] == -1) and np.all(plain["position"][~own] == 0.0) and np.all(plain["normal"][~own] == 0.0)
        assert np.all(np.abs(np.linalg.norm(plain["normal"][own], axis=1) - 1.0) < 1e-15 * 4)
        ident = both(H, IFWD, INRM, v, n if smooth else None, uv, w, h)
        assert R.same_bits(ident["tri"], plain["tri"])


def test_one_triangle_at_one_texel(H):
    v, n, uv, _ = CASES["one_triangle"]
    a = both(H, IFWD, INRM, v, None, uv, 1, 1)
    assert a["covered"][0, 0] == 1 and a["tri"][0, 0] == 0  # (0.5, 0.5) lies inside the triangle
    # the identity node: the point is the interpolated model point (2u - 1, 2v - 1, .) at u = v = 0.5 up to rounding, the flat normal the face's
    assert np.allclose(a["position"][0, 0, :2], [0.0, 0.0], atol=1e-15)


def test_the_quads_diagonal_is_inclusive_and_the_lower_index_owns_it(H):
    v, n, uv, _ = CASES["quad_diagonal"]
    a = both(H, IFWD, INRM, v, None, uv, 8, 8)
    assert np.all(a["covered"] == 1)
    _, count = R.coverage(uv, 8, 8)
    count = count.reshape(8, 8)
    diag = [(7 - k, k) for k in range(8)]  # (row, column): v = 1 is the top row, so u = v runs from the bottom left to the top right
    assert all(count[r, c] == 2 for r, c in diag) and int(np.sum(count == 2)) == 8 and np.all(count >= 1)
    assert all(a["tri"][r, c] == 0 for r, c in diag)


def test_both_windings_cover_the_same_texels_with_the_same_points(H):
    v, n, uv, _ = CASES["one_triangle"]
    v2, n2, uv2, _ = CASES["other_winding"]
    a, b = both(H, FWD, NRM, v, n, uv, 7, 5), both(H, FWD, NRM, v2, n2, uv2, 7, 5)
    assert R.same_bits(a["covered"], b["covered"]) and int(a["covered"].sum()) > 0
    assert np.allclose(a["position"], b["position"], atol=1e-14) and np.allclose(a["normal"], b["normal"], atol=1e-14)  # (another summation order: not the same bits)


def test_triangles_that_do_not_take_part_own_nothing_and_change_nothing(H):
    v, n, uv, sizes = CASES["bad_among_good"]
    gv, gn, guv, _ = CASES["good_alone"]
    back = np.array([-1, 0, -1, -1, 1, -1])  # the mixed set's index -> the good set's
    for (w, h) in sizes:
        a, g = both(H, FWD, NRM, v, n, uv, w, h), both(H, FWD, NRM, gv, gn, guv, w, h)
        assert set(np.unique(a["tri"])) <= {-1, 1, 4}
        assert R.same_bits(np.where(a["tri"] >= 0, back[a["tri"]], -1).astype(np.int32), g["tri"])
        assert R.same_bits(a["position"], g["position"]) and R.same_bits(a["normal"], g["normal"]) and R.same_bits(a["covered"], g["covered"])


def test_uvs_outside_the_unit_square_fall_off_the_map(H):
    v, n, uv, sizes = CASES["outside_unit"]
    for (w, h) in sizes:
        a = both(H, FWD, NRM, v, n, uv, w, h)
        assert not np.any(a["tri"] == 2), "a triangle wholly outside [0, 1] owns nothing: no wrap"
        assert int(a["covered"].sum()) > 0


def test_where_charts_overlap_the_lower_index_wins(H):
    v, n, uv, sizes = CASES["overlap"]
    for (w, h) in sizes:
        a = both(H, FWD, NRM, v, n, uv, w, h)
        st, part = R.corners(uv, w, h)
        o, _ = R.orientation(st)
        ps, pt = R.centres(w, h)
        cov = R.weights(st, o, ps, pt)[4]
        assert int(np.sum(cov.sum(axis=0) >= 2)) > 0, "the case has overlap"
        want = np.where(cov.any(axis=0), np.argmax(cov, axis=0), -1)
        assert np.array_equal(a["tri"].ravel(), want)
        assert np.array_equal(np.unique(a["tri"]), [-1, 0, 1, 2])


def test_flat_and_smooth_differ_only_in_the_normal(H):
    v, n, uv, _ = CASES["grid"]
    a, b = both(H, FWD, NRM, v, None, uv, 64, 64), both(H, FWD, NRM, v, n, uv, 64, 64)
    assert R.same_bits(a["position"], b["position"]) and R.same_bits(a["tri"], b["tri"]) and not R.same_bits(a["normal"], b["normal"])


@pytest.mark.parametrize("size", GRID_SIZES)
def test_watertight_no_texel_centre_falls_between_triangles(size):
    """An 8 x 8 grid of quads (128 triangles) over the exact unit square, interior UV vertices moved by random offsets below a third of a cell and then onto
    doubles for which edges pass through texel centres up to rounding (chart_restate.grid_uv says how and why: plain random offsets never put a centre where an
    edge function's sign is in doubt, and the guard below would test nothing). Over 20 seeds EVERY texel is covered: the cap is zero. The guard: the same grids
    with every edge evaluated from the triangle's own first endpoint - not the contract - leave at least one texel uncovered over the 20 seeds."""
    w, h = size
    uncovered, uncovered_plain = 0, 0
    for seed in SEEDS:
        uv = R.grid_uv(seed, w, h)
        assert uv.shape == (128, 6)
        uncovered += int(np.sum(R.coverage(uv, w, h)[1] == 0))
        uncovered_plain += int(np.sum(R.coverage(uv, w, h, canonical=False)[1] == 0))
    print("%d x %d, 20 seeds: uncovered %d with canonical edges, %d without" % (w, h, uncovered, uncovered_plain))
    assert uncovered == 0
    assert uncovered_plain >= 1, "the guard: these grids do not tell canonical edges from plain ones"


def test_the_grid_is_watertight_in_the_host_replay_too(H):
    for (w, h) in GRID_SIZES:
        for seed in (0, 7, 19):
            uv = R.grid_uv(seed, w, h)
            v, n = R._tri_from_uv(uv)
            assert np.all(both(H, FWD, NRM, v, n, uv, w, h)["covered"] == 1)


def test_the_hook_refuses_what_pt_chart_refuses(H):
    import ctypes as C
    lib = H.lib()
    v, n, uv, _ = CASES["one_triangle"]
    tri = np.zeros((2, 2), dtype=np.int32)
    b = H.PtChartBuffers(tri=tri.ctypes.data_as(H._ip))
    dp = lambda a: np.ascontiguousarray(a).ctypes.data_as(H._dp)
    args = lambda w, h, flags, bufs: (dp(IFWD), dp(INRM), 1, dp(v), None, dp(uv), w, h, flags, bufs)
    assert lib.pt_test_chart_host(*args(2, 2, 0, C.byref(b))) == H.OK
    for bad in (args(0, 2, 0, C.byref(b)), args(2, 0, 0, C.byref(b)), args(8192, 4096, 0, C.byref(b)), args(2, 2, 2, C.byref(b)), args(2, 2, 0, None),
                args(2, 2, 0, C.byref(H.PtChartBuffers()))):
        assert lib.pt_test_chart_host(*bad) == H.ERR_ARGUMENT
