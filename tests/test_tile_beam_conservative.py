"""The list kernel opens the scene tree with the beam of a whole 8x8 tile (pt_pixel_list.h 7.: pt_beam_setup over a rectangle of sample positions; pt_api.hip:
pt_pixel_list_kernel), so the obligation of the pixel's beam holds for a rectangle: whatever the walk's own f32 slab test accepts for the ray of a sample position inside
[x, x + nx] x [y, y + ny], the rectangle's beam accepts - otherwise an ancestor of a leaf that is hit would stay shut. Through the host build of that code
(pt_test_rect_beam: no GPU), on the 2.6 million fixed-seed cases of test_pixel_list_conservative.py (near misses, an eye inside boxes, axis-aligned views, ranges
touching zero, huge and tiny scales), each with rectangles of 8x8, 1x1, 8x1 and 1x8 around the case's pixel - the 8x8 ones half on the image's tile grid, half anywhere,
since a slice's tiles start at its own corner:

1. no case where the walk (the mixed-sign form or the form of the ray's octant, no bound on t) accepts the sample's ray and the rectangle's beam rejects;
2. no stored bound above the exact entry parameter of the sample's f64 ray (long double with an explicit error bound, and rationals for a sample);
3. for nx = ny = 1 accept and bound are pt_test_pixel_beam's, bit for bit.

The sample position is the rectangle's corner plus (the pixel's offset in it + the case's jitter), so it is one of the pixel's own sample positions up to one rounding.
Printed, not asserted: the cases where the pixel's beam accepts and the 8x8 beam around it rejects. That is no error - the two beams' f32 constants are rounded
independently, and such a box grazes the pixel's beam without any ray hitting it - but it is why records may differ from a walk with the pixel beams alone."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import test_pixel_list_conservative as P

SHAPES = [(8, 8), (1, 1), (8, 1), (1, 8)]


def rect_hook(cam, rect, off, lo, hi):
    from portrayer_amd import _hip as H
    n = len(cam)
    cam, rect, off, lo, hi = (np.ascontiguousarray(a) for a in (cam, rect, off, lo, hi))
    assert rect.dtype == np.uint32 and rect.shape == (n, 4) and off.shape == (n, 2)
    accept = np.zeros(n, np.int32)
    walk = np.zeros(n, np.int32)
    bound = np.zeros(n, np.float32)
    rays = np.zeros((n, 6))
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    rc = H.lib().pt_test_rect_beam(n, cam.ctypes.data_as(dp), rect.ctypes.data_as(C.POINTER(C.c_uint32)), off.ctypes.data_as(dp), lo.ctypes.data_as(fp), hi.ctypes.data_as(fp),
                                   accept.ctypes.data_as(ip), bound.ctypes.data_as(fp), walk.ctypes.data_as(ip), rays.ctypes.data_as(dp))
    assert rc == 0
    return accept, bound, walk, rays


def rectangles(rng, pix, jit, nx, ny):
    """A rectangle of nx x ny pixels around each case's pixel and the sample's offset from its corner."""
    n = len(pix)
    x, y = pix[:, 0].astype(np.int64), pix[:, 1].astype(np.int64)
    on_grid = rng.random(n) < 0.3
    ox, oy = rng.integers(0, nx, n), rng.integers(0, ny, n)
    # a jitter at an end of [0, 1) mostly sits in the rectangle's first or last column / row: the sample's ray then runs along the rectangle's edge, where a box that
    # grazes the ray grazes the rectangle's beam
    at_edge = rng.random((n, 2)) < 0.7
    ox = np.where(at_edge[:, 0] & (jit[:, 0] == 0.0), 0, np.where(at_edge[:, 0] & (jit[:, 0] == P.ONE_BELOW), nx - 1, ox))
    oy = np.where(at_edge[:, 1] & (jit[:, 1] == 0.0), 0, np.where(at_edge[:, 1] & (jit[:, 1] == P.ONE_BELOW), ny - 1, oy))
    ox = np.where(on_grid, x % nx, np.minimum(ox, x))  # (the corner stays at or above 0)
    oy = np.where(on_grid, y % ny, np.minimum(oy, y))
    rect = np.stack([x - ox, y - oy, np.full(n, nx), np.full(n, ny)], axis=1).astype(np.uint32)
    off = np.stack([ox + jit[:, 0], oy + jit[:, 1]], axis=1)
    assert np.all(off >= 0.0) and np.all(off[:, 0] <= nx) and np.all(off[:, 1] <= ny)
    return rect, off


@pytest.fixture(scope="module")
def cases():
    cam, pix, jit, lo, hi, cls, names = P.build_cases()
    pixel = P.hook(cam, pix, jit, lo, hi)
    rng = np.random.default_rng(20261020)
    by_shape = {}
    for nx, ny in SHAPES:
        rect, off = rectangles(rng, pix, jit, nx, ny)
        by_shape[(nx, ny)] = (rect, off) + rect_hook(cam, rect, off, lo, hi)
    return cam, pix, jit, lo, hi, cls, names, pixel, by_shape


def test_case_set_is_what_the_module_promises(cases):
    cam, pix, jit, lo, hi, cls, names, pixel, by_shape = cases
    assert len(cam) >= 2_600_000 and sorted(by_shape) == sorted(SHAPES)
    for k, name in enumerate(names):
        assert (cls == k).sum() >= 100_000, name
    for (nx, ny), (rect, off, accept, bound, walk, rays) in by_shape.items():
        assert np.all(rect[:, 2] == nx) and np.all(rect[:, 3] == ny)
        assert np.all(rect[:, 0] <= pix[:, 0]) and np.all(pix[:, 0] < rect[:, 0].astype(np.int64) + nx) and np.all(rect[:, 1] <= pix[:, 1]) and np.all(pix[:, 1] < rect[:, 1].astype(np.int64) + ny)
        assert np.array_equal(rays[:, 0:3], cam[:, 0:3])  # the rays start at the eye
        # Both answers occur in the classes made to graze, in every shape - also among the boxes that graze a ray along the rectangle's edge, which are the near misses
        # of a rectangle larger than the pixel (a box that grazes a ray through the middle of an 8x8 tile lies well inside the tile's beam). The sample sits in every
        # column and row of its rectangle.
        edge = (off[:, 0] == 0.0) | (off[:, 0] >= nx) | (off[:, 1] == 0.0) | (off[:, 1] >= ny)
        assert edge.mean() > 0.2
        for name in ("around the sample's ray", "grazing", "flat"):
            sl = cls == names.index(name)
            assert 0.05 < (walk[sl] != 0).mean() < 0.999 and (accept[sl] == 0).sum() >= 1000, (nx, ny, name, (walk[sl] != 0).mean(), (accept[sl] == 0).sum())
        sl = (cls == names.index("grazing")) & edge
        print("    %dx%d: %d grazing boxes at a ray along the rectangle's edge, the walk accepts %.1f %%, the rectangle's beam rejects %.1f %%"
              % (nx, ny, int(sl.sum()), 100.0 * (walk[sl] != 0).mean(), 100.0 * (accept[sl] == 0).mean()))
        assert sl.sum() >= 50_000 and (accept[sl] == 0).sum() >= 1000 and (walk[sl] != 0).sum() >= 1000
        assert len(np.unique(np.floor(np.minimum(off[:, 0], nx - 0.5)))) == nx and len(np.unique(np.floor(np.minimum(off[:, 1], ny - 0.5)))) == ny
        assert accept[cls == names.index("contains the eye")].all()


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_the_rectangles_beam_accepts_what_the_walk_accepts(cases, shape):
    cam, pix, jit, lo, hi, cls, names, pixel, by_shape = cases
    rect, off, accept, bound, walk, rays = by_shape[shape]
    bad = np.nonzero((walk != 0) & (accept == 0))[0]
    assert len(bad) == 0, (shape, len(bad), [(names[cls[i]], cam[i], rect[i], off[i], lo[i], hi[i]) for i in bad[:3]])
    print("    %dx%d: walk accepts %.1f %%, the rectangle's beam %.1f %% of %d cases" % (shape[0], shape[1], 100.0 * (walk != 0).mean(), 100.0 * accept.mean(), len(cam)))


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_the_stored_bound_lies_below_the_exact_entry_parameter(cases, shape):
    cam, pix, jit, lo, hi, cls, names, pixel, by_shape = cases
    rect, off, accept, bound, walk, rays = by_shape[shape]
    o, d = rays[:, 0:3], rays[:, 3:6]
    tn_lo, tn_hi, meets = P.entry_parameter(o, d, lo, hi)
    acc = accept != 0
    assert np.all(bound[acc] >= 0.0) and np.all(np.isfinite(bound[acc])) and np.all(bound[~acc] == 0.0)
    bad = np.nonzero(acc & (bound.astype(P.LD) > tn_lo))[0]
    assert len(bad) == 0, (shape, len(bad), [(names[cls[i]], float(bound[i]), float(tn_lo[i]), cam[i], rect[i], off[i], lo[i], hi[i]) for i in bad[:3]])
    rng = np.random.default_rng(7)
    for k, name in enumerate(names):  # the long double bound itself, against rationals
        idx = np.nonzero(acc & (cls == k))[0]
        for i in rng.choice(idx, 200, replace=False):
            assert Fraction(float(bound[i])) <= P.exact_entry(o[i], d[i], lo[i], hi[i]), (shape, name, i)


def test_a_rectangle_of_one_pixel_is_the_pixels_beam_bit_for_bit(cases):
    cam, pix, jit, lo, hi, cls, names, pixel, by_shape = cases
    p_accept, p_bound, p_walk, p_rays = pixel
    rect, off, accept, bound, walk, rays = by_shape[(1, 1)]
    assert np.array_equal(rect[:, 0:2], pix) and np.array_equal(off, jit)
    assert np.array_equal(accept, p_accept) and np.array_equal(walk, p_walk)
    assert np.array_equal(bound.view(np.uint32), p_bound.view(np.uint32))
    assert np.array_equal(rays.view(np.uint64), p_rays.view(np.uint64))


def test_report_boxes_a_pixels_beam_accepts_and_its_tiles_beam_rejects(cases):
    """A figure, no criterion: such a box grazes the pixel's beam and no ray hits it (tests 1 of both modules), so a list without it is as good."""
    cam, pix, jit, lo, hi, cls, names, pixel, by_shape = cases
    p_accept = pixel[0]
    for shape in [(8, 8), (8, 1), (1, 8)]:
        accept = by_shape[shape][2]
        only = (p_accept != 0) & (accept == 0)
        print("    %dx%d: the pixel's beam accepts and the rectangle's rejects in %d of %d cases (%s)"
              % (shape[0], shape[1], int(only.sum()), len(cam), ", ".join("%s: %d" % (names[k], int((only & (cls == k)).sum())) for k in range(len(names)) if (only & (cls == k)).any()) or "none"))
        assert not np.any(only & (by_shape[shape][4] != 0))  # (what test 1 says again: none of them is a box the walk accepts for the sample)
