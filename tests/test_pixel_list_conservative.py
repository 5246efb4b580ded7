"""The beam test behind the primary rays' per-pixel candidate lists (pt_pixel_list.h: pt_beam_setup, pt_beam_box) may only err towards listing more leaves.
Through the host build of that code (pt_test_pixel_beam: no GPU) 2.6 million fixed-seed cases - a camera, a pixel, a sample position inside it, a box:

1. whenever the walk's own f32 slab test (pt_slab_pk2 with pt_raypk's constants, the mixed-sign form or the form of the ray's octant, no bound on t) accepts the box for
   the sample's ray, the pixel's beam test accepts it. Zero tolerance: a leaf the walk would test and the list lacks could change a pixel;
2. for every accepted pair the stored bound is at most the exact entry parameter of the sample's f64 ray into the box, max(entering parameters of the three slabs, 0):
   in 80-bit long double with an explicit error bound (a parameter (P - o) / d takes two roundings of 2^-64: within |T| 2^-62), and in rational arithmetic for a sample.

Cameras as the host layer builds them (look_at inverse, tan(fovy / 2)): eye distances from 1e-3 to 1e6, fovy from 5 to 120 degrees, views exactly along an axis and oblique
ones. Pixels at the image centre, on the centre row and column (where a direction range straddles zero), in the corners and at random; jitters at random, 0 and 1 - 2^-53.
Boxes around a point of the sample's ray or of another ray through the pixel, in front of the eye and behind it; boxes that graze the sample's ray from both sides at
offsets from 1e-7 to 1e-2 of their size; boxes that contain the eye; boxes flat in one axis; boxes at +-1e18.

The share of boxes accepted although the walk turns them down for the case's sample is printed per class; it is no pass criterion (a box off this sample's ray may well
be reached by another ray through the pixel: the figure bounds the beam's slack from above)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

LD = np.longdouble
EPS = LD(2.0) ** -62
ONE_BELOW = 1.0 - 2.0 ** -53


def log_uniform(rng, lo, hi, shape):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), shape))


def boxes_outward(lo64, hi64):
    lo = lo64.astype(np.float32)
    hi = hi64.astype(np.float32)
    lo = np.where(lo.astype(np.float64) > lo64, np.nextafter(lo, np.float32(-np.inf)), lo)
    hi = np.where(hi.astype(np.float64) < hi64, np.nextafter(hi, np.float32(np.inf)), hi)
    return np.clip(lo, np.float32(-1e18), np.float32(1e18)), np.clip(hi, np.float32(-1e18), np.float32(1e18))


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def cameras(rng, n):
    """n x 19: eye, rows 0..2 of view_to_world, fov_factor, aspect, width, height - and the image sizes."""
    axes = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
    along = rng.random(n) < 0.4
    k = rng.integers(0, 6, n)
    fwd = np.where(along[:, None], axes[k], unit(rng.normal(size=(n, 3))))
    up = np.where(along[:, None], axes[(k + 2) % 6], unit(rng.normal(size=(n, 3))))
    s = unit(np.cross(fwd, up))
    u = np.cross(s, fwd)
    dist = log_uniform(rng, 1e-3, 1e6, (n, 1))
    centre = rng.normal(size=(n, 3)) * rng.choice([0.0, 1.0, 1e3], (n, 1))
    centre = np.where(along[:, None] & (rng.random((n, 1)) < 0.5), np.round(centre), centre)  # eyes ON an axis: coordinates exactly 0
    eye = centre - fwd * dist
    sizes = np.array([[64, 48], [1920, 1080], [7, 5], [93, 61], [8, 8]])
    wh = sizes[rng.integers(0, len(sizes), n)].astype(np.float64)
    fovy = np.radians(rng.choice([5.0, 20.0, 45.0, 60.0, 90.0, 120.0], n))
    cam = np.zeros((n, 19))
    cam[:, 0:3] = eye
    for r in range(3):
        cam[:, 3 + 4 * r + 0] = s[:, r]
        cam[:, 3 + 4 * r + 1] = u[:, r]
        cam[:, 3 + 4 * r + 2] = -fwd[:, r]
        cam[:, 3 + 4 * r + 3] = eye[:, r]
    cam[:, 15] = np.tan(fovy / 2.0)
    cam[:, 16] = wh[:, 0] / wh[:, 1]
    cam[:, 17] = wh[:, 0]
    cam[:, 18] = wh[:, 1]
    return cam, wh


def pixels_and_jitters(rng, wh):
    n = len(wh)
    w, h = wh[:, 0].astype(np.int64), wh[:, 1].astype(np.int64)
    kind = rng.integers(0, 5, n)
    x = rng.integers(0, 1 << 30, n) % w
    y = rng.integers(0, 1 << 30, n) % h
    cx, cy = w // 2 - rng.integers(0, 2, n) * (1 - w % 2), h // 2 - rng.integers(0, 2, n) * (1 - h % 2)  # (even sizes: either pixel beside the centre line)
    x = np.where((kind == 0) | (kind == 2), cx, x)   # 0: the centre pixel, 1: the centre row, 2: the centre column, 3: a corner, 4: anywhere
    y = np.where((kind == 0) | (kind == 1), cy, y)
    x = np.where(kind == 3, rng.integers(0, 2, n) * (w - 1), x)
    y = np.where(kind == 3, rng.integers(0, 2, n) * (h - 1), y)
    j = rng.random((n, 2))
    edge = rng.random((n, 2))
    j = np.where(edge < 0.2, 0.0, np.where(edge < 0.4, ONE_BELOW, j))
    return np.stack([x, y], axis=1).astype(np.uint32), j


def hook(cam, pix, jit, lo, hi):
    from portrayer_amd import _hip as H
    n = len(cam)
    cam, pix, jit, lo, hi = (np.ascontiguousarray(a) for a in (cam, pix, jit, lo, hi))
    accept = np.zeros(n, np.int32)
    walk = np.zeros(n, np.int32)
    bound = np.zeros(n, np.float32)
    rays = np.zeros((n, 6))
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    rc = H.lib().pt_test_pixel_beam(n, cam.ctypes.data_as(dp), pix.ctypes.data_as(C.POINTER(C.c_uint32)), jit.ctypes.data_as(dp), lo.ctypes.data_as(fp), hi.ctypes.data_as(fp),
                                    accept.ctypes.data_as(ip), bound.ctypes.data_as(fp), walk.ctypes.data_as(ip), rays.ctypes.data_as(dp))
    assert rc == 0
    return accept, bound, walk, rays


def build_cases():
    rng = np.random.default_rng(20261012)
    n = 2_600_000
    cam, wh = cameras(rng, n)
    pix, jit = pixels_and_jitters(rng, wh)
    zero = np.zeros((n, 3), np.float32)
    _, _, _, rays = hook(cam, pix, jit, zero, zero)           # the cases' own sample rays
    jit2 = np.where(rng.random((n, 2)) < 0.5, rng.random((n, 2)), rng.choice([0.0, ONE_BELOW], (n, 2)))
    _, _, _, rays2 = hook(cam, pix, jit2, zero, zero)         # another ray through the same pixel
    o, d = rays[:, 0:3], rays[:, 3:6]
    assert np.all(np.abs(np.linalg.norm(d, axis=1) - 1.0) < 1e-12)
    cls = rng.choice(7, n, p=[0.30, 0.10, 0.25, 0.10, 0.10, 0.10, 0.05])
    names = ["around the sample's ray", "around another ray of the pixel", "grazing", "contains the eye", "flat", "behind the eye", "at 1e18"]
    behind = cls == 5
    t = log_uniform(rng, 1e-4, 1e7, (n, 1)) * np.where(behind[:, None], -1.0, 1.0)
    dd = np.where((cls == 1)[:, None], rays2[:, 3:6], d)
    p = o + t * dd
    reach = np.abs(t)
    half = reach * log_uniform(rng, 1e-7, 3.0, (n, 3))
    off = half * rng.uniform(-1.6, 1.6, (n, 3)) * rng.choice([0.0, 1.0], (n, 1), p=[0.3, 0.7])
    # grazing: on one or two axes the point of the ray lies at the box's face, just inside or just outside by 1e-7 .. 1e-2 of the box's size there
    g = cls == 2
    gaxes = rng.random((n, 3)) < 0.5
    gaxes[np.arange(n), rng.integers(0, 3, n)] = True
    side = rng.choice([-1.0, 1.0], (n, 3))
    delta = log_uniform(rng, 1e-7, 1e-2, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    graze_off = side * half * (1.0 + delta)
    inner_off = half * rng.uniform(-0.9, 0.9, (n, 3))
    off = np.where(g[:, None], np.where(gaxes, graze_off, inner_off), off)
    c = p + off
    lo64, hi64 = c - half, c + half
    # boxes that contain the eye
    e = cls == 3
    ext_lo, ext_hi = log_uniform(rng, 1e-9, 1e3, (n, 3)), log_uniform(rng, 1e-9, 1e3, (n, 3))
    scale = np.maximum(np.abs(o), 1e-3)
    lo64 = np.where(e[:, None], o - ext_lo * scale, lo64)
    hi64 = np.where(e[:, None], o + ext_hi * scale, hi64)
    # at +-1e18
    f = cls == 6
    cf = log_uniform(rng, 1e9, 1e18, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    hf = np.abs(cf) * log_uniform(rng, 1e-3, 4.0, (n, 3))
    lo64 = np.where(f[:, None], cf - hf, lo64)
    hi64 = np.where(f[:, None], cf + hf, hi64)
    lo, hi = boxes_outward(lo64, hi64)
    # flat in one axis: both planes the same f32
    fl = cls == 4
    r = np.arange(n)[fl]
    k = rng.integers(0, 3, len(r))
    mid = (c[r, k]).astype(np.float32)
    lo[r, k] = mid
    hi[r, k] = mid
    return cam, pix, jit, lo, hi, cls, names


def entry_parameter(o, d, lo, hi):
    """Lower and upper bounds (long double, EPS) of max(entering parameters, 0), and whether the exact ray certainly / possibly meets the box."""
    n = len(o)
    tn_lo, tn_hi = np.zeros(n, LD), np.zeros(n, LD)
    tf_lo, tf_hi = np.full(n, np.inf, LD), np.full(n, np.inf, LD)
    empty = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for k in range(3):
            ok, dk = o[:, k].astype(LD), d[:, k].astype(LD)
            l, h = lo[:, k].astype(LD), hi[:, k].astype(LD)
            zero = d[:, k] == 0.0
            empty |= zero & ((o[:, k] < lo[:, k].astype(np.float64)) | (o[:, k] > hi[:, k].astype(np.float64)))
            dk = np.where(zero, LD(1.0), dk)
            a, b = (l - ok) / dk, (h - ok) / dk
            e, f = np.minimum(a, b), np.maximum(a, b)
            e = np.where(zero, -np.inf, e)
            f = np.where(zero, np.inf, f)
            we, wf = np.where(zero, LD(0.0), np.abs(e) * EPS), np.where(zero, LD(0.0), np.abs(f) * EPS)
            tn_lo = np.maximum(tn_lo, e - we)
            tn_hi = np.maximum(tn_hi, e + we)
            tf_hi = np.minimum(tf_hi, f + wf)
            tf_lo = np.minimum(tf_lo, f - wf)
    meets = ~empty & (tn_lo <= tf_hi)
    return tn_lo, tn_hi, meets


def exact_entry(o, d, lo, hi):
    tn = Fraction(0)
    for k in range(3):
        ok, dk, l, h = Fraction(float(o[k])), Fraction(float(d[k])), Fraction(float(lo[k])), Fraction(float(hi[k]))
        if dk == 0:
            continue
        tn = max(tn, min((l - ok) / dk, (h - ok) / dk))
    return tn


@pytest.fixture(scope="module")
def cases():
    cam, pix, jit, lo, hi, cls, names = build_cases()
    accept, bound, walk, rays = hook(cam, pix, jit, lo, hi)
    return cam, pix, jit, lo, hi, cls, names, accept, bound, walk, rays


def test_case_set_is_what_the_module_promises(cases):
    cam, pix, jit, lo, hi, cls, names, accept, bound, walk, rays = cases
    assert len(cam) >= 2_000_000 and np.all(lo <= hi) and np.abs(lo).max() <= 1e18 and np.abs(hi).max() <= 1e18
    assert np.all(pix[:, 0] < cam[:, 17]) and np.all(pix[:, 1] < cam[:, 18]) and jit.min() == 0.0 and jit.max() == ONE_BELOW
    dist = np.linalg.norm(rays[:, 0:3] - (cam[:, 0:3] + 0.0), axis=1)
    assert dist.max() == 0.0  # the rays start at the eye
    for k, name in enumerate(names):
        sl = cls == k
        assert sl.sum() >= 100_000, name
        if name in ("around the sample's ray", "grazing", "flat"):
            assert 0.05 < (walk[sl] != 0).mean() < 0.999 and (accept[sl] == 0).mean() > 0.01, (name, (walk[sl] != 0).mean(), (accept[sl] == 0).mean())  # both answers occur
        if name == "contains the eye":
            assert (walk[sl] != 0).mean() > 0.99 and accept[sl].all()
    # axis-parallel views put exact zeros into directions: the centre row / column of odd image sizes
    assert np.any(rays[:, 3:6] == 0.0)


def test_the_beam_accepts_what_the_walk_accepts(cases):
    cam, pix, jit, lo, hi, cls, names, accept, bound, walk, rays = cases
    bad = np.nonzero((walk != 0) & (accept == 0))[0]
    assert len(bad) == 0, (len(bad), [(names[cls[i]], cam[i], pix[i], jit[i], lo[i], hi[i]) for i in bad[:3]])
    for k, name in enumerate(names):
        sl = cls == k
        off = sl & (walk == 0)
        print("    %-34s %8d cases, walk accepts %5.1f %%, beam accepts %5.1f %%; of the %d the walk turns down for this sample the beam keeps %.2f %%"
              % (name, int(sl.sum()), 100.0 * (walk[sl] != 0).mean(), 100.0 * accept[sl].mean(), int(off.sum()), 100.0 * accept[off].mean() if off.any() else 0.0))


def test_the_stored_bound_lies_below_the_exact_entry_parameter(cases):
    cam, pix, jit, lo, hi, cls, names, accept, bound, walk, rays = cases
    o, d = rays[:, 0:3], rays[:, 3:6]
    tn_lo, tn_hi, meets = entry_parameter(o, d, lo, hi)
    acc = accept != 0
    assert np.all(bound[acc] >= 0.0) and np.all(np.isfinite(bound[acc]))
    bad = np.nonzero(acc & (bound.astype(LD) > tn_lo))[0]
    assert len(bad) == 0, (len(bad), [(names[cls[i]], float(bound[i]), float(tn_lo[i]), cam[i], pix[i], jit[i], lo[i], hi[i]) for i in bad[:3]])
    # the bound is worth something: for boxes the ray meets well in front of the eye it is within a few per cent of the entry parameter for most
    far = acc & meets & (cls == 0) & (tn_lo > 0)
    ratio = bound[far].astype(np.float64) / tn_lo[far].astype(np.float64)
    print("    bound / entry parameter over %d met boxes: median %.4f, 10th percentile %.4f" % (int(far.sum()), np.median(ratio), np.percentile(ratio, 10)))
    rng = np.random.default_rng(7)
    for k, name in enumerate(names):  # the long double bound itself, against rationals
        idx = np.nonzero(acc & (cls == k))[0]
        for i in rng.choice(idx, 800, replace=False):
            tn = exact_entry(o[i], d[i], lo[i], hi[i])
            assert Fraction(float(bound[i])) <= tn, (name, i)
