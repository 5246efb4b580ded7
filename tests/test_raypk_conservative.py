"""The tree walks' f32 slab test may only err towards visiting more boxes (pt_walk_lane.h: pt_raypk_axis, pt_slab_seg_pk; pt_walk_wave.h: pt_slab_pk2).
Through the host build of that code (pt_test_raypk: no GPU) 2.3 million ray / box pairs with a fixed seed: whenever the exact f64 ray
meets the f32 box within [0, t_max], every form of the test must accept the box.

"Exact" is decided in 80-bit long double with an explicit error bound. A plane's parameter T = (P - o) / d takes two roundings of
2^-64 relative each (P, o and d are exact inputs), so the computed T is within |T| 2^-62 of the true one with room to spare; a pair counts
as MEETING the box unless the intervals stay apart after widening every bound by that much - the doubtful pairs are on the side that
the code under test has to accept - and as MISSING it only if they stay apart. A sample of every class, the constructed grazing rays
among them, is decided again in rational arithmetic (fractions) to pin the long double classification itself.

What runs here is the HOST build: its reciprocal is a correctly rounded division (half an ulp). The device's v_rcp_f32, one ulp, is covered by the derivation
above pt_raypk_axis (which budgets 2u for it), not by these pairs.

The share of boxes accepted although the ray certainly misses them is printed for the f64-product body and the f32 body (profiles/r07/notes.md
records both); it is no pass criterion."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

LD = np.longdouble
EPS = LD(2.0) ** -62


def boxes_outward(lo64, hi64):
    """f64 bounds -> the f32 box pt_scene_upload stores: rounded outward, |coordinates| <= 1e18."""
    lo = lo64.astype(np.float32)
    hi = hi64.astype(np.float32)
    lo = np.where(lo.astype(np.float64) > lo64, np.nextafter(lo, np.float32(-np.inf)), lo)
    hi = np.where(hi.astype(np.float64) < hi64, np.nextafter(hi, np.float32(np.inf)), hi)
    return np.clip(lo, np.float32(-1e18), np.float32(1e18)), np.clip(hi, np.float32(-1e18), np.float32(1e18))


def log_uniform(rng, lo, hi, shape):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), shape))


def random_rays(rng, n):
    o = log_uniform(rng, 1e-3, 1e6, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= log_uniform(rng, 1e-3, 1e3, (n, 1))  # local rays of scaled instances are not unit vectors
    return o, d


def boxes_near_ray(rng, o, d):
    """Boxes around a point of the ray (in front of the origin, sometimes behind it), sized from much smaller to much larger than the distance: hits, near misses and misses."""
    n = len(o)
    t = log_uniform(rng, 1e-4, 1e5, (n, 1)) * rng.choice([1.0, 1.0, 1.0, -1.0], (n, 1))
    c = o + t * d
    reach = np.abs(t) * np.linalg.norm(d, axis=1, keepdims=True)
    half = reach * log_uniform(rng, 1e-7, 3.0, (n, 3))
    off = half * rng.uniform(-1.6, 1.6, (n, 3)) * rng.choice([0.0, 1.0], (n, 1), p=[0.3, 0.7])
    return boxes_outward(c + off - half, c + off + half)


def build_cases():
    rng = np.random.default_rng(20260707)
    O, D, TM, LO, HI, CLS = [], [], [], [], [], []

    def add(name, o, d, lo, hi, tm=None):
        n = len(o)
        if tm is None:
            tm = np.where(rng.random(n) < 0.5, np.inf, log_uniform(rng, 1e-4, 1e6, n))
        O.append(o); D.append(d); TM.append(tm); LO.append(lo); HI.append(hi); CLS.append((name, n))

    # 1. rays and boxes at random
    o, d = random_rays(rng, 900_000)
    add("random", o, d, *boxes_near_ray(rng, o, d))
    # boxes anywhere, up to the limit of +-1e18
    o, d = random_rays(rng, 100_000)
    c = log_uniform(rng, 1e-3, 1e18, (100_000, 3)) * rng.choice([-1.0, 1.0], (100_000, 3))
    h = np.abs(c) * log_uniform(rng, 1e-3, 4.0, (100_000, 3))
    add("far boxes", o, d, *boxes_outward(c - h, c + h))
    # the range ends near where the ray enters the box: t_max just below, at and just above that parameter
    o, d = random_rays(rng, 200_000)
    lo, hi = boxes_near_ray(rng, o, d)
    with np.errstate(all="ignore"):
        t0 = np.where(d > 0, (lo - o) / d, (hi - o) / d).max(axis=1)
    tm = np.abs(t0) * (1.0 + rng.choice([-1e-6, -3e-8, -2e-16, 0.0, 2e-16, 3e-8, 1e-6], 200_000))
    add("range ends at the box", o, d, lo, hi, tm)

    # 2. axis-parallel, denormal and zero components
    o, d = random_rays(rng, 300_000)
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 1e-40, -1e-40, 1e-45, 1.1e-38, -1.3e-38, 1e-19, -1e-19, 0.9e-18, -1.1e-18, 1e-18, 2e-18])
    k = rng.integers(0, 3, 300_000)
    d[np.arange(300_000), k] = rng.choice(special, 300_000)
    two = rng.random(300_000) < 0.4
    k2 = (k + 1 + rng.integers(0, 2, 300_000)) % 3
    d[np.arange(300_000)[two], k2[two]] = rng.choice(special, int(two.sum()))
    lo, hi = boxes_near_ray(rng, o, d)
    # half of them: the origin's coordinate on the special axis inside / on the edge of the box's slab, so the other axes decide
    inside = rng.random(300_000) < 0.5
    idx = np.arange(300_000)[inside]
    ok = o[idx, k[idx]]
    lo[idx, k[idx]] = np.nextafter(ok.astype(np.float32), np.float32(-np.inf)) - (np.abs(ok) * rng.choice([0.0, 1e-3], len(idx))).astype(np.float32)
    hi[idx, k[idx]] = np.nextafter(ok.astype(np.float32), np.float32(np.inf)) + (np.abs(ok) * rng.choice([0.0, 1e-3], len(idx))).astype(np.float32)
    add("parallel / denormal", o, d, lo, hi)

    # 3. one face of the box through the origin (the origin's coordinate there is an f32, so the plane's parameter is exactly 0)
    o, d = random_rays(rng, 300_000)
    k = rng.integers(0, 3, 300_000)
    o[np.arange(300_000), k] = o[np.arange(300_000), k].astype(np.float32).astype(np.float64)
    lo, hi = boxes_near_ray(rng, o, d)
    r = np.arange(300_000)
    ext = (np.abs(o[r, k]) * log_uniform(rng, 1e-6, 10.0, 300_000)).astype(np.float32)
    lower = rng.random(300_000) < 0.5
    ok32 = o[r, k].astype(np.float32)
    lo[r, k] = np.where(lower, ok32, ok32 - ext)
    hi[r, k] = np.where(lower, ok32 + ext, ok32)
    # the other two axes: around the origin for half of them, so the touching face is what the answer hangs on
    around = rng.random(300_000) < 0.5
    for j in (1, 2):
        kk = (k + j) % 3
        e = (np.abs(o[r, kk]) * log_uniform(rng, 1e-6, 10.0, 300_000))
        l2, h2 = boxes_outward(o[r, kk] - e, o[r, kk] + e)
        lo[r, kk] = np.where(around, l2, lo[r, kk])
        hi[r, kk] = np.where(around, h2, hi[r, kk])
    add("face through the origin", o, d, lo, hi)

    # 4. rays that graze an edge or a corner, CONSTRUCTED: the box's corner C (f32 coordinates), a direction of small dyadic components and an origin
    # o = C - s d with an integer s - every step exact in f64, so the exact ray passes through C at t = s and touches the box there. Directions that leave
    # the box at once (the signs point away from it on the grazed axes) make the touch the only contact.
    n = 500_000
    lo64 = log_uniform(rng, 1e-2, 1e4, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    lo = lo64.astype(np.float32)
    hi = (lo.astype(np.float64) + log_uniform(rng, 1e-3, 1e3, (n, 3))).astype(np.float32)
    hi = np.maximum(hi, np.nextafter(lo, np.float32(np.inf)))
    corner_hi = rng.integers(0, 2, (n, 3)).astype(bool)
    cpt = np.where(corner_hi, hi, lo).astype(np.float64)
    edge = rng.random(n) < 0.5  # an edge: the point lies strictly inside the box's extent on one axis, at an f32 between the planes
    ek = rng.integers(0, 3, n)
    mid = ((lo.astype(np.float64) + hi.astype(np.float64)) * 0.5).astype(np.float32).astype(np.float64)
    r = np.arange(n)
    cpt[r[edge], ek[edge]] = mid[r[edge], ek[edge]]
    scale = 2.0 ** rng.integers(-6, 7, (n, 1))
    d = rng.integers(1, 33, (n, 3)).astype(np.float64) / 32.0 * scale
    away = rng.random((n, 3)) < 0.5  # on this axis the ray is on its way OUT of the slab when it reaches C (else on its way in)
    d = np.where(corner_hi ^ away, -d, d)
    par = rng.random(n) < 0.2  # some run along the edge / in the face: a zero component
    d[r[par], ek[par]] = 0.0
    s = rng.integers(1, 200, (n, 1)).astype(np.float64)
    o = cpt - s * d
    exact = np.all((o + s * d == cpt) & (np.abs(s * d) < 2.0 ** 20) & (np.abs(cpt) > 2.0 ** -20), axis=1)  # (53 bits hold every such sum: kept only where that is so)
    o, d, lo, hi, s = o[exact], d[exact], lo[exact], hi[exact], s[exact]
    tm = np.where(rng.random(len(o)) < 0.3, s[:, 0], np.where(rng.random(len(o)) < 0.5, np.inf, s[:, 0] * 2.0))  # the touch at the very end of the range, or inside it
    add("grazing", o, d, lo, hi, tm)
    return (np.concatenate(O), np.concatenate(D), np.concatenate(TM), np.concatenate(LO).astype(np.float32), np.concatenate(HI).astype(np.float32), CLS)


def classify(o, d, tm, lo, hi):
    """(meets, doubtful) in long double with the error bound of the module's docstring: the pairs that certainly or possibly meet, and the merely possible ones among them."""
    assert np.finfo(LD).nmant >= 63, "the error bound below is that of the 80-bit long double"
    n = len(o)
    tn_lo = np.zeros(n, LD)            # lower bound of the exact entering parameter max(T_enter.., 0)
    tf_hi = tm.astype(LD)              # upper bound of the exact leaving parameter min(T_leave.., t_max)
    tn_hi = np.zeros(n, LD)
    tf_lo = tm.astype(LD)
    empty = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for k in range(3):
            ok, dk = o[:, k].astype(LD), d[:, k].astype(LD)
            l, h = lo[:, k].astype(LD), hi[:, k].astype(LD)
            zero = d[:, k] == 0.0
            empty |= zero & ((o[:, k] < lo[:, k].astype(np.float64)) | (o[:, k] > hi[:, k].astype(np.float64)))  # (f32 -> f64 is exact: an exact comparison)
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
    doubtful = meets & (tn_hi > tf_lo)
    return meets, doubtful


def exact_meets(o, d, tm, lo, hi):
    """One pair in rational arithmetic: does {o + t d, 0 <= t <= tm} touch the box?"""
    tn, tf = Fraction(0), (None if np.isinf(tm) else Fraction(float(tm)))
    for k in range(3):
        ok, dk, l, h = Fraction(float(o[k])), Fraction(float(d[k])), Fraction(float(lo[k])), Fraction(float(hi[k]))
        if dk == 0:
            if ok < l or ok > h:
                return False
            continue
        a, b = (l - ok) / dk, (h - ok) / dk
        e, f = min(a, b), max(a, b)
        tn = max(tn, e)
        tf = f if tf is None else min(tf, f)
    return tf is None or tn <= tf


@pytest.fixture(scope="module")
def cases():
    o, d, tm, lo, hi, cls = build_cases()
    meets, doubtful = classify(o, d, tm, lo, hi)
    return o, d, tm, lo, hi, cls, meets, ~meets, doubtful


def run(body, o, d, tm, lo, hi):
    from portrayer_amd import _hip as H
    n = len(o)
    o, d, tm, lo, hi = (np.ascontiguousarray(x) for x in (o, d, tm, lo, hi))
    verdict = np.zeros(n, np.int32)
    tn = np.zeros(n, np.float32)
    tf = np.zeros(n, np.float32)
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    rc = H.lib().pt_test_raypk(n, body, o.ctypes.data_as(dp), d.ctypes.data_as(dp), tm.ctypes.data_as(dp), lo.ctypes.data_as(fp), hi.ctypes.data_as(fp),
                               verdict.ctypes.data_as(C.POINTER(C.c_int32)), tn.ctypes.data_as(fp), tf.ctypes.data_as(fp))
    assert rc == 0
    return verdict, tn, tf


def test_case_set_is_what_the_module_promises(cases):
    o, d, tm, lo, hi, cls, meets, misses, doubtful = cases
    assert len(o) >= 2_000_000 and np.all(lo <= hi) and np.abs(lo).max() <= 1e18 and np.abs(hi).max() <= 1e18
    assert {name for name, _ in cls} == {"random", "far boxes", "range ends at the box", "parallel / denormal", "face through the origin", "grazing"}
    at = 0
    for name, n in cls:
        sl = slice(at, at + n)
        at += n
        assert n >= 50_000, name
        if name not in ("far boxes", "grazing"):
            assert 0.05 < meets[sl].mean() and misses[sl].mean() > 0.05, (name, meets[sl].mean(), misses[sl].mean())  # both answers are well represented
        if name == "grazing":
            assert meets[sl].all()  # constructed to touch


def test_long_double_classification_against_rationals(cases):
    o, d, tm, lo, hi, cls, meets, misses, doubtful = cases
    rng = np.random.default_rng(5)
    at = 0
    for name, n in cls:
        for i in at + rng.choice(n, 1500, replace=False):
            truth = exact_meets(o[i], d[i], tm[i], lo[i], hi[i])
            assert meets[i] if truth else (misses[i] or doubtful[i]), (name, i)
            if name == "grazing":
                assert truth
        at += n
    at = 0
    for name, n in cls:  # the doubtful band is thin - the classification decides nearly every pair - except where the touch was constructed
        assert name == "grazing" or doubtful[at:at + n].mean() < 1e-3, (name, doubtful[at:at + n].mean())
        at += n


@pytest.mark.parametrize("body", [0, 1, 2], ids=["as built", "f64 products", "f32 products"])
def test_no_box_the_ray_meets_is_rejected(cases, body):
    o, d, tm, lo, hi, cls, meets, misses, doubtful = cases
    verdict, tn, tf = run(body, o, d, tm, lo, hi)
    assert not np.any(verdict & 8), "the two children of a wavefront form disagree on the same box"
    assert np.array_equal((verdict & 1) != 0, ~(tn > tf))  # the interval reported is the one the verdict came from
    at = 0
    for name, n in cls:
        sl = slice(at, at + n)
        at += n
        for bit, form in ((1, "per lane"), (2, "wavefront, mixed signs"), (4, "wavefront, own octant")):
            bad = np.nonzero(meets[sl] & ((verdict[sl] & bit) == 0))[0]
            assert len(bad) == 0, (name, form, len(bad), [(o[at - n + i], d[at - n + i], tm[at - n + i], lo[at - n + i], hi[at - n + i]) for i in bad[:3]])
    # the octant form and the mixed form see the same constants: the same verdict
    assert np.array_equal((verdict & 2) != 0, (verdict & 4) != 0)
    false_accepts = np.mean((verdict[misses] & 1) != 0)
    print("body %d: %.4f %% of the %d boxes the ray certainly misses are accepted" % (body, 100.0 * false_accepts, int(misses.sum())))
    at = 0
    for name, n in cls:
        sl = slice(at, at + n)
        at += n
        m = misses[sl]
        print("    %-26s %8d pairs, %5.1f %% meet, false accepts %.4f %%" % (name, n, 100.0 * meets[sl].mean(), 100.0 * np.mean((verdict[sl][m] & 1) != 0) if m.any() else 0.0))
