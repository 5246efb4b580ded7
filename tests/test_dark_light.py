"""A light the launch calls dark must be dark for the reference (pt_certain.h 4.-8.: pt_dark_light, pt_dark_lane).
Through the host build of that code (pt_test_dark_light: no GPU) two million fixed-seed cases for each of the four analytic solids: a node's two matrices, a
light position L and a shaded point P. Whenever the table routine flags the light as enclosed in the node AND the lane guard lets P through, the reference's own
f64 test of that node - pt_unit_prim_hit on pt_ray_to_local(inv, {P, normalize(L - P)}) over [EPSILON, INF) - must report a hit. There is no tolerance: one case
with `flagged` and `guard` set and `exact_hit` clear fails the test.

The cases: scales from 1e-6 to 1e6, rotations, non-uniform scale and shear, one axis stretched by 1e3 .. 1e5 (conditioning beyond 2^10: no ball); lights from the
node's centre to outside the primitive, and - where the ball's radius is known here, a rotation times a uniform scale - within 1e-9 .. 1e-2 of the margin
(1 - 2^-6) rho from both sides; origins outside the solid, inside it, on its surface, within 1e-18 .. 1e-12 of L, equal to L, and anywhere out to |P| = 1e6.

Cylinder and cone have no ball (pt_certain.h 3.), so a light inside one is never flagged; area lights are never flagged (8.): both are checked.

Not vacuous: the SURE cases are built so that the derived margins alone guarantee the flag and the guard - a sphere or cube under a rotation times a uniform
scale s in [1, 1e3], its centre at |c| <= 1e3, the light at most three quarters of rho = r (1 - 2^-5) - 2^-10 - 2^-20 |c| from the centre (the table's radius is
that up to 2^-19, and it flags up to (1 - 2^-6) of it), and 1e-3 <= |L - P| <= 1e3. The guard's ceiling is |L - P| < 2^12 rho (1 - 2^-10) - 2^-21 |L| (pt_certain.h
5.), which for the smallest such ball (the cube at s = 1: rho > 0.48) is 1,960: the range up to 1e4 would exceed it, so the construction stops at 1e3; the floor is
1e-15. ALL of them must be flagged and pass the guard."""
import ctypes as C

import numpy as np
import pytest

from test_certain_shadow import (CONE, CONE_R, CUBE, CYLINDER, NAMES, SPHERE, interior_points, log_uniform, records, rotations, surface_points,
                                 unit_vectors)

N_XFORMS = 250_000
RAYS_PER_XFORM = 8
RM = {SPHERE: 1.0, CUBE: 0.5, CYLINDER: 0.5, CONE: CONE_R}


def transforms(rng, n):
    """kind 0: SURE nodes (rotation x uniform scale in [1, 1e3], |c| <= 1e3); 1: rotation x uniform scale 1e-6 .. 1e6; 2: x non-uniform scale; 3: with shear;
    4: one axis stretched by 1e3 .. 1e5. Centres from next to the origin to 1e6 away, half of them within 100 scales."""
    kind = rng.integers(0, 5, n)
    scale = log_uniform(rng, 1e-6, 1e6, (n, 1))
    sure = kind == 0
    scale[sure] = log_uniform(rng, 1.0, 1e3, (int(sure.sum()), 1))
    s3 = np.repeat(scale, 3, axis=1)
    nonuni = kind >= 2
    s3[nonuni] *= log_uniform(rng, 1.0 / 30.0, 30.0, (int(nonuni.sum()), 3))
    stretched = kind == 4
    s3[stretched, 0] *= log_uniform(rng, 1e3, 1e5, int(stretched.sum()))
    A = rotations(rng, n) * s3[:, None, :]
    shear = np.tile(np.eye(3), (n, 1, 1))
    sheared = kind == 3
    k = int(sheared.sum())
    shear[sheared, 0, 1] = rng.uniform(-2.0, 2.0, k)
    shear[sheared, 0, 2] = rng.uniform(-2.0, 2.0, k)
    shear[sheared, 1, 2] = rng.uniform(-2.0, 2.0, k)
    A = A @ shear
    far = log_uniform(rng, 1e-3, 1e6, (n, 1))
    near = scale * log_uniform(rng, 1e-3, 1e2, (n, 1))
    dist = np.where(rng.integers(0, 2, (n, 1)) == 0, far, near)
    dist[sure] = log_uniform(rng, 1e-3, 1e3, (int(sure.sum()), 1))
    t = unit_vectors(rng, n) * dist
    return A, t, scale, kind


def build_cases(typ, seed):
    rng = np.random.default_rng(seed)
    A, t, scale, kind = transforms(rng, N_XFORMS)
    fwd, inv = records(A, t)
    A, t, scale, kind, fwd, inv = (np.repeat(x, RAYS_PER_XFORM, axis=0) for x in (A, t, scale, kind, fwd, inv))
    n = len(A)
    rm = RM[typ]
    cm = np.array([0.0, CONE_R - 0.5 if typ == CONE else 0.0, 0.0])
    to_world = lambda pm: (A @ pm[:, :, None])[:, :, 0] + t
    c = to_world(np.broadcast_to(cm, (n, 3)))
    r = rm * scale[:, 0]
    rho = r * (1.0 - 2.0 ** -5) - 2.0 ** -10 - 2.0 ** -20 * np.linalg.norm(c, axis=1)  # the table's radius where A is a rotation times a uniform scale
    uniform = (kind <= 1) & (rho >= 0.5 * r)

    # ---- the light: in model space from the centre to outside the primitive; where rho is known, in world space relative to it
    L = to_world(cm + unit_vectors(rng, n) * (rm * rng.uniform(0.0, 1.3, (n, 1))))
    lcat = rng.integers(0, 4, n)
    frac = np.where(lcat == 0, rng.uniform(0.0, 0.75, n),                                                      # deep inside
                    np.where(lcat == 1, (1.0 - 2.0 ** -6) * (1.0 - log_uniform(rng, 1e-9, 1e-2, n)),          # a hair inside the margin
                             np.where(lcat == 2, (1.0 - 2.0 ** -6) * (1.0 + log_uniform(rng, 1e-9, 1e-2, n)),  # a hair outside it
                                      rng.uniform(0.9, 1.3, n))))                                              # around the ball's surface and outside
    Lw = c + unit_vectors(rng, n) * (rho * frac)[:, None]
    L[uniform] = Lw[uniform]
    deep = uniform & (lcat == 0)

    # ---- the origin
    pcat = rng.integers(0, 8, n)
    outside = to_world(unit_vectors(rng, n) * log_uniform(rng, 1.01, 1e4, (n, 1)))
    P = outside.copy()                                                           # 0, 1: outside the solid
    m = pcat == 2
    P[m] = to_world(interior_points(rng, typ, n))[m]                             # 2: inside it
    m = pcat == 3
    P[m] = to_world(surface_points(rng, typ, n))[m]                              # 3: on its surface
    m = pcat == 4                                                                # 4: within 1e-18 .. 1e-12 (relative to |L| where that is larger) of L
    P[m] = (L + unit_vectors(rng, n) * (log_uniform(rng, 1e-18, 1e-12, (n, 1)) * np.maximum(1.0, np.linalg.norm(L, axis=1, keepdims=True))))[m]
    m = pcat == 5
    P[m] = L[m]                                                                  # 5: equal to L
    m = pcat == 6
    P[m] = (unit_vectors(rng, n) * log_uniform(rng, 1e-3, 1e6, (n, 1)))[m]      # 6: anywhere out to |P| = 1e6
    m = pcat == 7                                                                # 7: a chosen distance from L, 1e-3 .. 1e3 (the SURE cases' range)
    P[m] = (L + unit_vectors(rng, n) * log_uniform(rng, 1e-3, 1e3, (n, 1)))[m]

    P = np.ascontiguousarray(P)
    L = np.ascontiguousarray(L)
    dist = np.linalg.norm(L - P, axis=1)
    sure = deep & (kind == 0) & (dist >= 1e-3) & (dist <= 1e3)
    return fwd, inv, P, L, sure


def run(typ, fwd, inv, P, L, area=None):
    from portrayer_amd import _hip as H
    n = len(P)
    out = [np.zeros(n, dtype=np.int32) for _ in range(3)]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = H.lib().pt_test_dark_light(n, typ, fwd.ctypes.data_as(dp), inv.ctypes.data_as(dp), P.ctypes.data_as(dp), L.ctypes.data_as(dp),
                                    area.ctypes.data_as(dp) if area is not None else None, *(o.ctypes.data_as(ip) for o in out))
    assert rc == 0
    return out


@pytest.mark.parametrize("typ", [SPHERE, CUBE, CYLINDER, CONE], ids=lambda t: NAMES[t])
def test_a_dark_light_is_dark_for_the_reference(typ):
    fwd, inv, P, L, sure = build_cases(typ, 20261021 + typ)
    n = len(P)
    assert n == 2_000_000
    flagged, guard, exact = run(typ, fwd, inv, P, L)
    skipped = (flagged != 0) & (guard != 0)
    print(f"dark-light {NAMES[typ]}: {n} cases, {int(exact.sum())} exact hits, {int(flagged.sum())} flagged, {int(skipped.sum())} flagged and through the guard, "
          f"{int(sure.sum())} sure by construction")
    assert int(exact.sum()) > n // 10, "the cases no longer exercise the test"
    assert not np.any((guard != 0) & (flagged == 0))
    if typ in (SPHERE, CUBE):
        assert int(sure.sum()) > n // 100, "the cases no longer exercise the test"
        assert np.all(flagged[sure] != 0), "a light deep inside a well-conditioned node's ball is not flagged"
        assert np.all(guard[sure] != 0), "the guard turns down an origin the derived bounds let through"
        assert int(skipped.sum()) > int(sure.sum()), "nothing beyond the sure cases is flagged"
        assert int(((flagged != 0) & (guard == 0)).sum()) > n // 100, "the guard's bounds are never reached"
        assert int((flagged == 0).sum()) > n // 10, "every light is flagged"
    else:
        assert int(flagged.sum()) == 0, "this type has no ball"
    bad = np.flatnonzero(skipped & (exact == 0))
    assert bad.size == 0, f"{bad.size} cases skipped without an exact hit, first: fwd={fwd[bad[0]]} inv={inv[bad[0]]} P={P[bad[0]]} L={L[bad[0]]}"


def test_the_origin_equal_to_the_light_takes_the_exact_path():
    """P == L, and P within a few ulps of L: the reference's direction is NaN (or decided by rounding), so the guard must turn the lane down."""
    fwd = np.array([[4.0, 0, 0, 10.0, 0, 4.0, 0, 20.0, 0, 0, 4.0, 30.0]])
    inv = np.array([[0.25, 0, 0, -2.5, 0, 0.25, 0, -5.0, 0, 0, 0.25, -7.5]])
    L = np.array([[10.5, 20.25, 29.5]])
    for typ in (SPHERE, CUBE):
        for P in (L.copy(), np.nextafter(L, np.inf), L + 1e-16, L + 1e-9):
            flagged, guard, _ = run(typ, fwd, inv, np.ascontiguousarray(P), L)
            assert (int(flagged[0]), int(guard[0])) == (1, 0)
        flagged, guard, exact = run(typ, fwd, inv, L + np.array([[0.0, 1e-3, 0.0]]), L)
        assert (int(flagged[0]), int(guard[0]), int(exact[0])) == (1, 1, 1)


def test_area_lights_cylinders_cones_and_flat_types_are_never_flagged():
    rng = np.random.default_rng(7)
    n = 20_000
    s = log_uniform(rng, 1.0, 100.0, (n, 1))
    A = rotations(rng, n) * np.repeat(s, 3, axis=1)[:, None, :]
    t = unit_vectors(rng, n) * log_uniform(rng, 1e-3, 1e3, (n, 1))
    fwd, inv = records(A, t)
    L = np.ascontiguousarray(t + unit_vectors(rng, n) * (0.2 * s * rng.uniform(0.0, 1.0, (n, 1))))  # well inside every solid's ball (the cube's: 0.48 s)
    P = np.ascontiguousarray(L + unit_vectors(rng, n) * log_uniform(rng, 1e-2, 1e2, (n, 1)))
    for typ in (SPHERE, CUBE):
        flagged, guard, exact = run(typ, fwd, inv, P, L)
        assert np.all(flagged != 0) and np.all(guard != 0) and np.all(exact != 0)
        # an area light - both vectors non-zero, however small - draws its position per sample: never flagged
        area = np.ascontiguousarray(unit_vectors(rng, 2 * n).reshape(n, 6) * log_uniform(rng, 1e-300, 1.0, (n, 1)))
        flagged, guard, _ = run(typ, fwd, inv, P, L, area)
        assert not flagged.any() and not guard.any()
        # one vector zero: the kernel's criterion makes it a point light
        area[:, 3:] = 0.0
        flagged, guard, _ = run(typ, fwd, inv, P, L, area)
        assert np.all(flagged != 0) and np.all(guard != 0)
    for typ in (1, 2, 3, 4, CYLINDER, CONE):
        flagged, guard, _ = run(typ, fwd, inv, P, L)
        assert not flagged.any() and not guard.any()
    # NaN and infinite lights, a node without a ball (zero scale): never flagged
    for bad in (np.nan, np.inf, -np.inf, 1e300):
        Lb = L.copy(); Lb[:, 1] = bad
        assert not run(SPHERE, fwd, inv, P, np.ascontiguousarray(Lb))[0].any()
    zero = np.zeros_like(fwd)
    assert not run(SPHERE, zero, zero, P, L)[0].any()
