"""The shadow rays' certain-occlusion test may only err towards "not certain" (pt_certain.h: pt_certain_ball, pt_certain_lane).
Through the host build of that code (pt_test_certain_shadow: no GPU) two million fixed-seed cases for each of the four analytic solids: a node's two
matrices, a shaded point P and a light position L. Whenever the f32 test says the shadow ray certainly ends in the node, the reference's own f64 test of
that node - pt_unit_prim_hit on pt_ray_to_local(inv, {P, normalize(L - P)}) over [EPSILON, INF) - must report a hit. There is no tolerance: one case with
`certain` set and `exact_hit` clear fails the test.

The cases: rays grazing the certain ball from both sides (offsets from 1e-7 to 1e-2 of its radius); origins on the primitive's surface, the light
in front of it or behind it; origins inside; the light inside the primitive and the light behind it; |P| from 1e-3 to 1e6; scales from 1e-6 to 1e6;
non-uniform scale and shear; for the cone rays steeper than its side, aimed at the apex with offsets from 1e-9 of the primitive and down through the mirror
nappe, for the cylinder and the cone rays aimed at a rim with offsets from 1e-9.

Sphere and cube have a ball. Cylinder and cone have none (pt_certain.h, 3.: at a rim and at the apex the reference's own tests may turn down a crossing the
exact ray makes, and no ball can know): for them the test also checks that no case is certain - the cone's apex cases hold rays, some hundreds, that pass
through the solid and that the reference reports as misses.

What runs here is the HOST build: it divides where the device multiplies by v_rcp_f32 (one ulp). The quotient only chooses WHICH point of the ray is
measured against the ball, so its rounding enters no bound (pt_certain.h, 1.).

The share of exact hits that the test calls certain is printed per type; it is no pass criterion."""
import ctypes as C

import numpy as np
import pytest

SPHERE, CUBE, CYLINDER, CONE = 0, 5, 6, 7
NAMES = {SPHERE: "sphere", CUBE: "cube", CYLINDER: "cylinder", CONE: "cone"}
N_XFORMS = 250_000
RAYS_PER_XFORM = 8
CONE_R = 0.5 / (0.5 + np.sqrt(1.25))


def log_uniform(rng, lo, hi, shape):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), shape))


def unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)


def transforms(rng, n):
    """Forward 3x3 blocks A and translations t: rotation x uniform scale (half), x non-uniform scale (a quarter), with shear (a quarter);
    scales 1e-6 .. 1e6; centres from next to the origin to 1e6 away, half of them within 100 scales (where the node can have a ball at all)."""
    scale = log_uniform(rng, 1e-6, 1e6, (n, 1))
    kind = rng.integers(0, 4, n)
    s3 = np.repeat(scale, 3, axis=1)
    nonuni = kind >= 2
    s3[nonuni] *= log_uniform(rng, 1.0 / 30.0, 30.0, (int(nonuni.sum()), 3))
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
    t = unit_vectors(rng, n) * np.where(rng.integers(0, 2, (n, 1)) == 0, far, near)
    return A, t, scale


def records(A, t):
    n = len(A)
    fwd = np.concatenate([A, t[:, :, None]], axis=2).reshape(n, 12)
    Ai = np.linalg.inv(A)
    ti = -(Ai @ t[:, :, None])
    inv = np.concatenate([Ai, ti], axis=2).reshape(n, 12)
    return np.ascontiguousarray(fwd), np.ascontiguousarray(inv)


def disc(rng, n, radius):
    th = rng.uniform(0.0, 2.0 * np.pi, n)
    r = radius * np.sqrt(rng.uniform(0.0, 1.0, n))
    return r * np.cos(th), r * np.sin(th)


def surface_points(rng, typ, n):
    if typ == SPHERE:
        return unit_vectors(rng, n)
    if typ == CUBE:
        p = rng.uniform(-0.5, 0.5, (n, 3))
        ax = rng.integers(0, 3, n)
        p[np.arange(n), ax] = rng.choice([-0.5, 0.5], n)
        return p
    th = rng.uniform(0.0, 2.0 * np.pi, n)
    y = rng.uniform(-0.5, 0.5, n)
    rad = np.full(n, 0.5) if typ == CYLINDER else (0.5 - y) / 2.0
    side = np.stack([rad * np.cos(th), y, rad * np.sin(th)], axis=1)
    cx, cz = disc(rng, n, 0.5)
    cap_y = rng.choice([-0.5, 0.5], n) if typ == CYLINDER else np.full(n, -0.5)
    cap = np.stack([cx, cap_y, cz], axis=1)
    return np.where(rng.integers(0, 3, (n, 1)) == 0, cap, side)


def interior_points(rng, typ, n):
    if typ == SPHERE:
        return unit_vectors(rng, n) * rng.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0)
    if typ == CUBE:
        return rng.uniform(-0.5, 0.5, (n, 3))
    y = rng.uniform(-0.5, 0.5, n)
    x, z = disc(rng, n, 1.0)
    rad = 0.5 if typ == CYLINDER else (0.5 - y) / 2.0
    return np.stack([x * rad, y, z * rad], axis=1)


def model_cases(rng, typ, n):
    """(P, L) in model space, by category."""
    rm = {SPHERE: 1.0, CUBE: 0.5, CYLINDER: 0.5, CONE: CONE_R}[typ]
    cm = np.array([0.0, CONE_R - 0.5 if typ == CONE else 0.0, 0.0])
    cat = rng.integers(0, 8, n)
    P = np.empty((n, 3))
    L = np.empty((n, 3))
    near_ball = cm + rm * rng.uniform(-1.5, 1.5, (n, 3))
    outside = unit_vectors(rng, n) * log_uniform(rng, 1.01, 1e4, (n, 1))
    surf = surface_points(rng, typ, n)
    inner = interior_points(rng, typ, n)
    anyway = unit_vectors(rng, n) * log_uniform(rng, 1e-2, 1e2, (n, 1))
    # 0, 1: origin on the surface, the light anywhere (front-facing and back-facing alike)
    m = cat <= 1
    P[m] = surf[m]; L[m] = surf[m] + anyway[m]
    # 2: origin on the surface, the ray through the region of the ball, the light in front of the ball, inside it or far behind
    m = cat == 2
    P[m] = surf[m]; L[m] = surf[m] + (near_ball[m] - surf[m]) * log_uniform(rng, 0.3, 100.0, (int(m.sum()), 1))
    # 3: origin inside the primitive
    m = cat == 3
    P[m] = inner[m]; L[m] = inner[m] + anyway[m]
    # 4: origin outside, the light inside the primitive
    m = cat == 4
    P[m] = outside[m]; L[m] = inner[m]
    # 5, 6: origin outside, the light behind the primitive
    m = (cat == 5) | (cat == 6)
    P[m] = outside[m]; L[m] = outside[m] + (near_ball[m] - outside[m]) * log_uniform(rng, 1.0, 1e3, (int(m.sum()), 1))
    # 7: the type's own: the cone's apex region, steep rays, the mirror nappe; the cylinder's and the cone's rims
    m = cat == 7
    k = int(m.sum())
    jitter = unit_vectors(rng, k) * log_uniform(rng, 1e-9, 1e-1, (k, 1))
    if typ == CONE:
        sub = rng.integers(0, 4, k)
        apex = np.array([0.0, 0.5, 0.0])
        th = rng.uniform(0.0, 2.0 * np.pi, k)
        up = log_uniform(rng, 1e-3, 10.0, k)
        rad = up / 2.0 * rng.uniform(0.0, 1.0, k)
        mirror = apex + np.stack([rad * np.cos(th), up, rad * np.sin(th)], axis=1)  # inside the mirror nappe
        rim = np.stack([0.5 * np.cos(th), np.full(k, -0.5), 0.5 * np.sin(th)], axis=1)
        p = np.where(sub[:, None] == 0, mirror, np.where(sub[:, None] == 1, inner[m], outside[m]))
        target = np.where(sub[:, None] == 0, near_ball[m], np.where(sub[:, None] == 3, rim + jitter, apex + jitter))
        P[m] = p; L[m] = p + (target - p) * log_uniform(rng, 0.5, 100.0, (k, 1))
    elif typ == CYLINDER:
        th = rng.uniform(0.0, 2.0 * np.pi, k)
        rim = np.stack([0.5 * np.cos(th), rng.choice([-0.5, 0.5], k), 0.5 * np.sin(th)], axis=1)
        p = np.where(rng.integers(0, 2, (k, 1)) == 0, inner[m], outside[m])
        P[m] = p; L[m] = p + (rim + jitter - p) * log_uniform(rng, 0.5, 100.0, (k, 1))
    else:
        P[m] = outside[m]; L[m] = outside[m] + (near_ball[m] - outside[m]) * log_uniform(rng, 0.5, 100.0, (k, 1))
    return P, L


def build_cases(typ, seed):
    rng = np.random.default_rng(seed)
    A, t, scale = transforms(rng, N_XFORMS)
    fwd, inv = records(A, t)
    rep = RAYS_PER_XFORM
    A, t, scale, fwd, inv = (np.repeat(x, rep, axis=0) for x in (A, t, scale, fwd, inv))
    n = len(A)
    Pm, Lm = model_cases(rng, typ, n)
    P = (A @ Pm[:, :, None])[:, :, 0] + t
    L = (A @ Lm[:, :, None])[:, :, 0] + t
    # a quarter of the cases in world space instead: rays grazing the certain ball from both sides, where A is a rotation times a uniform scale (the ball's radius is
    # then known here: pt_certain_ball's formula); and origins anywhere from 1e-3 to 1e6, the light behind the node
    world = rng.integers(0, 4, n) == 0
    cm = np.array([0.0, CONE_R - 0.5 if typ == CONE else 0.0, 0.0])
    rm = {SPHERE: 1.0, CUBE: 0.5, CYLINDER: 0.5, CONE: CONE_R}[typ]
    c = (A @ np.broadcast_to(cm, (n, 3))[:, :, None])[:, :, 0] + t
    r = rm * scale[:, 0]
    rho = np.maximum(r * (1.0 - 2.0 ** -5) - 2.0 ** -10 - 2.0 ** -20 * np.linalg.norm(c, axis=1), 1e-3 * r)
    d = unit_vectors(rng, n)
    nrm = np.cross(d, unit_vectors(rng, n))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    off = 1.0 + rng.choice([-1.0, 1.0], n) * log_uniform(rng, 1e-7, 1e-2, n)
    foot = c + nrm * (rho * off)[:, None]
    graze = world & (rng.integers(0, 3, n) != 0)
    P[graze] = (foot - d * (r * log_uniform(rng, 1e-3, 1e3, n))[:, None])[graze]
    L[graze] = (foot + d * (r * log_uniform(rng, 1e-3, 1e3, n))[:, None])[graze]
    far = world & ~graze
    Pf = unit_vectors(rng, n) * log_uniform(rng, 1e-3, 1e6, (n, 1))
    P[far] = Pf[far]
    L[far] = (Pf + (c + r[:, None] * rng.uniform(-1.0, 1.0, (n, 3)) - Pf) * log_uniform(rng, 1.0, 100.0, (n, 1)))[far]
    return fwd, inv, np.ascontiguousarray(P), np.ascontiguousarray(L)


@pytest.mark.parametrize("typ", [SPHERE, CUBE, CYLINDER, CONE], ids=lambda t: NAMES[t])
def test_certain_implies_the_exact_hit(typ):
    from portrayer_amd import _hip as H
    fwd, inv, P, L = build_cases(typ, 20261019 + typ)
    n = len(P)
    assert n == 2_000_000
    certain = np.zeros(n, dtype=np.int32)
    exact = np.zeros(n, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = H.lib().pt_test_certain_shadow(n, typ, fwd.ctypes.data_as(dp), inv.ctypes.data_as(dp), P.ctypes.data_as(dp), L.ctypes.data_as(dp), certain.ctypes.data_as(ip), exact.ctypes.data_as(ip))
    assert rc == 0
    hits, cert = int(exact.sum()), int(certain.sum())
    print(f"certain-shadow {NAMES[typ]}: {n} cases, {hits} exact hits, {cert} certain = {100.0 * cert / max(hits, 1):.1f} % of the exact hits")
    assert hits > n // 10, "the cases no longer exercise the test"
    if typ in (SPHERE, CUBE):
        assert cert > n // 50, "the cases no longer exercise the test"
    else:
        assert cert == 0, "this type has no ball"
    bad = np.flatnonzero((certain != 0) & (exact == 0))
    assert bad.size == 0, f"{bad.size} cases certain without an exact hit, first: fwd={fwd[bad[0]]} inv={inv[bad[0]]} P={P[bad[0]]} L={L[bad[0]]}"


def test_no_ball_for_the_flat_types_and_bad_arguments():
    """plane, triangle, the meshes, cylinder and cone are never certain; a record whose two matrices are no pair gets no ball."""
    from portrayer_amd import _hip as H
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    fwd = np.array([[1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]])
    P = np.array([[0.1, 3.0, 0.05]])
    L = np.array([[0.1, -3.0, 0.05]])
    certain = np.zeros(1, dtype=np.int32)
    exact = np.zeros(1, dtype=np.int32)

    def run(typ, f, i):
        assert H.lib().pt_test_certain_shadow(1, typ, f.ctypes.data_as(dp), i.ctypes.data_as(dp), P.ctypes.data_as(dp), L.ctypes.data_as(dp), certain.ctypes.data_as(ip), exact.ctypes.data_as(ip)) == 0
        return int(certain[0]), int(exact[0])

    for typ in (SPHERE, CUBE):
        assert run(typ, fwd, fwd) == (1, 1)
    for typ in (CYLINDER, CONE):
        assert run(typ, fwd, fwd) == (0, 1)
    for typ in (1, 2, 3, 4):
        assert run(typ, fwd, fwd)[0] == 0
    moved = fwd.copy(); moved[0, 3] = 0.25
    assert run(SPHERE, moved, fwd)[0] == 0               # the centre does not map back
    assert H.lib().pt_test_certain_shadow(1, 9, fwd.ctypes.data_as(dp), fwd.ctypes.data_as(dp), P.ctypes.data_as(dp), L.ctypes.data_as(dp), certain.ctypes.data_as(ip), exact.ctypes.data_as(ip)) != 0
