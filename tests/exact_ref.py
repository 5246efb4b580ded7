"""The reference's ray/primitive decision structure restated in multi-precision arithmetic (test infrastructure).

Written from the Rust sources (primitive/*.rs, ray.rs, scene.rs, flat_scene.rs, camera.rs, math.rs, bounding_box.rs), not from oracle/ or the kernels:
this file is the third, independent reading that the other two are compared with. It evaluates what the reference DECIDES (first in-range root only,
half-open ranges, EPSILON-padded `contains`, faces and triangles in index order with a shrinking range), not idealised geometry, with mpmath at 256 bits
(`prec=256`), or at 53 bits (`prec=53`): the same expressions in plain f64 rounding, used only to measure how far a naive f64 evaluation strays.

Every comparison the algorithm makes records a margin: |gap to the threshold| / max(1, magnitudes compared). The discriminant's sign is relative to
max(b^2, |4ac|). A ray whose smallest margin is below 2^-30 is FRAGILE: a correct f64 implementation may decide it either way. The gap between the nearest
and the second-nearest candidate is among the margins by construction: every candidate's t is compared with the shrinking end of the range, which is the
best t so far. A division by an exact zero, a NaN and a zero-length normal are margin 0.
A triangle's six comparisons are one conjunction (see hit_triangle): a miss takes the margin of its most decisive failed comparison.

mode="kd" walks a scene k-d tree as kdtree/node.rs does: the ray segment's end is `start + extent` with extent the squared diagonal (quirk Q3), so with
directions that are not unit vectors it loses hits the flat walk finds, and the clipped start of a range decides which body root a cone sees (Q1). The
scene's tree is an input (the oracle's dump of its build; tests/exact_kd.py restates the build and tests/test_exact_kdtree.py holds the dump to it).

KDMesh (kdtree/kdmesh.rs:62-74) is the same walk over a tree of triangles in the mesh's model space, behind BoundingBox::test_hit on the tree's root
bounds. Its tree is NOT an input: it is built by tests/exact_kd.py in plain f64, which equals the reference's tree in every bit (argued there). The
walk's extent is the squared diagonal of the root bounds, so a KDMesh that is small against its distance from a ray's origin loses hits a Mesh finds
(Q3 again), and a KDMesh does not answer as a Mesh on purpose. Where the reference would panic (node.rs:146-147, quirk Q4) KdPanic is raised; cast()
reports such a ray as a miss of margin 0 with `panic` set. ExactScene.mutant names one deliberate misreading of the walk (WALK_MUTANTS), for showing that
the comparisons can fail.
"""
from __future__ import annotations

import math
from collections import deque

from mpmath import mp, mpf

import exact_kd
from scene_dsl import CONE, CUBE, CYLINDER, KDMESH, MESH, PLANE, SPHERE, TRIANGLE

EPS_F64 = 0.00001          # math.rs EPSILON: the f64 nearest to 1e-5, an exact rational here
FRAGILE = 2.0 ** -30
PREC = 256

# parts of a primitive, for coverage
BODY, CAP_TOP, CAP_BOTTOM = 0, 1, 2   # cylinder: 0, 1, 2; cone: 0 and 2 (its only cap is the bottom one)
TRI_FLAT, TRI_SMOOTH = 0, 1
WALK_MUTANTS = ("extent_plain_diagonal", "t_max_without_epsilon", "t_min_without_epsilon", "leaf_range_not_shrinking", "root_box_skipped",
                "far_side_from_start")


class Trace:
    """Smallest margin of the comparisons made for one ray, and whether a Q1 alternative exists."""
    __slots__ = ("margin", "q1", "far", "mutant")

    def __init__(self, mutant=None):
        self.margin = math.inf
        self.q1 = False
        self.far = {}        # per KDMesh geometry: was its last hit found on a pending far side of its tree?
        self.mutant = mutant

    def note(self, m):
        if m != m:
            self.margin = 0.0
        elif m < self.margin:
            self.margin = m

    def cmp(self, a, b):
        fa, fb = float(a), float(b)
        if fa != fa or fb != fb:
            self.margin = 0.0
            return
        if math.isinf(fa) or math.isinf(fb):
            return
        self.note(abs(float(a - b)) / max(1.0, abs(fa), abs(fb)))


def _margin(a, b):
    fa, fb = float(a), float(b)
    if fa != fa or fb != fb:
        return 0.0
    if math.isinf(fa) or math.isinf(fb):
        return math.inf
    return abs(float(a - b)) / max(1.0, abs(fa), abs(fb))


def _lt(tr, a, b):
    tr.cmp(a, b)
    return a < b


def _le(tr, a, b):
    tr.cmp(a, b)
    return a <= b


def _div(tr, a, b):
    if b == 0:
        tr.margin = 0.0   # the sign of an IEEE zero is not represented here
        return mp.nan if a == 0 else (mp.inf if a > 0 else -mp.inf)
    return a / b


def _in_range(tr, t, lo, hi):
    """Range<f64>::contains: lo <= t && t < hi."""
    if t != t:
        tr.margin = 0.0
        return False
    return _le(tr, lo, t) and _lt(tr, t, hi)


def _at(o, d, t):
    return (o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t)


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


# ---- matrices: 3x4 affine (rows of [A | t]); every builder call of scene.rs is affine
def _ident():
    return [[mpf(1), mpf(0), mpf(0), mpf(0)], [mpf(0), mpf(1), mpf(0), mpf(0)], [mpf(0), mpf(0), mpf(1), mpf(0)]]


def _mul(a, b):
    """a * b (b applied first)."""
    out = []
    for i in range(3):
        row = [a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j] for j in range(4)]
        row[3] = row[3] + a[i][3]
        out.append(row)
    return out


def _inverse(m):
    a, b, c = m[0][0], m[0][1], m[0][2]
    d, e, f = m[1][0], m[1][1], m[1][2]
    g, h, i = m[2][0], m[2][1], m[2][2]
    co = [[e * i - f * h, c * h - b * i, b * f - c * e],
          [f * g - d * i, a * i - c * g, c * d - a * f],
          [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = a * co[0][0] + b * co[1][0] + c * co[2][0]
    inv = [[co[r][k] / det for k in range(3)] for r in range(3)]
    t = (m[0][3], m[1][3], m[2][3])
    for r in range(3):
        inv[r].append(-(inv[r][0] * t[0] + inv[r][1] * t[1] + inv[r][2] * t[2]))
    return inv


def _point(m, p):
    return tuple(m[r][0] * p[0] + m[r][1] * p[1] + m[r][2] * p[2] + m[r][3] for r in range(3))


def _direction(m, v):
    return tuple(m[r][0] * v[0] + m[r][1] * v[1] + m[r][2] * v[2] for r in range(3))


def _normal(inv, n):
    """transformed_direction(invtrans.transposed()): the transpose of the inverse's 3x3 block."""
    return tuple(inv[0][c] * n[0] + inv[1][c] * n[1] + inv[2][c] * n[2] for c in range(3))


def _op_matrix(op, args):
    m = _ident()
    if op == "s":
        for k in range(3):
            m[k][k] = mpf(args[k])
    elif op == "t":
        for k in range(3):
            m[k][3] = mpf(args[k])
    else:
        a = mpf(args[0])
        c, s = mp.cos(a), mp.sin(a)
        if op == "x":
            m[1][1], m[1][2], m[2][1], m[2][2] = c, -s, s, c
        elif op == "y":
            m[0][0], m[0][2], m[2][0], m[2][2] = c, s, -s, c
        elif op == "z":
            m[0][0], m[0][1], m[1][0], m[1][1] = c, -s, s, c
        else:
            raise ValueError(op)
    return m


def compose_ops(ops):
    """scene.rs:163-205: each builder call multiplies its matrix onto the LEFT of the node's (the call made last is applied last)."""
    m = _ident()
    for op, args in ops:
        m = _mul(_op_matrix(op, args), m)
    return m


def from_f64_matrix(t):
    """A 4x4 f64 matrix (row-major, last row 0 0 0 1) as exact rationals."""
    assert float(t[3][0]) == 0.0 and float(t[3][1]) == 0.0 and float(t[3][2]) == 0.0 and float(t[3][3]) == 1.0
    return [[mpf(float(t[r][c])) for c in range(4)] for r in range(3)]


# ---- math.rs Quadratic::solve (roots::find_roots_quadratic): the real roots in ascending order
def _roots(tr, a, b, c, a_terms):
    if a == 0:
        tr.margin = 0.0
        if b == 0:
            return [mpf(0)] if c == 0 else []
        return [-c / b]
    tr.note(float(abs(a)) / max(float(abs(a_terms[0])), float(abs(a_terms[1])), 1e-300))
    bb, ac4 = b * b, 4 * a * c
    disc = bb - ac4
    tr.note(float(abs(disc)) / max(float(bb), float(abs(ac4)), 1e-300))
    if disc < 0:
        return []
    if disc == 0:
        return [-b / (2 * a)]
    sq = mp.sqrt(disc)
    q = -(b + sq) / 2 if b >= 0 else -(b - sq) / 2   # no cancellation: b and the root's sign agree
    if q == 0:
        tr.margin = 0.0
        return sorted([(-b + sq) / (2 * a), (-b - sq) / (2 * a)])
    x1, x2 = q / a, c / q
    return [x1, x2] if x1 < x2 else [x2, x1]


def _body_root(tr, roots, o, d, lo, hi, alt):
    """find_in_range, then the y window of cylinder.rs:57-60 / cone.rs:73-76. The reference tries the first in-range root only (quirk Q1); with
    `alt` the next in-range root is tried when the first fails the window. tr.q1 reports that this would have made a difference."""
    first = True
    for r in roots:
        if not _in_range(tr, r, lo, hi):
            continue
        p = _at(o, d, r)
        inside = not (_lt(tr, mpf(0.5), p[1]) | _lt(tr, p[1], mpf(-0.5)))
        if inside:
            if first:
                return r, p
            tr.q1 = True
            return (r, p) if alt else None
        if not first:
            return None
        first = False
    return None


def _cap(tr, height, o, d, lo, hi):
    t = _div(tr, height - o[1], d[1])
    if not _in_range(tr, t, lo, hi):
        return None
    p = _at(o, d, t)
    if _lt(tr, mpf(0.25), p[0] * p[0] + p[2] * p[2]):
        return None
    return t, p


def hit_sphere(tr, o, d, lo, hi, alt=False):
    a, b, c = _dot(d, d), 2 * _dot(o, d), _dot(o, o) - 1
    for r in _roots(tr, a, b, c, (a, a)):
        if _in_range(tr, r, lo, hi):
            p = _at(o, d, r)
            return r, p, p, 0, 0
    return None


def hit_cylinder(tr, o, d, lo, hi, alt=False):
    a = d[0] * d[0] + d[2] * d[2]
    b = 2 * o[0] * d[0] + 2 * o[2] * d[2]
    c = o[0] * o[0] + o[2] * o[2] - mpf(0.25)
    found = None
    body = _body_root(tr, _roots(tr, a, b, c, (a, a)), o, d, lo, hi, alt)
    if body is not None:
        t, p = body
        found, hi = (t, p, (p[0], mpf(0), p[2]), 0, BODY), t
    top = _cap(tr, mpf(0.5), o, d, lo, hi)
    if top is not None:
        found, hi = (top[0], top[1], (mpf(0), mpf(1), mpf(0)), 0, CAP_TOP), top[0]
    bottom = _cap(tr, mpf(-0.5), o, d, lo, hi)
    if bottom is not None:
        found = (bottom[0], bottom[1], (mpf(0), mpf(-1), mpf(0)), 0, CAP_BOTTOM)
    return found


def hit_cone(tr, o, d, lo, hi, alt=False):
    h, r2 = mpf(1), mpf(0.25)   # HEIGHT, RADIUS^2; cone.rs:58-62 as written
    a1, a2 = 4 * d[1] * d[1] * r2, 4 * h * h * (d[0] * d[0] + d[2] * d[2])
    a = a1 - a2
    b = -8 * h * h * (d[0] * o[0] + d[2] * o[2]) - 4 * r2 * (d[1] * h - 2 * d[1] * o[1])
    c = -4 * h * h * (o[0] * o[0] + o[2] * o[2]) + r2 * (h * h - 4 * h * o[1] + 4 * o[1] * o[1])
    found = None
    body = _body_root(tr, _roots(tr, a, b, c, (a1, a2)), o, d, lo, hi, alt)
    if body is not None:
        t, p = body
        tangent1 = _sub((mpf(0), mpf(0.5), mpf(0)), p)
        across = _sub((-p[0], p[1], -p[2]), p)
        n = _cross(tangent1, _cross(tangent1, across))
        found, hi = (t, p, n, 0, BODY), t
    cap = _cap(tr, mpf(-0.5), o, d, lo, hi)
    if cap is not None:
        found = (cap[0], cap[1], (mpf(0), mpf(-1), mpf(0)), 0, CAP_BOTTOM)
    return found


_CUBE_FACES = ((0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1))   # cube.rs:48-67: right, left, top, bottom, near, far


def _padded(tr, x):
    r = mpf(0.5) + mpf(EPS_F64)
    return _le(tr, -r, x) and _le(tr, x, r)


def _cube_contains(tr, p):
    return _padded(tr, p[0]) and _padded(tr, p[1]) and _padded(tr, p[2])


def hit_cube(tr, o, d, lo, hi, alt=False):
    found = None
    for k, (axis, s) in enumerate(_CUBE_FACES):
        # infinite_plane.rs:64-67 with normal s*e_axis and point (s/2)*e_axis
        t = _div(tr, -((o[axis] - mpf(s) / 2) * s), d[axis] * s)
        if not _in_range(tr, t, lo, hi):
            continue
        p = _at(o, d, t)
        if _cube_contains(tr, p):
            n = [mpf(0), mpf(0), mpf(0)]
            n[axis] = mpf(s)
            found, hi = (t, p, tuple(n), 0, k), t
    return found


def hit_plane(tr, o, d, lo, hi, alt=False):
    t = _div(tr, -o[1], d[1])
    if not _in_range(tr, t, lo, hi):
        return None
    p = _at(o, d, t)
    if _padded(tr, p[0]) and _padded(tr, p[2]):
        return t, p, (mpf(0), mpf(1), mpf(0)), 0, 0
    return None


def hit_triangle(tr, va, vb, vc, normals, o, dr, lo, hi):
    """triangle.rs:39-81 (Cramer's rule, bounds as written)."""
    a, b, c = _sub(va, vb)
    d, e, f = _sub(va, vc)
    g, h, i = dr
    j, k, l = _sub(va, o)
    ei_hf, gf_di, dh_eg = e * i - h * f, g * f - d * i, d * h - e * g
    m = a * ei_hf + b * gf_di + c * dh_eg
    ak_jb, jc_al, bl_ck = a * k - j * b, j * c - a * l, b * l - c * k
    t = _div(tr, -(f * ak_jb + e * jc_al + d * bl_ck), m)
    if m == 0 or t != t:
        return None
    gamma = (i * ak_jb + h * jc_al + g * bl_ck) / m
    beta = (j * ei_hf + k * gf_di + l * dh_eg) / m
    # The triangle is hit when all six comparisons pass, whatever their order. A hit is as safe as its weakest comparison; a miss is as safe as
    # its most decisive failed one (a triangle coplanar with the best hit so far ties with it in t, and is still a certain miss by beta or gamma).
    tests = ((lo <= t, lo, t), (t < hi, t, hi), (not gamma < 0, gamma, mpf(0)), (not gamma > 1, gamma, mpf(1)),
             (not beta < 0, beta, mpf(0)), (not beta > 1 - gamma, beta, 1 - gamma))
    failed = [_margin(a, b) for passed, a, b in tests if not passed]
    if failed:
        tr.note(max(failed))
        return None
    tr.note(min(_margin(a, b) for _, a, b in tests))
    if normals is not None:
        alpha = 1 - beta - gamma
        n = tuple(normals[0][q] * alpha + normals[1][q] * beta + normals[2][q] * gamma for q in range(3))
        part = TRI_SMOOTH
    else:
        n = _cross(_sub(vb, va), _sub(vc, va))
        part = TRI_FLAT
    return t, _at(o, dr, t), n, 0, part, (beta, gamma)   # beta and gamma: what triangle.rs:82-138 interpolates texture coordinates with


class KdPanic(Exception):
    pass


PANICS = [0]   # how many casts of this process reached the reference's panic


def _walk_kd(tr, t, leaf, me, o, d, lo, hi, extent):
    """kdtree/node.rs:66-203 over the tree `t` (the arrays of exact_kd / the oracle's dump). leaf(items, lo, hi) is `cast_ray` on a leaf's list: the
    nearest hit of the items in order, the range's end shrinking, as (t, ...) or None. Returns (hit, found on a pending far side)."""
    if t["kind"][me] == 1:
        f = t["first"][me]
        return leaf(t["items"][f:f + t["count"][me]], lo, hi), False
    mut = tr.mutant
    axis, plane = t["axis"][me], mpf(t["plane"][me])
    t_max = lo + extent
    if not _in_range(tr, t_max, lo, hi):
        t_max = hi if mut == "t_max_without_epsilon" else hi - mpf(EPS_F64)
    t_min = lo if mut == "t_min_without_epsilon" else lo + mpf(EPS_F64)
    # which_side: (p - point) . normal >= 0 is Front; the normal is the positive axis
    start_front = _le(tr, plane, o[axis] + d[axis] * t_min)
    end = o[axis] + d[axis] * t_max
    end_front = False if end != end else _le(tr, plane, end)
    if start_front == end_front:
        return _walk_kd(tr, t, leaf, t["front"][me] if start_front else t["back"][me], o, d, lo, hi, extent)
    plane_t = _div(tr, plane - o[axis], d[axis])
    if not _in_range(tr, plane_t, lo, hi):
        raise KdPanic()   # node.rs:146-147: the reference panics here (quirk Q4)
    first, second = (t["front"][me], t["back"][me]) if start_front else (t["back"][me], t["front"][me])
    h, far = _walk_kd(tr, t, leaf, first, o, d, lo, plane_t, extent)
    if h is not None:
        return h, far
    h, _ = _walk_kd(tr, t, leaf, second, o, d, lo if mut == "far_side_from_start" else plane_t, hi, extent)
    return h, h is not None


def _extent(tr, rb):
    """bounding_box.rs:95-99: the SQUARED diagonal (quirk Q3)."""
    e = sum((rb[3 + q] - rb[q]) ** 2 for q in range(3))
    return mp.sqrt(e) if tr.mutant == "extent_plain_diagonal" else e


class _Geometry:
    """A primitive's data, converted to the working precision on first use."""
    _trees = {}   # id(MeshData) -> (MeshData, its KDMesh tree): two nodes of one MeshData share one tree, and so do two scenes

    def __init__(self, prim):
        self.kind = prim.kind
        self.prim = prim
        self._cache = {}
        if self.kind not in (SPHERE, TRIANGLE, MESH, KDMESH, PLANE, CUBE, CYLINDER, CONE):
            raise ValueError("primitive kind %d is out of scope" % self.kind)

    def data(self):
        key = mp.prec
        if key not in self._cache:
            p = self.prim
            vec = lambda v: tuple(mpf(float(x)) for x in v)
            if self.kind == TRIANGLE:
                self._cache[key] = (vec(p.tri[0]), vec(p.tri[1]), vec(p.tri[2]), None if p.tri_normals is None else tuple(vec(n) for n in p.tri_normals))
            elif self.kind in (MESH, KDMESH):
                pos = [vec(v) for v in p.mesh.positions]
                nrm = [vec(v) for v in p.mesh.normals] if p.smooth else None
                if self.kind == KDMESH:   # kdmesh.rs:26-30: the root node's bounds
                    rb = [mpf(x) for x in self.tree()["root_bounds"]]
                    mn, mx = tuple(rb[:3]), tuple(rb[3:])
                else:
                    mn = tuple(min(v[q] for v in pos) for q in range(3))
                    mx = tuple(max(v[q] for v in pos) for q in range(3))
                size = tuple(max(mx[q] - mn[q], mpf(EPS_F64)) for q in range(3))   # bounding_box.rs:58-64
                centre = tuple((mn[q] + mx[q]) / 2 for q in range(3))
                self._cache[key] = (pos, nrm, [tuple(int(x) for x in t) for t in p.mesh.triangles], size, centre)
            else:
                self._cache[key] = None
        return self._cache[key]

    def tree(self):
        """KDMesh::new: the tree over the mesh's triangles (exact_kd.mesh_tree, plain f64), built once per MeshData."""
        m = self.prim.mesh
        if id(m) not in _Geometry._trees:
            _Geometry._trees[id(m)] = (m, exact_kd.mesh_tree(m))
        return _Geometry._trees[id(m)][1]

    def hit(self, tr, o, d, lo, hi, alt):
        k = self.kind
        if k == SPHERE:
            return hit_sphere(tr, o, d, lo, hi)
        if k == CYLINDER:
            return hit_cylinder(tr, o, d, lo, hi, alt)
        if k == CONE:
            return hit_cone(tr, o, d, lo, hi, alt)
        if k == CUBE:
            return hit_cube(tr, o, d, lo, hi)
        if k == PLANE:
            return hit_plane(tr, o, d, lo, hi)
        if k == TRIANGLE:
            va, vb, vc, nr = self.data()
            return hit_triangle(tr, va, vb, vc, nr, o, d, lo, hi)
        pos, nrm, tris, size, centre = self.data()
        # mesh.rs:152-166 behind bounding_box.rs:100-113: the box is the unit cube under scale(size) then translate(centre)
        bo = tuple((o[q] - centre[q]) / size[q] for q in range(3))
        bd = tuple(d[q] / size[q] for q in range(3))
        if not (k == KDMESH and tr.mutant == "root_box_skipped"):
            if not _cube_contains(tr, _at(bo, bd, lo)) and hit_cube(tr, bo, bd, lo, hi) is None:
                return None

        def nearest(items, lo, hi):   # ray.rs:50-63: [T]::ray_hit, the items in order, the range's end shrinking
            found = None
            for idx in items:
                ia, ib, ic = tris[idx]
                h = hit_triangle(tr, pos[ia], pos[ib], pos[ic], None if nrm is None else (nrm[ia], nrm[ib], nrm[ic]), o, d, lo, hi)
                if h is not None:
                    found = (h[0], h[1], h[2], idx, h[4], h[5])
                    if tr.mutant != "leaf_range_not_shrinking":
                        hi = h[0]
            return found

        if k == MESH:
            return nearest(range(len(tris)), lo, hi)
        # kdmesh.rs:72 over node.rs:33-51: the walk of the mesh's own tree; the first leaf with a hit wins
        tree = self.tree()
        found, far = _walk_kd(tr, tree, nearest, 0, o, d, lo, hi, _extent(tr, [mpf(x) for x in tree["root_bounds"]]))
        if found is not None:
            tr.far[id(self)] = far
        return found


class _Node:
    __slots__ = ("ops", "geometry", "children", "flat_id", "_m")

    def __init__(self, ops, geometry, children):
        self.ops, self.geometry, self.children, self.flat_id, self._m = ops, geometry, children, -1, {}

    def matrices(self):
        """(trans, inverse) of this level alone, composed from the builder calls at the working precision."""
        key = mp.prec
        if key not in self._m:
            t = compose_ops(self.ops)
            self._m[key] = (t, _inverse(t))
        return self._m[key]


class Hit:
    __slots__ = ("t", "node", "sub", "part", "point", "normal", "model_point", "kind", "margin", "q1", "bary", "far")   # bary: a triangle's (beta, gamma), else None
    panic = False

    def __repr__(self):
        return "Hit(t=%s node=%d sub=%d part=%d margin=%g q1=%s)" % (mp.nstr(self.t, 17), self.node, self.sub, self.part, self.margin, self.q1)


class Miss:
    __slots__ = ("margin", "q1", "panic")
    t = None
    far = False

    def __init__(self, margin, q1, panic=False):
        self.margin, self.q1, self.panic = margin, q1, panic

    def __bool__(self):
        return False


class ExactScene:
    """scene: a scene_dsl.Scene. flat_trans: the (n, 4, 4) f64 matrices of the flattened nodes (oracle_lib.flatten(...)["trans"]), taken as exact
    rationals; flat_scene.rs:22-38 orders them breadth first, which is re-derived here to tie each to its primitive."""

    def __init__(self, scene, flat_trans, prim_type=None):
        def build(n):
            return _Node(list(n.ops), None if n.geometry is None else _Geometry(n.geometry[0]), [build(c) for c in n.children])
        self.scene = scene   # its materials, lights and ambient colour are read by exact_shade
        self.root = build(scene.root)
        self.flat = []
        queue = deque([self.root])
        while queue:
            n = queue.popleft()
            if n.geometry is not None:
                n.flat_id = len(self.flat)
                self.flat.append(n)
            queue.extend(n.children)
        assert len(flat_trans) == len(self.flat), (len(flat_trans), len(self.flat))
        if prim_type is not None:
            assert [int(k) for k in prim_type] == [n.geometry.kind for n in self.flat]
        self.flat_trans = flat_trans
        self._fm = {}
        self.mutant = None   # one of WALK_MUTANTS

    def kinds(self):
        return [n.geometry.kind for n in self.flat]

    def flat_matrices(self):
        key = mp.prec
        if key not in self._fm:
            ts = [from_f64_matrix(t) for t in self.flat_trans]
            self._fm[key] = [(t, _inverse(t)) for t in ts]
        return self._fm[key]

    def composed(self, flat_id):
        """The product of the per-level matrices down to a flattened node (for checks)."""
        def walk(n, m):
            m = _mul(m, n.matrices()[0])
            if n.flat_id == flat_id:
                return m
            for c in n.children:
                r = walk(c, m)
                if r is not None:
                    return r
            return None
        return walk(self.root, _ident())

    # flat_scene.rs:71-99 under ray.rs:50-63
    def _cast_flat(self, tr, o, d, lo, hi, alt):
        best = None
        for i, (node, (t, inv)) in enumerate(zip(self.flat, self.flat_matrices())):
            lo_, ld = _point(inv, o), _direction(inv, d)
            h = node.geometry.hit(tr, lo_, ld, lo, hi, alt)
            if h is not None:
                hi = h[0]
                best = (h[0], i, h[3], h[4], _point(t, h[1]), _normal(inv, h[2]), h[1], node.geometry.kind, h[5] if len(h) > 5 else None)
        return best

    # kdtree/node.rs:66-203 over a given tree (the arrays of oracle_lib.kd_scene_dump: the BUILD of the tree is not restated here, its walk is)
    def set_tree(self, tree):
        self.tree = {k: ([int(x) for x in v] if k != "plane" and k != "root_bounds" else [float(x) for x in v]) for k, v in tree.items()}

    def _cast_kd(self, tr, o, d, lo, hi, extent, alt):
        mats = self.flat_matrices()

        def nearest(items, lo, hi):   # a leaf: its nodes in order, the range's end shrinking (ray.rs:80-92)
            best = None
            for i in items:
                tm, inv = mats[i]
                h = self.flat[i].geometry.hit(tr, _point(inv, o), _direction(inv, d), lo, hi, alt)
                if h is not None:
                    if tr.mutant != "leaf_range_not_shrinking":
                        hi = h[0]
                    best = (h[0], i, h[3], h[4], _point(tm, h[1]), _normal(inv, h[2]), h[1], self.flat[i].geometry.kind, h[5] if len(h) > 5 else None)
            return best
        return _walk_kd(tr, self.tree, nearest, 0, o, d, lo, hi, extent)[0]

    # scene.rs:80-120
    def _cast_hier(self, tr, node, o, d, lo, hi, alt):
        t, inv = node.matrices()
        lo_, ld = _point(inv, o), _direction(inv, d)
        best = None
        if node.geometry is not None:
            h = node.geometry.hit(tr, lo_, ld, lo, hi, alt)
            if h is not None:
                hi = h[0]
                best = (h[0], node.flat_id, h[3], h[4], _point(t, h[1]), _normal(inv, h[2]), h[1], node.geometry.kind, h[5] if len(h) > 5 else None)
        for c in node.children:
            h = self._cast_hier(tr, c, lo_, ld, lo, hi, alt)
            if h is not None:
                hi = h[0]
                best = (h[0], h[1], h[2], h[3], _point(t, h[4]), _normal(inv, h[5]), h[6], h[7], h[8])
        return best

    def cast(self, origin, direction, t_max=math.inf, mode="flat", prec=PREC, alt=False):
        """Nearest hit over [EPSILON, t_max): a Hit, or a Miss (falsy). `alt` evaluates the Q1 alternative."""
        old = mp.prec
        mp.prec = prec
        try:
            assert self.mutant is None or self.mutant in WALK_MUTANTS, self.mutant
            tr = Trace(self.mutant)
            panic = False
            o = tuple(mpf(float(x)) if not isinstance(x, mpf) else +x for x in origin)
            d = tuple(mpf(float(x)) if not isinstance(x, mpf) else +x for x in direction)
            lo = mpf(EPS_F64)
            hi = t_max if isinstance(t_max, mpf) else (mp.inf if math.isinf(t_max) else mpf(float(t_max)))
            try:
                if mode == "flat":
                    best = self._cast_flat(tr, o, d, lo, hi, alt)
                elif mode == "hier":
                    best = self._cast_hier(tr, self.root, o, d, lo, hi, alt)
                elif mode == "kd":
                    best = self._cast_kd(tr, o, d, lo, hi, _extent(tr, [mpf(x) for x in self.tree["root_bounds"]]), alt)
                else:
                    raise ValueError(mode)
            except KdPanic:   # in the scene's tree or in a KDMesh's
                best, panic = None, True
                PANICS[0] += 1
                tr.margin = 0.0
            if best is None:
                return Miss(tr.margin, tr.q1, panic)
            h = Hit()
            h.t, h.node, h.sub, h.part, h.point, n, h.model_point, h.kind, h.bary = best
            s = _dot(n, n)
            if s == 0 or s != s:
                tr.margin = 0.0
                h.normal = (mp.nan, mp.nan, mp.nan)
            else:
                r = mp.sqrt(s)
                h.normal = (n[0] / r, n[1] / r, n[2] / r)
            h.margin, h.q1 = tr.margin, tr.q1
            h.far = tr.far.get(id(self.flat[h.node].geometry), False)
            return h
        finally:
            mp.prec = old


def implicit_residual(kind, part, p, geometry=None, sub=0):
    """How far a model-space hit point is from satisfying its surface's equation (0 on the surface)."""
    x, y, z = p
    if kind == SPHERE:
        return abs(x * x + y * y + z * z - 1)
    if kind == PLANE:
        return abs(y)
    if kind == CUBE:
        axis, s = _CUBE_FACES[part]
        return abs(p[axis] - mpf(s) / 2)
    if kind == CYLINDER:
        return abs(x * x + z * z - mpf(0.25)) if part == BODY else abs(y - (mpf(0.5) if part == CAP_TOP else mpf(-0.5)))
    if kind == CONE:
        return abs(x * x + z * z - (y - mpf(0.5)) ** 2 / 4) if part == BODY else abs(y + mpf(0.5))
    if kind == TRIANGLE:
        va, vb, vc, _ = geometry.data()
    else:
        pos, _, tris, _, _ = geometry.data()
        va, vb, vc = (pos[q] for q in tris[sub])
    n = _cross(_sub(vb, va), _sub(vc, va))
    return abs(_dot(n, _sub(p, va))) / mp.sqrt(_dot(n, n))


# ---- camera.rs:34-84
def camera_rays(cam, width, height, xy, prec=PREC):
    """Eye rays through the image positions xy (pixels): (origin, [directions]) at the working precision, not rounded."""
    old = mp.prec
    mp.prec = prec
    try:
        eye = tuple(mpf(float(x)) for x in cam.eye)
        centre = tuple(mpf(float(x)) for x in cam.center)
        up = tuple(mpf(float(x)) for x in cam.up)
        unit = lambda v: tuple(c / mp.sqrt(_dot(v, v)) for c in v)
        f = unit(_sub(centre, eye))
        s = unit(_cross(f, up))
        u = _cross(s, f)
        # look_at_rh: world to view; rows s, u, -f and the eye moved to the origin
        world_to_view = [[s[0], s[1], s[2], -_dot(s, eye)], [u[0], u[1], u[2], -_dot(u, eye)], [-f[0], -f[1], -f[2], _dot(f, eye)]]
        view_to_world = _inverse(world_to_view)
        fov = mp.tan(mpf(float(cam.fovy_radians)) / 2)
        w, h = mpf(float(width)), mpf(float(height))
        aspect = w / h
        dirs = []
        for x, y in xy:
            vy = (1 - 2 * (mpf(float(y)) / h)) * fov
            vx = (2 * (mpf(float(x)) / w) - 1) * aspect * fov
            dirs.append(unit(_sub(_point(view_to_world, (vx, vy, mpf(-1))), eye)))
        return eye, dirs
    finally:
        mp.prec = old
