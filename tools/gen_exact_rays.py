#!/usr/bin/env python3
"""Generates tests/golden/exact/: scenes, ray batches and the exact reference's answers for them (tests/exact_ref.py).

    python tools/gen_exact_rays.py            # regenerate every file (a few minutes; deterministic, byte for byte)
    python tools/gen_exact_rays.py --check    # regenerate one batch and compare its bytes, re-assert the input conditions, print the shares

The scene builders and the input conditions need only numpy and tests/scene_dsl.py, so the tests import them from here; mpmath is needed to evaluate.
The fragility margin (2^-30), the factor on the measured tolerance (64) and the caps on the shares below were fixed before anything was measured.
"""
from __future__ import annotations

import argparse
import io
import json
import math
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from scene_dsl import (ASSETS, CONE, CUBE, CYLINDER, MESH, PLANE, SPHERE, TRIANGLE, Camera, Cone, Cube, Cylinder, Material, Mesh, MeshData,  # noqa: E402
                       Node, Plane, Scene, Sphere, Triangle)

OUT = os.path.join(ROOT, "tests", "golden", "exact")
SCENES = ("flat15", "nested15", "thin", "tris")
BATCHES = (("random", 1024), ("near", 1024), ("special", 512))
CAM_W, CAM_H = 16, 12
FRAGILE = 2.0 ** -30
SLACK = 64.0
THRESHOLD_CAP = 2.0 ** -32
ILL = THRESHOLD_CAP / SLACK / 2   # 2^-39: see well_conditioned()
FRAGILE_CAP = {"random": 0.01, "near": 0.10, "special": 0.15, "camera": 0.10}
HIT_SHARE = 0.25
KIND_MIN, PART_MIN = 20, 5
Q1_CAP = 0.15
SEGMENT = 2.0 ** -20
T_MAX_MISS = 1000.0
KD_DEPTH = 6
KIND_NAME = {SPHERE: "sphere", TRIANGLE: "triangle", MESH: "mesh", PLANE: "plane", CUBE: "cube", CYLINDER: "cylinder", CONE: "cone"}
# the parts every kind must be hit on: cylinder body/top/bottom, cone body/bottom cap, the six cube faces
PARTS = {SPHERE: (0,), PLANE: (0,), CUBE: (0, 1, 2, 3, 4, 5), CYLINDER: (0, 1, 2), CONE: (0, 2)}
CHECK_BATCH = ("thin", "special")


# ---------------------------------------------------------------- scenes
def _material(k):
    return Material(diffuse=(0.1 + 0.05 * (k % 16), 0.9 - 0.05 * (k % 13), 0.2 + 0.04 * (k % 19)), specular=(0.3, 0.3, 0.3), shininess=10.0 + k)


def _leaves15(seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(15):
        prim = (Sphere, Cube, Plane, Cylinder, Cone)[k % 5]()
        n = Node.geo(prim, _material(k)).scaled(tuple(rng.uniform(0.5, 2.5, 3))).rotated_xzy(tuple(rng.uniform(-math.pi, math.pi, 3)))
        out.append(n.translated(tuple(rng.uniform(-4.0, 4.0, 3))))
    return out


def scene_flat15():
    return Scene(Node.group(_leaves15(1501)), [], (0.1, 0.1, 0.1))


def scene_nested15():
    lv = _leaves15(1501)
    rng = np.random.default_rng(1502)
    def placed(g, scale):
        return g.scaled(scale).rotated_xzy(tuple(rng.uniform(-math.pi, math.pi, 3))).translated(tuple(rng.uniform(-2.0, 2.0, 3)))
    g3 = placed(Node.group(lv[10:15]), (0.8, 1.3, 0.9))
    g2 = placed(Node.group(lv[5:10] + [g3]), (-1.2, 0.75, 1.1))   # a mirroring scale: negative determinant
    g1 = placed(Node.group(lv[0:5] + [g2]), (1.25, 0.9, 0.7))
    return Scene(Node.group([g1]), [], (0.1, 0.1, 0.1))


def scene_thin():
    rng = np.random.default_rng(1503)
    spec = ((Cylinder, (2.0, 2.0 / 64, 2.0)),        # a disc
            (Cylinder, (0.05, 3.2, 0.05)),          # a needle
            (Plane, (4.0, 1.0, 4.0 / 64)),          # a sliver
            (Cone, (0.0625, 4.0, 0.0625)),          # a needle
            (Sphere, (1.5, 1.5 / 64, 1.5)),         # a disc
            (Cube, (3.0, 3.0 / 64, 2.0)))           # a slab, 1e3 from the origin
    nodes = []
    for k, (prim, scale) in enumerate(spec):
        n = Node.geo(prim(), _material(k)).scaled(scale).rotated_xzy(tuple(rng.uniform(-math.pi, math.pi, 3)))
        nodes.append(n.translated((600.0, -640.0, 480.0) if k == 5 else tuple(rng.uniform(-3.0, 3.0, 3))))
    return Scene(Node.group(nodes), [], (0.1, 0.1, 0.1))


def scene_tris():
    rng = np.random.default_rng(1504)
    centre = (0.0, 0.6, 0.0)
    rim = [(1.5 * math.cos(k * math.pi / 4), 0.25 * (k % 2), 1.5 * math.sin(k * math.pi / 4)) for k in range(8)]
    angles, shift = tuple(rng.uniform(-math.pi, math.pi, 3)), (-2.5, 1.0, 0.5)
    nodes = []
    for k in range(8):   # a closed fan: triangle k shares an edge with k-1 and k+1, and all share the centre
        a, b, c = centre, rim[(k + 1) % 8], rim[k]
        normals = None
        if k % 2:
            normals = [(0.0, 1.0, 0.0), (0.4 * b[0], 1.0, 0.4 * b[2]), (0.4 * c[0], 1.0, 0.4 * c[2])]
        nodes.append(Node.geo(Triangle(a, b, c, normals=normals), _material(k)).scaled((1.4, 0.8, 1.1)).rotated_xzy(angles).translated(shift))
    dodeca = MeshData.load_obj(os.path.join(ASSETS, "dodeca.obj"))
    bucky = MeshData.load_obj(os.path.join(ASSETS, "buckyball.obj"))
    nodes.append(Node.geo(Mesh(dodeca), _material(8)).scaled((0.9, 0.6, 0.75)).rotated_xzy(tuple(rng.uniform(-math.pi, math.pi, 3))).translated((2.0, -1.0, -1.5)))
    nodes.append(Node.geo(Mesh(bucky, smooth=True), _material(9)).scaled((0.5, 0.65, 0.4)).rotated_xzy(tuple(rng.uniform(-math.pi, math.pi, 3)))
                 .translated((1.0, 2.0, 2.5)))
    return Scene(Node.group(nodes), [], (0.1, 0.1, 0.1))


def build_scene(name):
    return {"flat15": scene_flat15, "nested15": scene_nested15, "thin": scene_thin, "tris": scene_tris}[name]()


def flat_prims(scene):
    """The primitives of the flattened nodes, breadth first (flat_scene.rs:22-38)."""
    out, queue = [], [scene.root]
    while queue:
        n = queue.pop(0)
        if n.geometry is not None:
            out.append(n.geometry[0])
        queue.extend(n.children)
    return out


def model_box(prim):
    if prim.kind == SPHERE:
        return np.full(3, -1.0), np.full(3, 1.0)
    if prim.kind == TRIANGLE:
        return prim.tri.min(axis=0), prim.tri.max(axis=0)
    if prim.kind == MESH:
        return prim.mesh.positions.min(axis=0), prim.mesh.positions.max(axis=0)
    lo = np.array([-0.5, 0.0 if prim.kind == PLANE else -0.5, -0.5])
    return lo, -lo


def world_box(trans, prim):
    lo, hi = model_box(prim)
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    w = corners @ trans[:3, :3].T + trans[:3, 3]
    return w.min(axis=0), w.max(axis=0)


def regions(trans, prims):
    """Boxes to start rays in and around: the nodes near the origin together, every far node on its own. (box lo, box hi, node ids)."""
    boxes = [world_box(t, p) for t, p in zip(trans, prims)]
    near = [i for i, (lo, hi) in enumerate(boxes) if np.linalg.norm((lo + hi) / 2) < 100.0]
    out = []
    if near:
        out.append((np.min([boxes[i][0] for i in near], axis=0), np.max([boxes[i][1] for i in near], axis=0), near))
    for i in range(len(boxes)):
        if i not in near:
            e = np.maximum(boxes[i][1] - boxes[i][0], 1.0)
            out.append((boxes[i][0] - 2 * e, boxes[i][1] + 2 * e, [i]))
    return out


def scene_camera(trans, prims):
    lo, hi, _ = regions(trans, prims)[0]
    c, e = (lo + hi) / 2, (hi - lo) / 2
    eye = c + np.array([0.55, 0.4, 1.0]) * np.linalg.norm(e) * 1.35
    return Camera(eye=tuple(eye), center=tuple(c + 0.05 * e), up=(0.0, 1.0, 0.0), fovy_degrees=50.0)


# ---------------------------------------------------------------- rays
def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _lengths(rng, d):
    return d / np.linalg.norm(d) * 10.0 ** rng.uniform(-2.0, 2.0)


def _to_world(trans, p):
    return trans[:3, :3] @ p + trans[:3, 3]


def _inside_point(rng, prim, spread=0.35):
    lo, hi = model_box(prim)
    return (lo + hi) / 2 + (hi - lo) / 2 * spread * rng.uniform(-1, 1, 3)


def _pick_region(rng, regs):
    w = np.array([len(r[2]) for r in regs], dtype=np.float64)
    return regs[rng.choice(len(regs), p=w / w.sum())]


def batch_random(seed, n, trans, prims):
    rng = np.random.default_rng(seed)
    regs = regions(trans, prims)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    for k in range(n):
        lo, hi, ids = _pick_region(rng, regs)
        c, e = (lo + hi) / 2, (hi - lo) / 2 * 1.1
        o[k] = c + e * rng.uniform(-1, 1, 3) if rng.random() < 0.5 else c + _unit(rng) * rng.uniform(1.2, 4.0) * np.linalg.norm(e)
        if k % 2 == 0:   # half the rays aim into the scene
            i = ids[rng.integers(len(ids))]
            d[k] = _to_world(trans[i], _inside_point(rng, prims[i])) - o[k]
        else:
            d[k] = _unit(rng)
        d[k] = _lengths(rng, d[k])
    # origins on a 2^-6 grid and directions of 11 significant bits: arbitrary rays all the same, and a fraction of the bytes in the fixture
    o, d = _grid(o), d.astype(np.float16).astype(np.float64)
    p = rng.permutation(n)
    return o[p], d[p]


def _grid(o):
    return np.round(o * 64.0) / 64.0


def _perp(rng, v):
    w = np.cross(v, _unit(rng))
    return w / np.linalg.norm(w)


def _rim(rng, y):
    th = rng.uniform(0, 2 * math.pi)
    r = np.array([math.cos(th), 0.0, math.sin(th)])
    return 0.5 * r + np.array([0.0, y, 0.0]), (r if rng.random() < 0.5 else np.array([0.0, 1.0, 0.0]))


def _tri_feature(rng, a, b, c):
    v = [a, b, c]
    k = rng.integers(3)
    p0, p1 = v[k], v[(k + 1) % 3]
    nrm = np.cross(b - a, c - a)
    if rng.random() < 0.35:   # a vertex, displaced anywhere in the plane
        u = _perp(rng, nrm)
        return p0, np.cross(nrm, u) / np.linalg.norm(np.cross(nrm, u))
    u = np.cross(nrm, p1 - p0)
    return p0 + rng.uniform(0.05, 0.95) * (p1 - p0), u / np.linalg.norm(u)


def feature(rng, prim, model_origin):
    """A model-space feature point of the primitive and a unit direction that runs across the feature."""
    k = prim.kind
    if k == SPHERE:   # a point of the silhouette as the origin sees it, displaced radially
        l2 = float(model_origin @ model_origin)
        if l2 <= 1.0001:
            p = _unit(rng)
            return p, p
        p = model_origin / l2 + math.sqrt(1.0 - 1.0 / l2) * _perp(rng, model_origin)
        return p, p / np.linalg.norm(p)
    if k == CUBE:     # an edge or a corner, displaced along its diagonal
        s = rng.choice([-1.0, 1.0], size=3)
        p, u = 0.5 * s, s.copy()
        if rng.random() < 0.6:
            ax = rng.integers(3)
            p[ax], u[ax] = rng.uniform(-0.45, 0.45), 0.0
        return p, u / np.linalg.norm(u)
    if k == PLANE:    # the border
        ax = 0 if rng.random() < 0.5 else 2
        p, u = np.zeros(3), np.zeros(3)
        p[ax], u[ax] = 0.5 * rng.choice([-1.0, 1.0]), 1.0
        p[2 - ax] = rng.uniform(-0.5, 0.5) if rng.random() < 0.8 else 0.5 * rng.choice([-1.0, 1.0])
        return p, u
    if k == CYLINDER:  # the seam of the body and a cap
        return _rim(rng, 0.5 * rng.choice([-1.0, 1.0]))
    if k == CONE:     # the apex or the base rim
        if rng.random() < 0.35:
            return np.array([0.0, 0.5, 0.0]), _unit(rng)
        return _rim(rng, -0.5)
    if k == TRIANGLE:
        return _tri_feature(rng, *prim.tri)
    lo, hi = model_box(prim)
    if rng.random() < 0.3:   # a corner of the mesh's box
        s = rng.choice([-1.0, 1.0], size=3)
        return np.where(s > 0, hi, lo), s / math.sqrt(3.0)
    t = prim.mesh.triangles[rng.integers(len(prim.mesh.triangles))]
    return _tri_feature(rng, *(prim.mesh.positions[int(q)] for q in t))


def batch_near(seed, n, trans, prims):
    rng = np.random.default_rng(seed)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    for k in range(n):
        i = int(rng.integers(len(prims)))
        lo, hi = world_box(trans[i], prims[i])
        if prims[i].kind == SPHERE:   # a silhouette is grazed: from 1.5 to 2.5 radii the discriminant's margin stays above 2^-27 at the smallest offset
            o[k] = _grid(_to_world(trans[i], _unit(rng) * rng.uniform(1.5, 2.5)))
        elif k % 2:   # a distance chosen in world space, or in model space (where a thin node's silhouette is better conditioned)
            o[k] = _grid((lo + hi) / 2 + _unit(rng) * rng.uniform(1.5, 4.0) * np.linalg.norm(hi - lo) / 2)
        else:
            mlo, mhi = model_box(prims[i])
            o[k] = _grid(_to_world(trans[i], (mlo + mhi) / 2 + _unit(rng) * rng.uniform(1.5, 4.0) * np.linalg.norm(mhi - mlo) / 2))
        p, u = feature(rng, prims[i], (np.linalg.inv(trans[i]) @ np.append(o[k], 1.0))[:3])
        off = rng.choice([-1.0, 1.0]) * 2.0 ** rng.uniform(-24.0, -6.0)
        d[k] = _lengths(rng, _to_world(trans[i], p + off * u) - o[k])
    p = rng.permutation(n)
    return o[p], d[p]


def batch_special(seed, n, trans, prims, prev):
    """prev: the scene's `random` batch with its answers (surface points to start from)."""
    rng = np.random.default_rng(seed)
    regs = regions(trans, prims)
    n_axis, n_zero, n_surface = n // 4, n // 4, 3 * (n // 8)
    o, d = [], []
    for _ in range(n_axis):   # exactly axis-parallel in a node's model space, mapped out with trans
        i = int(rng.integers(len(prims)))
        lo, hi = model_box(prims[i])
        c, e = (lo + hi) / 2, np.maximum((hi - lo) / 2, 0.25)
        ax, s = int(rng.integers(3)), float(rng.choice([-1.0, 1.0]))
        om = c + e * rng.uniform(-0.9, 0.9, 3)
        om[ax] = c[ax] - s * e[ax] * rng.uniform(2.0, 6.0) if rng.random() < 0.75 else c[ax] + e[ax] * rng.uniform(-0.5, 0.5)
        dm = np.zeros(3)
        dm[ax] = s * 10.0 ** rng.uniform(-2.0, 2.0)
        o.append(_to_world(trans[i], om)); d.append(trans[i][:3, :3] @ dm)
    for _ in range(n_zero):   # world components of +0 or -0
        lo, hi, ids = _pick_region(rng, regs)
        i = ids[rng.integers(len(ids))]
        target = _to_world(trans[i], _inside_point(rng, prims[i]))
        v = _unit(rng)
        zero = rng.choice(3, size=int(rng.integers(1, 3)), replace=False)
        v[zero] = rng.choice([0.0, -0.0], size=len(zero))
        v = v / np.linalg.norm(v)
        o.append(target - v * rng.uniform(1.0, 5.0) * np.linalg.norm(hi - lo) / 4)
        d.append(v * 10.0 ** rng.uniform(-2.0, 2.0))
    ok = np.flatnonzero(prev["hit"] & ~prev["fragile"])
    pick = ok[rng.choice(len(ok), size=n_surface // 3, replace=len(ok) < n_surface // 3)]
    for j in pick:            # origins on surfaces: exact hit points rounded to f64, re-cast along the normal, against it, along the mirror direction
        p, nr = prev["point"][j], prev["normal"][j]
        din = prev["d"][j] / np.linalg.norm(prev["d"][j])
        for v in (nr, -nr, din - 2.0 * float(din @ nr) * nr):
            o.append(p.copy()); d.append(_lengths(rng, v))
    cones = [i for i, p in enumerate(prims) if p.kind == CONE]
    rest = n - len(o)
    for _ in range(3 * rest // 8 if cones else 0):   # the last hundredth of a cone below its apex, met squarely from a short distance (well conditioned there)
        i = cones[rng.integers(len(cones))]
        y, th = 0.5 - 10.0 ** rng.uniform(-3.5, -2.0), rng.uniform(0, 2 * math.pi)
        r = (0.5 - y) / 2
        p = np.array([r * math.cos(th), y, r * math.sin(th)])
        om = p + np.array([2 * math.cos(th), 1.0, 2 * math.sin(th)]) / math.sqrt(5.0) * rng.uniform(0.1, 0.3)
        o.append(_to_world(trans[i], om)); d.append(_lengths(rng, trans[i][:3, :3] @ (p - om)))
    for j in ok[rng.choice(len(ok), size=3 * rest // 8)]:   # hits between EPSILON and ten times EPSILON: the start of the range
        t0 = 10.0 ** rng.uniform(-4.7, -4.1)
        dj = prev["d"][j] * rng.choice([-1.0, 1.0])
        o.append(prev["point"][j] - dj * t0); d.append(dj.copy())
    solid = [i for i, p in enumerate(prims) if p.kind in (SPHERE, CUBE, CYLINDER, CONE, MESH)] or list(range(len(prims)))
    while len(o) < n:          # origins inside primitives
        i = solid[rng.integers(len(solid))]
        o.append(_to_world(trans[i], _inside_point(rng, prims[i], 0.2))); d.append(_lengths(rng, _unit(rng)))
    o, d = np.array(o), np.array(d)
    p = rng.permutation(n)
    return o[p], d[p]


# ---------------------------------------------------------------- evaluation
_EX = None
_RAYS = None
try:
    from mpmath import mp
    import exact_ref
except ImportError:   # the tests' numpy-only half
    mp = exact_ref = None


def _row(h):
    f = lambda v: [float(x) for x in v]
    if not h:
        return dict(hit=False, t=math.inf, node=-1, sub=-1, part=-1, point=[0.0] * 3, normal=[0.0] * 3)
    return dict(hit=True, t=float(h.t), node=h.node, sub=h.sub, part=h.part, point=f(h.point), normal=f(h.normal))


def _same(a, b):
    return bool(a) == bool(b) and (not a or (a.node == b.node and a.sub == b.sub))


def _identical(a, b):
    return _same(a, b) and (not a or a.t == b.t)


def _deviation(h53, h):
    """The 53-bit evaluation minus the 256-bit one, before either is rounded to f64: t, point, normal. None where they cannot be compared."""
    if not h or not h53 or h53.node != h.node or h53.sub != h.sub:
        return None
    with mp.workprec(exact_ref.PREC):
        return [float(h53.t - h.t)] + [float(a - b) for a, b in zip(h53.point, h.point)] + [float(a - b) for a, b in zip(h53.normal, h.normal)]


def _evaluate(k):
    ex = _EX
    o, d = _RAYS[k]
    d53 = d
    if isinstance(d, tuple):   # a camera ray: (direction at 256 bits, direction at 53 bits)
        d, d53 = d
    h = ex.cast(o, d)
    r = _row(h)
    margin = h.margin
    hh = ex.cast(o, d, mode="hier")
    r["hier"] = _row(hh)
    r["hier_margin"] = hh.margin
    h53 = ex.cast(o, d53, prec=53)
    r["f53"] = _row(h53)
    r["dev"] = _deviation(h53, h) or [0.0] * 7
    # the k-d tree walk answers differently where quirks Q1 and Q3 bite; it is stored where it does
    kd = ex.cast(o, d, mode="kd")
    r["kd"], r["kd_margin"], r["kd_differs"] = _row(kd), kd.margin, not _identical(kd, h)
    r["kd_dev"] = [0.0] * 7
    if r["kd_differs"] and kd:
        r["kd_dev"] = _deviation(ex.cast(o, d53, mode="kd", prec=53), kd) or [math.inf] * 7
    r["q1"] = bool(h.q1)
    r["alt"] = _row(ex.cast(o, d, alt=True)) if h.q1 else None
    if h:
        t = float(h.t)
        r["t_max"] = [t * (1.0 - SEGMENT), t * (1.0 + SEGMENT)]
        below, above = ex.cast(o, d, t_max=r["t_max"][0]), ex.cast(o, d, t_max=r["t_max"][1])
        assert _same(above, h) and above.t == h.t, "a bound just above the hit must not change it"
        r["below"] = _row(below)
        r["segment_margin"] = min(below.margin, above.margin)
        kd_below, kd_above = ex.cast(o, d, mode="kd", t_max=r["t_max"][0]), ex.cast(o, d, mode="kd", t_max=r["t_max"][1])
        r["kd_below"], r["kd_below_differs"] = _row(kd_below), not _identical(kd_below, below)
        r["kd_above"], r["kd_above_differs"] = _row(kd_above), not _identical(kd_above, h)
        r["kd_segment_margin"] = min(kd_below.margin, kd_above.margin)
    else:
        r["t_max"] = [T_MAX_MISS, T_MAX_MISS]
        below = ex.cast(o, d, t_max=T_MAX_MISS)
        assert not below
        r["below"] = _row(below)
        r["segment_margin"] = below.margin
        kd_below = ex.cast(o, d, mode="kd", t_max=T_MAX_MISS)
        r["kd_below"], r["kd_below_differs"] = _row(kd_below), bool(kd_below)
        r["kd_above"], r["kd_above_differs"] = r["kd_below"], bool(kd_below)
        r["kd_segment_margin"] = kd_below.margin
    r["margin"] = margin
    return r


def well_conditioned(r):
    """The threshold is 64 times what the reference's own f64 evaluation strays by and has to stay below 2^-32, so a batch cannot hold a ray that
    strays by 2^-38 on its own: such a ray (a hit that grazes a quadric, or lies next to a cone's apex, where the discriminant's margin is small but above
    the fragility margin) is left out as badly conditioned and the next ray of the stream takes its place. A property of the exact reference alone."""
    for dev, hit in ((np.array(r["kd_dev"]), r["kd"]), (np.array(r["dev"]), r)):
        if not _well(dev, hit):
            return False
    return True


def _well(dev, r):
    if not r["hit"]:
        return True
    return (abs(dev[0]) <= ILL * max(1.0, abs(r["t"])) and np.linalg.norm(dev[1:4]) <= ILL * max(1.0, float(np.linalg.norm(r["point"])))
            and np.linalg.norm(dev[4:7]) <= ILL)


def evaluate(ex, rays, workers):
    global _EX, _RAYS
    _EX, _RAYS = ex, rays
    if workers <= 1:
        return [_evaluate(k) for k in range(len(rays))]
    import multiprocessing
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        return pool.map(_evaluate, range(len(rays)), chunksize=8)


def _largest(dev, t, point):
    if not len(dev):
        return np.zeros(3)
    return np.array([np.max(np.abs(dev[:, 0]) / np.maximum(1.0, np.abs(t))),
                     np.max(np.linalg.norm(dev[:, 1:4], axis=1) / np.maximum(1.0, np.linalg.norm(point, axis=1))),
                     np.max(np.linalg.norm(dev[:, 4:7], axis=1))])


def columns(o, d, rows):
    """The stored arrays of a batch. Values are the 256-bit results rounded to f64; *53 are the 53-bit evaluation's."""
    n = len(rows)
    col = lambda key, dt, sub=None: np.array([(r[key] if sub is None else r[sub][key]) for r in rows], dtype=dt)
    c = dict(o=np.ascontiguousarray(o, dtype=np.float64), d=np.ascontiguousarray(d, dtype=np.float64))
    c["hit"], c["t"], c["node"], c["sub"], c["part"] = col("hit", np.bool_), col("t", np.float64), col("node", np.int32), col("sub", np.int32), col("part", np.int8)
    c["point"], c["normal"] = col("point", np.float64).reshape(n, 3), col("normal", np.float64).reshape(n, 3)
    c["fragile"] = np.array([r["margin"] < FRAGILE for r in rows])
    c["hier_fragile"] = np.array([r["hier_margin"] < FRAGILE for r in rows])
    c["hier_hit"], c["hier_node"], c["hier_sub"] = col("hit", np.bool_, "hier"), col("node", np.int32, "hier"), col("sub", np.int32, "hier")
    with np.errstate(invalid="ignore"):
        c["hier_dt"] = (col("t", np.float64, "hier") - c["t"]).astype(np.float32)
    c["hier_dt"][~(c["hit"] & c["hier_hit"])] = 0.0
    c["hit53"], c["node53"] = col("hit", np.bool_, "f53"), col("node", np.int32, "f53")
    dev = col("dev", np.float64).reshape(n, 7)
    c["dt53"], c["dnormal53"] = dev[:, 0].astype(np.float32), dev[:, 4:7].astype(np.float32)   # the 53-bit evaluation's t and normal, as differences
    m = c["hit"] & ~c["fragile"] & c["hit53"] & (c["node53"] == c["node"])
    c["dev53"] = _largest(dev[m], c["t"][m], c["point"][m])
    # the k-d walk's answers, nearest and for the two bounds, where they are not the flat walk's
    c["kd_fragile"] = np.array([r["kd_margin"] < FRAGILE for r in rows])
    c["kd_segment_fragile"] = np.array([r["kd_segment_margin"] < FRAGILE for r in rows])
    for key in ("kd", "kd_below", "kd_above"):
        idx = [k for k, r in enumerate(rows) if r[key + "_differs"]]
        c[key + "_idx"] = np.array(idx, dtype=np.int32)
        sp = lambda name, dt, w: np.array([rows[k][key][name] for k in idx], dtype=dt).reshape((len(idx),) + w)
        c[key + "_hit"], c[key + "_t"], c[key + "_node"], c[key + "_sub"] = sp("hit", np.bool_, ()), sp("t", np.float64, ()), sp("node", np.int32, ()), sp("sub", np.int32, ())
        c[key + "_point"], c[key + "_normal"] = sp("point", np.float64, (3,)), sp("normal", np.float64, (3,))
    kdev = np.array([rows[k]["kd_dev"] for k in c["kd_idx"]], dtype=np.float64).reshape(len(c["kd_idx"]), 7)
    c["kd_dt53"], c["kd_dnormal53"] = kdev[:, 0].astype(np.float32), kdev[:, 4:7].astype(np.float32)
    m = c["kd_hit"] & ~c["kd_fragile"][c["kd_idx"]]
    c["dev53"] = np.maximum(c["dev53"], _largest(kdev[m], c["kd_t"][m], c["kd_point"][m]))
    c["q1"] = col("q1", np.bool_)
    q = [r for r in rows if r["q1"]]
    qcol = lambda key, dt, w: np.array([r["alt"][key] for r in q], dtype=dt).reshape((len(q),) + w)
    c["alt_hit"], c["alt_t"], c["alt_node"], c["alt_sub"] = qcol("hit", np.bool_, ()), qcol("t", np.float64, ()), qcol("node", np.int32, ()), qcol("sub", np.int32, ())
    c["alt_point"], c["alt_normal"] = qcol("point", np.float64, (3,)), qcol("normal", np.float64, (3,))
    c["t_max"] = np.array([r["t_max"] for r in rows], dtype=np.float64).reshape(n, 2)
    c["below_hit"], c["below_t"], c["below_node"], c["below_sub"] = (col("hit", np.bool_, "below"), col("t", np.float64, "below"), col("node", np.int32, "below"),
                                                                     col("sub", np.int32, "below"))
    c["below_point"], c["below_normal"] = col("point", np.float64, "below").reshape(n, 3), col("normal", np.float64, "below").reshape(n, 3)
    c["segment_fragile"] = np.array([r["segment_margin"] < FRAGILE for r in rows])
    return c


FLAGS = ("hit", "fragile", "hier_fragile", "hier_hit", "hit53", "q1", "below_hit", "segment_fragile", "kd_fragile", "kd_segment_fragile")
IDS = ("node", "sub", "part", "hier_node", "hier_sub", "node53", "below_node", "below_sub")
SPARSE = ("alt", "kd", "kd_below", "kd_above")     # rows of (index, hit, node, sub, t, point, normal[, dt53, dnormal53])
TREE = ("kind", "axis", "front", "back", "first", "count")


def _packed(c):
    """Few members instead of many small ones (each costs a few hundred bytes in the archive): flags as bits, ids as one matrix, sparse answers as rows."""
    c = dict(c)
    out = {"flags": sum(c.pop(k).astype(np.uint16) << i for i, k in enumerate(FLAGS)).astype(np.uint16)}
    out["ids"] = np.stack([c.pop(k).astype(np.int32) for k in IDS], axis=1)
    out["below"] = np.concatenate([c.pop("below_t")[:, None], c.pop("below_point"), c.pop("below_normal")], axis=1)
    for key in SPARSE:
        idx = np.flatnonzero(out["flags"] >> FLAGS.index("q1") & 1) if key == "alt" else c.pop(key + "_idx")
        m = [idx, c.pop(key + "_hit"), c.pop(key + "_node"), c.pop(key + "_sub"), c.pop(key + "_t")]
        m = [np.asarray(x, dtype=np.float64)[:, None] for x in m] + [c.pop(key + "_point"), c.pop(key + "_normal")]
        if key == "kd":
            m += [c.pop("kd_dt53").astype(np.float64)[:, None], c.pop("kd_dnormal53").astype(np.float64)]
        out[key] = np.concatenate(m, axis=1)
    out["tree"] = np.stack([c.pop("tree_" + k).astype(np.int32) for k in TREE], axis=1)
    out.update(c)
    return out


def _unpacked(z):
    c = dict(z)
    for i, k in enumerate(FLAGS):
        c[k] = (c["flags"] >> i & 1).astype(np.bool_)
    for i, k in enumerate(IDS):
        c[k] = np.ascontiguousarray(c["ids"][:, i]).astype(np.int8 if k == "part" else np.int32)
    c["below_t"], c["below_point"], c["below_normal"] = c["below"][:, 0].copy(), c["below"][:, 1:4].copy(), c["below"][:, 4:7].copy()
    for key in SPARSE:
        m = c.pop(key)
        c[key + "_idx"], c[key + "_hit"], c[key + "_node"], c[key + "_sub"] = m[:, 0].astype(np.int32), m[:, 1] != 0, m[:, 2].astype(np.int32), m[:, 3].astype(np.int32)
        c[key + "_t"], c[key + "_point"], c[key + "_normal"] = m[:, 4].copy(), m[:, 5:8].copy(), m[:, 8:11].copy()
        if key == "kd":
            c["kd_dt53"], c["kd_dnormal53"] = m[:, 11].astype(np.float32), m[:, 12:15].astype(np.float32)
    for i, k in enumerate(TREE):
        c["tree_" + k] = np.ascontiguousarray(c["tree"][:, i])
    for k in ("flags", "ids", "below", "tree"):
        del c[k]
    return c


def npz_bytes(cols):
    """An .npz whose bytes depend on nothing but the arrays: fixed member times, sorted names."""
    cols = _packed(cols)
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(cols):
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(cols[name]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, member.getvalue(), compresslevel=9)
    return buf.getvalue()


def path(scene, batch):
    return os.path.join(OUT, "%s_%s.npz" % (scene, batch))


def load(scene, batch):
    with np.load(path(scene, batch)) as z:
        return _unpacked({k: z[k] for k in z.files})


def scene_inputs(name):
    """(scene, flattened f64 matrices, primitives, kinds) - the matrices from the oracle's flatten, as the issue's inputs are defined."""
    import oracle_lib
    scene = build_scene(name)
    flat = oracle_lib.flatten(oracle_lib.pack(scene))
    prims = flat_prims(scene)
    assert [p.kind for p in prims] == [int(k) for k in flat["prim_type"]]
    flat["kd_tree"] = oracle_lib.kd_scene_dump(oracle_lib.pack(scene), kd_depth=KD_DEPTH)
    return scene, flat["trans"], prims, flat


def make_batch(name, batch, workers, ex=None, inputs=None):
    import exact_ref
    scene, trans, prims, flat = inputs or scene_inputs(name)
    if ex is None:
        ex = exact_ref.ExactScene(scene, trans, flat["prim_type"])
        ex.set_tree(flat["kd_tree"])
    seed = [17, SCENES.index(name), [b for b, _ in BATCHES].index(batch) if batch != "camera" else 9]
    extra = {}
    if batch == "camera":
        cam = scene_camera(trans, prims)
        ys, xs = np.mgrid[0:CAM_H, 0:CAM_W]
        xy = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float64)
        eye, dirs = exact_ref.camera_rays(cam, CAM_W, CAM_H, xy)
        eye53, dirs53 = exact_ref.camera_rays(cam, CAM_W, CAM_H, xy, prec=53)
        f = lambda v: [float(x) for x in v]
        o, d = np.array([f(eye)] * len(xy)), np.array([f(v) for v in dirs])
        rays = [(o[k], (dirs[k], dirs53[k])) for k in range(len(xy))]
        extra = dict(cam=np.array([*cam.eye, *cam.center, *cam.up, cam.fovy_radians], dtype=np.float64), xy=xy)
    else:
        n = dict(BATCHES)[batch]
        m = n + n // 2
        if batch == "random":
            o, d = batch_random(seed, m, trans, prims)
        elif batch == "near":
            o, d = batch_near(seed, m, trans, prims)
        else:
            o, d = batch_special(seed, m, trans, prims, load(name, "random"))
        rays = [(o[k], d[k]) for k in range(m)]
    rows = evaluate(ex, rays, workers)
    if batch != "camera":   # draw half as many rays again, and keep the first n that are well conditioned
        keep = [k for k in range(len(rows)) if well_conditioned(rows[k])]
        extra["replaced"] = np.array([sum(1 for k in range(keep[n - 1]) if k not in set(keep))], dtype=np.int32)
        keep = keep[:n]
        o, d, rows = o[keep], d[keep], [rows[k] for k in keep]
    cols = columns(o, d, rows)
    cols.update(extra)
    cols["trans"] = np.ascontiguousarray(trans, dtype=np.float64)
    cols["prim_type"] = np.ascontiguousarray(flat["prim_type"], dtype=np.int32)
    for k, v in flat["kd_tree"].items():
        cols["tree_" + k] = np.ascontiguousarray(v)
    return cols


# ---------------------------------------------------------------- conditions and tolerances (numpy only)
def deviations(c):
    """Largest deviation of the 53-bit evaluation from the 256-bit one over the non-fragile hits: (t, point, normal)."""
    m = c["hit"] & ~c["fragile"]
    assert np.array_equal(c["hit53"][~c["fragile"]], c["hit"][~c["fragile"]]) and np.array_equal(c["node53"][m], c["node"][m]), \
        "the 53-bit evaluation decides a non-fragile ray differently"
    return tuple(float(x) for x in c["dev53"])


def tolerances(batches):
    """batches: {scene: {batch: columns}} -> {scene: {quantity: {"deviation", "threshold"}}}."""
    out = {}
    for scene, bs in batches.items():
        dev = np.max([deviations(c) for c in bs.values()], axis=0)
        out[scene] = {q: {"deviation": float(v), "threshold": float(SLACK * v)} for q, v in zip(("t", "point", "normal"), dev)}
        for q, v in out[scene].items():
            assert 0.0 < v["threshold"] < THRESHOLD_CAP, "%s %s: threshold %g is not below 2^-32: the batch is badly conditioned" % (scene, q, v["threshold"])
    return out


def shares(c):
    n = len(c["hit"])
    return dict(rays=n, fragile=float(c["fragile"].mean()), hit=float(c["hit"].mean()), q1=float(c["q1"].mean()), kd_fragile=float(c["kd_fragile"].mean()),
                kd_differs=len(c["kd_idx"]) / n)


def check_conditions(scene, bs, log=print):
    """bs: {batch: columns} of one scene. The caps of the issue, asserted from the exact reference's columns alone."""
    kinds = bs["random"]["prim_type"]
    total = q1 = 0
    for batch, c in bs.items():
        s = shares(c)
        log("%-9s %-8s rays %4d  fragile %.4f  hit %.3f  q1 %.4f" % (scene, batch, s["rays"], s["fragile"], s["hit"], s["q1"]))
        assert s["fragile"] <= FRAGILE_CAP[batch], (scene, batch, "fragile share", s["fragile"])
        assert batch == "camera" or s["hit"] >= HIT_SHARE, (scene, batch, "hit share", s["hit"])
        ok = ~c["fragile"]
        assert np.array_equal(c["hier_hit"][ok & ~c["hier_fragile"]], c["hit"][ok & ~c["hier_fragile"]]), (scene, batch, "hierarchical hit differs")
        both = ok & ~c["hier_fragile"] & c["hit"]
        assert np.array_equal(c["hier_node"][both], c["node"][both]) and np.array_equal(c["hier_sub"][both], c["sub"][both]), (scene, batch, "hierarchical node differs")
        assert np.all(np.abs(c["hier_dt"][both]) <= 2.0 ** -40 * np.maximum(1.0, np.abs(c["t"][both]))), (scene, batch, "hierarchical t differs")
        total += s["rays"]; q1 += int(c["q1"].sum())
    if any(int(k) in (CONE, CYLINDER) for k in kinds):
        assert q1 <= Q1_CAP * total, (scene, "Q1 exposure", q1, total)
    node = np.concatenate([c["node"][c["hit"] & ~c["fragile"]] for c in bs.values()])
    part = np.concatenate([c["part"][c["hit"] & ~c["fragile"]] for c in bs.values()])
    kind = np.asarray(kinds)[node]
    for k in sorted(set(int(x) for x in kinds)):
        assert int((kind == k).sum()) >= KIND_MIN, (scene, KIND_NAME[k], "nearest hit of", int((kind == k).sum()))
        for p in PARTS.get(k, (0, 1) if k == TRIANGLE else ()):
            assert int(((kind == k) & (part == p)).sum()) >= PART_MIN, (scene, KIND_NAME[k], "part", p, int(((kind == k) & (part == p)).sum()))
    if scene == "tris":   # flat and smooth triangles, as primitives and inside meshes
        for k in (TRIANGLE, MESH):
            for p in (0, 1):
                assert int(((kind == k) & (part == p)).sum()) >= PART_MIN, (scene, KIND_NAME[k], "shading", p)


# ---------------------------------------------------------------- what the tests compare with (numpy only)
def load_tolerances():
    with open(os.path.join(OUT, "tolerances.json")) as fh:
        return json.load(fh)["scenes"]


def expected(c, which="nearest"):
    """The exact answer of a batch as full-length arrays: "nearest", the Q1 "alt"ernative (the nearest hit where a ray is not exposed), the nearest hit
    "below" the lower of the two bounds in c["t_max"], or what the k-d tree walk answers: "kd", "kd_below", "kd_above" (the upper bound)."""
    keys = ("hit", "t", "node", "sub", "point", "normal")
    if which in ("below", "kd_below"):
        e = {k: c["below_" + k].copy() for k in keys}
    else:
        e = {k: c[k].copy() for k in keys}
    if which == "alt":
        q = np.flatnonzero(c["q1"])
        for k in e:
            e[k][q] = c["alt_" + k]
    elif which.startswith("kd"):
        for k in e:
            e[k][c[which + "_idx"]] = c[which + "_" + k]
    return e


def agreement(exp, got, tol):
    """Per ray: does `got` (hit, t, point, normal and, where present, node and sub) agree with the exact answer `exp` within the scene's thresholds `tol`?
    hit, node and sub exactly; t and point relative to max(1, magnitude); the unit normal by Euclidean distance."""
    ok = exp["hit"] == got["hit"]
    h = exp["hit"] & got["hit"]
    with np.errstate(all="ignore"):
        good = np.abs(got["t"] - exp["t"]) <= tol["t"]["threshold"] * np.maximum(1.0, np.abs(exp["t"]))
        good &= np.linalg.norm(got["point"] - exp["point"], axis=1) <= tol["point"]["threshold"] * np.maximum(1.0, np.linalg.norm(exp["point"], axis=1))
        good &= np.linalg.norm(got["normal"] - exp["normal"], axis=1) <= tol["normal"]["threshold"]
    for k in ("node", "sub"):
        if k in got:
            good &= got[k] == exp[k]
    return ok & (good | ~h)


def first_disagreement(exp, got, bad):
    k = int(np.flatnonzero(bad)[0])
    return "ray %d: exact %s, got %s" % (k, {q: exp[q][k].tolist() for q in exp}, {q: got[q][k].tolist() for q in got})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--workers", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--scenes", default=",".join(SCENES))
    a = ap.parse_args()
    if a.check:
        scene, batch = CHECK_BATCH
        same = npz_bytes(make_batch(scene, batch, a.workers)) == open(path(scene, batch), "rb").read()
        print("%s_%s regenerated: %s" % (scene, batch, "byte-identical" if same else "DIFFERENT"))
        assert same
        allb = {s: {b: load(s, b) for b in [x for x, _ in BATCHES] + ["camera"]} for s in SCENES}
        for s in SCENES:
            check_conditions(s, allb[s])
        tol = tolerances(allb)
        assert tol == json.load(open(os.path.join(OUT, "tolerances.json")))["scenes"], "tolerances.json is stale"
        for s in SCENES:
            print(s, {q: "%.3g" % v["threshold"] for q, v in tol[s].items()})
        return
    import exact_ref
    os.makedirs(OUT, exist_ok=True)
    for name in a.scenes.split(","):
        inputs = scene_inputs(name)
        ex = exact_ref.ExactScene(inputs[0], inputs[1], inputs[3]["prim_type"])
        ex.set_tree(inputs[3]["kd_tree"])
        bs = {}
        for batch in [b for b, _ in BATCHES] + ["camera"]:
            bs[batch] = make_batch(name, batch, a.workers, ex, inputs)
            with open(path(name, batch), "wb") as fh:
                fh.write(npz_bytes(bs[batch]))
            print(name, batch, shares(bs[batch]), os.path.getsize(path(name, batch)), flush=True)
        check_conditions(name, bs)
    allb = {s: {b: load(s, b) for b in [x for x, _ in BATCHES] + ["camera"]} for s in SCENES if os.path.exists(path(s, "camera"))}
    tol = tolerances(allb)
    with open(os.path.join(OUT, "tolerances.json"), "w") as fh:
        json.dump({"fragile_margin": FRAGILE, "slack": SLACK, "threshold_cap": THRESHOLD_CAP, "scenes": tol}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(tol, indent=1))


if __name__ == "__main__":
    main()
