#!/usr/bin/env python3
"""Generates tests/golden/exact_kdmesh/: KDMesh scenes, ray batches and the exact reference's answers for them (tests/exact_ref.py, whose KDMesh trees
are the independent build of tests/exact_kd.py), and the comparison of that build with the committed scene trees.

    python tools/gen_exact_kdmesh.py            # regenerate every file (minutes; deterministic, byte for byte)
    python tools/gen_exact_kdmesh.py --check    # regenerate one batch and compare its bytes, re-assert the conditions, print the counts

A sibling of tools/gen_exact_rays.py: its column layout, its evaluation of a ray, its fragility margin (2^-30), factor (64), threshold cap (2^-32) and
caps on the fragile shares are used unchanged, and its fixtures in tests/golden/exact/ are read, never written. The scene builders and the conditions need
only numpy and tests/scene_dsl.py, so the tests import them from here; mpmath is needed to evaluate."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_exact_rays as G  # noqa: E402
from scene_dsl import (ASSETS, KDMESH, MESH, Camera, Cone, Cube, Cylinder, KDMesh, Mesh, MeshData, Node, Plane, Scene, Sphere)  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "exact_kdmesh")
SCENES = ("kdm_far", "kdm_near", "kdm_nested", "kdm_grid")      # with rays
BUILD_ONLY = ("scatter40",)                                      # the scene build alone
BATCHES = G.BATCHES
BATCH_NAMES = tuple(b for b, _ in BATCHES) + ("camera",)
KD_DEPTH = G.KD_DEPTH                                            # the scene tree of the ray scenes; KD_MESH_DEPTH is the default (10)
SCATTER_DEPTH = 10                                               # KD_DEPTH's default, for scatter40
CHECK_BATCH = ("kdm_grid", "special")
MIN_DIFFER = MIN_ALIKE = 100
MIN_TRIANGLES = MIN_FAR = 20
KDM_FLAGS = ("far", "panic", "mesh_decidable", "mesh_differs", "mesh_alike")
# A mutant that cannot change an answer. Every triangle lies inside its tree's root box, so BoundingBox::test_hit can only turn away rays that would hit
# nothing, and a hit's parameter is never below the box's: leaving the test out changes which comparisons are made (what is fragile), never what is hit.
EQUIVALENT_MUTANTS = ("root_box_skipped",)


# ---------------------------------------------------------------- scenes
def _scaled(data, factor, name):
    """The mesh's vertices times a power of two (exact in f64): KDMesh's extent is a property of the DATA, whatever the node's matrix."""
    assert math.frexp(factor)[0] == 0.5
    out = MeshData(data.positions * factor, data.triangles.copy(), None if data.normals is None else data.normals.copy(), name)
    out.unit = factor   # for as_meshes
    return out


def grid_mesh():
    """An 8 x 8 grid of quads in the plane y = 0 with vertices at the integers 0..8, and a second copy at y = 1: 256 triangles, every box of zero
    thickness, every centre plane and most retried planes exactly on vertex coordinates."""
    pos, tris = [], []
    for y in (0.0, 1.0):
        base = len(pos)
        pos += [(float(x), y, float(z)) for z in range(9) for x in range(9)]
        for z in range(8):
            for x in range(8):
                a, b, c, d = base + 9 * z + x, base + 9 * z + x + 1, base + 9 * (z + 1) + x + 1, base + 9 * (z + 1) + x
                tris += [(a, c, b), (a, d, c)]
    return MeshData(np.array(pos, dtype=np.float64), np.array(tris, dtype=np.uint32), None, "grid")


def scene_kdm_far(kd=True):
    prim = KDMesh if kd else Mesh
    bucky = _scaled(MeshData.load_obj(os.path.join(ASSETS, "buckyball.obj")), 2.0 ** -4, "buckyball/16")   # diagonal^2 = 0.28
    n = Node.geo(prim(bucky), G._material(0)).scaled((1.5, 1.25, 1.75)).rotated_xzy((0.3, -0.8, 0.5)).translated((0.25, -0.5, 0.125))
    return Scene(Node.group([n]), [], (0.1, 0.1, 0.1))


def scene_kdm_near(kd=True):
    prim = KDMesh if kd else Mesh
    # The fish's data is turned before it is scaled (by rotations with rational entries, 3-4-5 about z and then 5-12-13 about x, so that the vertices are
    # the same f64 numbers on every machine). As the file has it, the fish has a flat side: 92 triangles in a plane x = c, whose vertices differ in the
    # last place of the f32 they were parsed as. Where a list holds such triangles alone it is split AT their coordinate, so a hit there ties with the
    # end of the clipped range (as everywhere in kdm_grid); and planes fall 1e-8 before that side, inside the last EPSILON of a clipped range, where
    # the walk does not look (node.rs:122), so some hits there are lost at any extent. With the axis-aligned data a fifth of the hits on that side were
    # ties and 10 decidable rays of 2,752 differed from Mesh, whatever the scale. Scaled by 32, the squared diagonal is 3.1e4;
    # the nodes are 20 units long in the world, since the last EPSILON of a range is EPSILON |d| long and |d| goes up to 100.
    rz = np.array([[0.6, -0.8, 0.0], [0.8, 0.6, 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, 5.0 / 13.0, -12.0 / 13.0], [0.0, 12.0 / 13.0, 5.0 / 13.0]])
    raw = MeshData.load_obj(os.path.join(ASSETS, "fish.obj"))
    turn = lambda v: np.array([[sum(float((rx @ rz)[r][q]) * float(p[q]) for q in range(3)) for r in range(3)] for p in v], dtype=np.float64)
    fish = _scaled(MeshData(turn(raw.positions), raw.triangles, turn(raw.normals), "fish turned"), 32.0, "fish turned*32")
    dodeca = _scaled(MeshData.load_obj(os.path.join(ASSETS, "dodeca.obj")), 32.0, "dodeca*32")   # 3.2e4
    c = fish.positions.min(axis=0) / 2 + fish.positions.max(axis=0) / 2
    a = Node.geo(prim(fish, smooth=True), G._material(0)).translated(tuple(-np.round(c))).scaled(1.0 / 8).rotated_xzy((0.2, 1.1, -0.4)).translated((-4.0, 2.0, 0.0))
    b = Node.geo(prim(dodeca), G._material(1)).scaled((0.08, 0.1, 0.12)).rotated_xzy((-0.7, 0.3, 0.9)).translated((10.0, -2.0, 4.0))
    return Scene(Node.group([a, b]), [], (0.1, 0.1, 0.1))


def scene_kdm_nested(kd=True):
    prim = KDMesh if kd else Mesh
    bucky = MeshData.load_obj(os.path.join(ASSETS, "buckyball.obj"))                             # diagonal^2 = 70.7
    rng = np.random.default_rng(2601)
    ang = lambda: tuple(rng.uniform(-math.pi, math.pi, 3))
    k1 = Node.geo(prim(bucky), G._material(0)).scaled((0.5, 0.4, 0.6)).rotated_xzy(ang()).translated((1.5, 0.5, -1.0))
    k2 = Node.geo(prim(bucky, smooth=True), G._material(1)).scaled((0.45, 0.6, 0.35)).rotated_xzy(ang()).translated((-1.0, -0.5, 1.5))
    plain = Node.geo(Mesh(bucky), G._material(2)).scaled((0.4, 0.4, 0.5)).rotated_xzy(ang()).translated((-2.5, 1.0, -1.5))
    sphere = Node.geo(Sphere(), G._material(3)).scaled((0.8, 0.6, 0.7)).translated((0.0, 2.0, 0.5))
    cube = Node.geo(Cube(), G._material(4)).scaled((1.2, 0.8, 1.0)).rotated_xzy(ang()).translated((2.0, -2.0, 1.0))
    cyl = Node.geo(Cylinder(), G._material(5)).scaled((0.9, 1.6, 0.9)).rotated_xzy(ang()).translated((-2.0, -2.0, -0.5))
    g2 = Node.group([k2, cube]).scaled((-1.2, 0.75, 1.1)).rotated_xzy(ang()).translated((0.5, 0.25, -0.5))   # mirroring: negative determinant
    g1 = Node.group([k1, sphere, g2]).scaled((1.25, 0.9, 0.7)).rotated_xzy(ang()).translated((0.25, -0.25, 0.5))
    return Scene(Node.group([g1, plain, cyl]), [], (0.1, 0.1, 0.1))


def scene_kdm_grid(kd=True):
    prim = KDMesh if kd else Mesh
    # a power of two and integers: the node's matrix and its inverse are exact, so an origin chosen on a split plane in model space is on it
    n = Node.geo(prim(grid_mesh()), G._material(0)).scaled(0.5).translated((-2.0, 0.0, -2.0))
    return Scene(Node.group([n]), [], (0.1, 0.1, 0.1))


def scene_scatter40():
    rng = np.random.default_rng(4003)
    nodes = []
    for k in range(40):
        p = (Sphere, Cube, Plane, Cylinder, Cone)[k % 5]()
        n = Node.geo(p, G._material(k)).scaled(tuple(rng.uniform(0.3, 1.2, 3))).rotated_xzy(tuple(rng.uniform(-math.pi, math.pi, 3)))
        nodes.append(n.translated(tuple(rng.uniform(-6.0, 6.0, 3))))
    return Scene(Node.group(nodes), [], (0.1, 0.1, 0.1))


_BUILDERS = {"kdm_far": scene_kdm_far, "kdm_near": scene_kdm_near, "kdm_nested": scene_kdm_nested, "kdm_grid": scene_kdm_grid}


def build_scene(name, kd=True):
    if name == "scatter40":
        return scene_scatter40()
    return _BUILDERS[name](kd) if name in _BUILDERS else G.build_scene(name)


def as_meshes(prims, trans):
    """(primitives, matrices) for gen_exact_rays' ray makers: every KDMesh as a Mesh, and a mesh whose data was scaled (_scaled) as the unscaled data under
    a matrix that scales it back - the same surface in the world - so that the makers' model-space offsets (2^-24 to 2^-6) keep their meaning."""
    view, vt = [], np.array(trans, dtype=np.float64)
    for i, p in enumerate(prims):
        if p.kind in (KDMESH, MESH):
            k = getattr(p.mesh, "unit", 1.0)
            m = MeshData(p.mesh.positions / k, p.mesh.triangles, p.mesh.normals, p.mesh.name)
            vt[i] = trans[i] @ np.diag([k, k, k, 1.0])
            p = Mesh(m, p.smooth)
        view.append(p)
    return view, vt


def meshes_by_first_use(prims):
    """(mesh index per primitive or -1, the distinct MeshData) in the order the host numbers them: first use among the flattened nodes."""
    ids, meshes = [], []
    for p in prims:
        if p.kind in (MESH, KDMESH):
            if not any(p.mesh is m for m in meshes):
                meshes.append(p.mesh)
            ids.append([p.mesh is m for m in meshes].index(True))
        else:
            ids.append(-1)
    return ids, meshes


# ---------------------------------------------------------------- rays
def _length(rng, v):
    return v / np.linalg.norm(v) * 2.0 ** rng.uniform(-6.0, 6.0)


def batch_special(seed, n, trans, prims):
    """Origins inside a tree's root box, origins exactly on a split plane (model space; exact in the world where the node's matrix is), directions with a
    zero component, rays that graze a root box, rays inside a split plane; every direction 2^-6 to 2^6 long."""
    import exact_kd
    rng = np.random.default_rng(seed)
    kdm = [i for i, p in enumerate(prims) if p.kind == KDMESH]
    trees = {i: exact_kd.mesh_tree(prims[i].mesh) for i in kdm}
    o, d = [], []

    def emit(i, om, dm):
        o.append(G._to_world(trans[i], om)); d.append(trans[i][:3, :3] @ dm)

    def box(i):
        rb = np.array(trees[i]["root_bounds"])
        return rb[:3], rb[3:]

    def split(i):
        t = trees[i]
        s = [k for k, kind in enumerate(t["kind"]) if kind == 0]
        k = s[int(rng.integers(len(s)))]
        return t["axis"][k], t["plane"][k]

    def touching(i):
        """(split node's axis, plane, triangle): triangles that are in front of a split only, with a vertex ON its plane (a list whose boxes begin at
        one coordinate is split there)."""
        t, m = trees[i], prims[i].mesh
        bx = exact_kd.triangle_boxes(m.positions, m.triangles)

        def items(me):
            if t["kind"][me] == 1:
                return set(t["items"][t["first"][me]:t["first"][me] + t["count"][me]])
            return items(t["front"][me]) | items(t["back"][me])
        return [(t["axis"][me], t["plane"][me], j) for me, kind in enumerate(t["kind"]) if kind == 0
                for j in sorted(items(t["front"][me]) - items(t["back"][me])) if bx[j][0][t["axis"][me]] == t["plane"][me]]
    touch = {i: touching(i) for i in kdm}
    fixed_length = False
    for k in range(n):
        i = kdm[int(rng.integers(len(kdm)))]
        lo, hi = box(i)
        c, e = (lo + hi) / 2, np.maximum((hi - lo) / 2, 0.125)
        kind = k % 16
        if kind == 3 and touch[i]:
            # the start of the range: the ray starts 1.3 EPSILON before such a triangle, next to its vertex on the plane, and crosses the plane at
            # 1.6 EPSILON. The walk classifies the start at t_min = start + EPSILON = 2 EPSILON, already behind the plane, so it never asks the front.
            ax, pl, j = touch[i][int(rng.integers(len(touch[i])))]
            m = prims[i].mesh
            v = [m.positions[int(q)] for q in m.triangles[j]]
            v0 = min(v, key=lambda p: p[ax])
            cen = (v[0] + v[1] + v[2]) / 3
            nrm = np.cross(v[1] - v[0], v[2] - v[0])
            speed = 24.0 / np.linalg.norm(trans[i][:3, ax])          # model units per unit of t across the plane: about 24 in the world
            q = v0 + (cen - v0) * (speed * 0.3e-5 / (cen[ax] - v0[ax]))
            dm = G._unit(rng) * 0.3
            dm[ax] = -1.0
            if abs(dm @ nrm) < 0.3 * np.linalg.norm(nrm) * np.linalg.norm(dm):   # not along the triangle
                dm = dm + 0.5 * nrm / np.linalg.norm(nrm) * np.sign(dm @ nrm or 1.0)
                dm = dm / -dm[ax]
            dm = dm * speed
            emit(i, q - dm * 1.3e-5, dm)
            fixed_length = True
        elif kind < 4:      # inside the root box
            emit(i, c + e * rng.uniform(-0.95, 0.95, 3) * (hi > lo), G._unit(rng))
        elif kind < 8:      # on a split plane, inside or outside the box; the ray leaves the plane
            ax, pl = split(i)
            om = c + e * rng.uniform(-1.5, 1.5, 3)
            om[ax] = pl
            emit(i, om, G._unit(rng) if kind % 2 else c + e * rng.uniform(-0.5, 0.5, 3) - om)
        elif kind < 11:     # a zero component of either sign, in model space (kind 8) or in the world
            target = c + e * rng.uniform(-0.8, 0.8, 3)
            v = G._unit(rng)
            zero = rng.choice(3, size=int(rng.integers(1, 3)), replace=False)
            v[zero] = rng.choice([0.0, -0.0], size=len(zero))
            if kind == 8:
                emit(i, target - v * rng.uniform(1.0, 4.0) * np.linalg.norm(e), v)
            else:
                w = G._to_world(trans[i], target)
                o.append(w - v * rng.uniform(1.0, 4.0) * np.linalg.norm(trans[i][:3, :3] @ e)); d.append(v)
        elif kind < 15:     # grazing the root box: at an edge or a corner, displaced along its diagonal by 2^-24 to 2^-6
            s = rng.choice([-1.0, 1.0], size=3)
            p, u = np.where(s > 0, hi, lo).astype(np.float64), s.copy()
            if rng.random() < 0.6:
                ax = int(rng.integers(3))
                p[ax], u[ax] = c[ax] + e[ax] * rng.uniform(-0.9, 0.9), 0.0
            u /= np.linalg.norm(u)
            om = c + G._unit(rng) * rng.uniform(1.5, 4.0) * np.linalg.norm(e)
            emit(i, om, p + rng.choice([-1.0, 1.0]) * 2.0 ** rng.uniform(-24.0, -6.0) * getattr(prims[i].mesh, "unit", 1.0) * u - om)
        else:               # inside a split plane: on it, with no component across it (a tie at every which_side: never decidable, counted as fragile)
            ax, pl = split(i)
            om = c + e * rng.uniform(-1.5, 1.5, 3)
            om[ax] = pl
            v = G._unit(rng)
            v[ax] = 0.0
            emit(i, om, v)
        if fixed_length:
            fixed_length = False
            assert 2.0 ** -6 <= np.linalg.norm(d[-1]) <= 2.0 ** 6
        else:
            d[-1] = _length(rng, d[-1])
    o, d = np.array(o), np.array(d)
    p = rng.permutation(n)
    return o[p], d[p]


# ---- kdm_grid: its triangles lie IN split planes of their own tree (a list of boxes of zero thickness is split at its own coordinate, ten times over),
# so a ray whose segment crosses a sheet inside the grid's outline meets its hit exactly at the end of the clipped range: a tie, never decidable, in
# the reference a matter of the last bit. What is decidable there: misses outside the outline, rays that cross no sheet, and hits whose parameter
# exceeds the extent (129), where the segment ends before the sheet, no y split clips, and Q3 decides by the origin's column which triangles are tried.
GRID_EXTENT = 129.0


def _grid_clear(om, dm):
    """Does the ray keep clear of both sheets inside the outline (0..8 squared, with a margin)?"""
    for y in (0.0, 1.0):
        if dm[1] == 0.0:
            if om[1] == y:
                return False
            continue
        t = (y - om[1]) / dm[1]
        if t > 0.0:
            x, z = om[0] + t * dm[0], om[2] + t * dm[2]
            if -0.01 <= x <= 8.01 and -0.01 <= z <= 8.01:
                return False
    return True


def _grid_drop(rng, feature=False, cross=False, axial=False):
    """A ray that falls (or rises) onto a sheet with a parameter of 200 to 400 at the hit: (model origin, model direction). feature: the target is 2^-24
    to 2^-6 off a grid line or a cell's diagonal. cross: the origin is just before the plane x = 4 or z = 4 and drifts across it early, so the hit is found
    on a pending far side. axial: no drift at all - two components of the direction are zeros of either sign."""
    cell = rng.integers(0, 8, size=2)
    u = rng.uniform(0.2, 0.8, size=2)
    if abs(u[0] - u[1]) < 0.1:       # keep off the diagonal x - x0 = z - z0
        u[1] = (u[1] + 0.3) % 0.6 + 0.2 if abs((u[1] + 0.3) % 0.6 + 0.2 - u[0]) >= 0.1 else 0.95 - u[0] * 0.5
    if feature:
        off = rng.choice([-1.0, 1.0]) * 2.0 ** rng.uniform(-24.0, -6.0)
        which = int(rng.integers(3))
        if which == 0:
            u[0] = off if off > 0 else 1.0 + off
        elif which == 1:
            u[1] = off if off > 0 else 1.0 + off
        else:
            u[1] = min(max(u[0] + off, 2.0 ** -7), 1.0 - 2.0 ** -7)
    target = np.array([cell[0] + u[0], float(rng.integers(2)), cell[1] + u[1]])
    side = rng.choice([-1.0, 1.0])
    if side < 0 and target[1] == 1.0 or side > 0 and target[1] == 0.0:   # the other sheet would be met first: aim at that one
        target[1] = 1.0 - target[1]
    om = target + np.array([rng.uniform(-0.04, 0.04), side * rng.uniform(12.0, 30.0), rng.uniform(-0.04, 0.04)])
    if axial:
        om[0], om[2] = target[0], target[2]
    if cross:
        ax = 0 if rng.random() < 0.5 else 2
        target[ax] = 4.0 + rng.uniform(0.15, 0.8)
        om[ax] = 4.0 - rng.uniform(0.005, 0.035)
    dm = (target - om) / rng.uniform(200.0, 400.0)
    if axial:
        dm[0], dm[2] = rng.choice([0.0, -0.0], size=2)
    return om, dm


def _grid_miss(rng, level=False, inside=False, on_plane=None):
    """A ray that keeps clear of the sheets inside the outline, of any length: level (no y component, a zero of either sign), from inside the root box, or
    from a point of a split plane (axis, coordinate)."""
    for _ in range(1000):
        if inside:
            om = np.array([rng.uniform(0.1, 7.9), rng.uniform(0.05, 0.95), rng.uniform(0.1, 7.9)])
        else:
            om = np.array([4.0, 0.5, 4.0]) + G._unit(rng) * rng.uniform(7.0, 16.0)
        if on_plane is not None:
            om[on_plane[0]] = on_plane[1]
        dm = G._unit(rng) if rng.random() < 0.5 else np.array([rng.uniform(-2.0, 10.0), rng.uniform(-1.0, 2.0), rng.uniform(-2.0, 10.0)]) - om
        if level:
            dm[1] = rng.choice([0.0, -0.0])
        if np.linalg.norm(dm) > 0 and _grid_clear(om, dm):
            return om, dm * 2.0 ** rng.uniform(-6.0, 6.0) / np.linalg.norm(dm)
    raise AssertionError("no clear ray found")


def batch_grid(seed, n, trans, prims, batch):
    import exact_kd
    rng = np.random.default_rng(seed)
    tree = exact_kd.mesh_tree(prims[0].mesh)
    splits = [(tree["axis"][k], tree["plane"][k]) for k, kind in enumerate(tree["kind"]) if kind == 0]
    o, d = [], []
    for k in range(n):
        c = k % 16
        if batch == "random":
            om, dm = _grid_drop(rng, cross=c % 3 == 0) if c < 10 else _grid_miss(rng, inside=c == 15)
        elif batch == "near":
            om, dm = _grid_drop(rng, feature=True, cross=c < 4)
        elif c < 3:                                       # special: inside the root box
            om, dm = _grid_miss(rng, inside=True)
        elif c < 6:                                       # on a split plane
            om, dm = _grid_miss(rng, inside=c == 3, on_plane=splits[int(rng.integers(len(splits)))])
        elif c < 8:                                       # a drop, a drop with crossing
            om, dm = _grid_drop(rng, cross=c == 7)
        elif c == 8:                                      # zero components: two in a drop, one in a level ray. This node's matrix keeps them zeros in model
            om, dm = _grid_drop(rng, axial=True) if k % 32 < 16 else _grid_miss(rng, level=True)   # space, where the root box's faces divide by them:
        elif c < 11:                                      # the sign of a zero decides there, which the exact reference does not represent (margin 0)
            om, dm = _grid_miss(rng)
        elif c < 14:                                      # grazing the root box: past an upper or lower edge of it, 2^-24 to 2^-6 outside
            ax, far_side = (0, 2)[int(rng.integers(2))], int(rng.integers(2))
            p = np.array([rng.uniform(0.5, 7.5), float(rng.integers(2)), rng.uniform(0.5, 7.5)])
            p[ax] = 8.0 + 2.0 ** rng.uniform(-24.0, -6.0) if far_side else -2.0 ** rng.uniform(-24.0, -6.0)
            om = p + np.array([0.0, (1.0 if p[1] == 1.0 else -1.0) * rng.uniform(3.0, 9.0), 0.0])
            om[ax] += (-1.0 if far_side else 1.0) * rng.uniform(0.5, 3.0)   # from over the grid outwards: the other sheet's plane is met further out
            om[2 - ax] += rng.uniform(-0.5, 0.5)
            dm = (p - om) / np.linalg.norm(p - om) * 2.0 ** rng.uniform(-6.0, 6.0)
        elif c == 14:                                     # a drop with crossing
            om, dm = _grid_drop(rng, cross=True)
        elif k % 32 < 16:
            om, dm = _grid_drop(rng)
        else:                                             # the tie itself: from between the sheets onto one; never decidable, counted as fragile
            om = np.array([rng.uniform(0.5, 7.5), rng.uniform(0.2, 0.8), rng.uniform(0.5, 7.5)])
            dm = np.array([rng.uniform(-0.2, 0.2), rng.choice([-1.0, 1.0]), rng.uniform(-0.2, 0.2)]) * 2.0 ** rng.uniform(-6.0, 6.0)
        o.append(G._to_world(trans[0], om)); d.append(trans[0][:3, :3] @ dm)
    o, d = np.array(o), np.array(d)
    p = rng.permutation(n)
    return o[p], d[p]


# ---------------------------------------------------------------- evaluation
_EXM = None


def _evaluate(k):
    """gen_exact_rays._evaluate, with one difference: a bound just above the hit MAY change a KDMesh's answer (the walk's segment then ends at the bound
    instead of at start + extent, so other sides of its splits are visited), so the flat walk's answer for the upper bound is recorded like the k-d
    walk's, not asserted to be the nearest hit. Added: the far-side, panic and Mesh-equivalence flags."""
    import exact_ref
    ex, row, same = G._EX, G._row, G._identical
    before = exact_ref.PANICS[0]
    o, d = G._RAYS[k]
    d53 = d
    if isinstance(d, tuple):   # a camera ray: (direction at 256 bits, direction at 53 bits)
        d, d53 = d
    h = ex.cast(o, d)
    r = row(h)
    hh = ex.cast(o, d, mode="hier")
    r["hier"], r["hier_margin"] = row(hh), hh.margin
    h53 = ex.cast(o, d53, prec=53)
    r["f53"] = row(h53)
    r["dev"] = G._deviation(h53, h) or [0.0] * 7
    kd = ex.cast(o, d, mode="kd")
    r["kd"], r["kd_margin"], r["kd_differs"] = row(kd), kd.margin, not same(kd, h)
    r["kd_dev"] = [0.0] * 7
    if r["kd_differs"] and kd:
        r["kd_dev"] = G._deviation(ex.cast(o, d53, mode="kd", prec=53), kd) or [math.inf] * 7
    r["q1"] = bool(h.q1)
    r["alt"] = row(ex.cast(o, d, alt=True)) if h.q1 else None
    if h:
        t = float(h.t)
        r["t_max"] = [t * (1.0 - G.SEGMENT), t * (1.0 + G.SEGMENT)]
    else:
        r["t_max"] = [G.T_MAX_MISS, G.T_MAX_MISS]
    below, above = ex.cast(o, d, t_max=r["t_max"][0]), ex.cast(o, d, t_max=r["t_max"][1])
    r["below"], r["above"], r["above_differs"] = row(below), row(above), not same(above, h)
    r["segment_margin"] = min(below.margin, above.margin)
    kd_below, kd_above = ex.cast(o, d, mode="kd", t_max=r["t_max"][0]), ex.cast(o, d, mode="kd", t_max=r["t_max"][1])
    r["kd_below"], r["kd_below_differs"] = row(kd_below), not same(kd_below, below)
    r["kd_above"], r["kd_above_differs"] = row(kd_above), not same(kd_above, h)
    r["kd_segment_margin"] = min(kd_below.margin, kd_above.margin)
    r["margin"] = h.margin
    r["panic"] = exact_ref.PANICS[0] != before
    r["far"] = bool(h) and bool(h.far)
    m = _EXM.cast(o, d)          # the same scene with every KDMesh as a Mesh
    r["mesh_decidable"] = min(m.margin, h.margin) >= G.FRAGILE
    r["mesh_differs"] = not same(m, h)
    r["mesh_alike"] = bool(m) and bool(h) and same(m, h)
    return r


def evaluate(ex, exm, rays, workers):
    global _EXM
    G._EX, G._RAYS, _EXM = ex, rays, exm
    if workers <= 1:
        return [_evaluate(k) for k in range(len(rays))]
    import multiprocessing
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        return pool.map(_evaluate, range(len(rays)), chunksize=8)


def path(scene, batch):
    return os.path.join(OUT, "%s_%s.npz" % (scene, batch))


def load(scene, batch):
    with np.load(path(scene, batch)) as z:
        c = G._unpacked({k: z[k] for k in z.files})
    for i, k in enumerate(KDM_FLAGS):
        c[k] = (c["kdm_flags"] >> i & 1).astype(np.bool_)
    m = c.pop("above")
    c["above_idx"], c["above_hit"], c["above_node"], c["above_sub"] = m[:, 0].astype(np.int32), m[:, 1] != 0, m[:, 2].astype(np.int32), m[:, 3].astype(np.int32)
    c["above_t"], c["above_point"], c["above_normal"] = m[:, 4].copy(), m[:, 5:8].copy(), m[:, 8:11].copy()
    del c["kdm_flags"]
    return c


def npz_bytes(cols):
    cols = dict(cols)
    cols["kdm_flags"] = sum(cols.pop(k).astype(np.uint8) << i for i, k in enumerate(KDM_FLAGS)).astype(np.uint8)
    return G.npz_bytes(cols)


def expected(c, which="nearest"):
    """gen_exact_rays.expected, and "above": the flat walk's nearest hit under the upper of the two bounds in c["t_max"]."""
    if which != "above":
        return G.expected(c, which)
    e = G.expected(c, "nearest")
    for k in e:
        e[k][c["above_idx"]] = c["above_" + k]
    return e


def scene_inputs(name):
    """(scene, flattened f64 matrices, primitives, the oracle's flattened arrays with its scene tree) - the matrices and the scene's tree are inputs."""
    import oracle_lib
    scene = build_scene(name)
    ps = oracle_lib.pack(scene)
    flat = oracle_lib.flatten(ps)
    prims = G.flat_prims(scene)
    assert [p.kind for p in prims] == [int(k) for k in flat["prim_type"]]
    flat["kd_tree"] = oracle_lib.kd_scene_dump(ps, kd_depth=SCATTER_DEPTH if name in BUILD_ONLY else KD_DEPTH)
    return scene, flat["trans"], prims, flat


def exact_scenes(name, inputs):
    import exact_ref
    scene, trans, prims, flat = inputs
    ex = exact_ref.ExactScene(scene, trans, flat["prim_type"])
    ex.set_tree(flat["kd_tree"])
    exm = exact_ref.ExactScene(build_scene(name, kd=False), trans)
    return ex, exm


def make_batch(name, batch, workers, exs=None, inputs=None):
    import exact_ref
    scene, trans, prims, flat = inputs = inputs or scene_inputs(name)
    ex, exm = exs or exact_scenes(name, inputs)
    view, vtrans = as_meshes(prims, trans)
    seed = [26, SCENES.index(name), BATCH_NAMES.index(batch)]
    extra = {}
    if batch == "camera":
        cam = G.scene_camera(vtrans, view)
        if name == "kdm_grid":   # from far above: the parameter at the sheets exceeds the extent, and few eye rays cross an x or z plane in the last 129
            cam = Camera(eye=(0.05, 16000.0, 0.15), center=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), fovy_degrees=0.02)   # units before them (see batch_grid)
        ys, xs = np.mgrid[0:G.CAM_H, 0:G.CAM_W]
        xy = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float64)
        eye, dirs = exact_ref.camera_rays(cam, G.CAM_W, G.CAM_H, xy)
        eye53, dirs53 = exact_ref.camera_rays(cam, G.CAM_W, G.CAM_H, xy, prec=53)
        f = lambda v: [float(x) for x in v]
        o, d = np.array([f(eye)] * len(xy)), np.array([f(v) for v in dirs])
        rays = [(o[k], (dirs[k], dirs53[k])) for k in range(len(xy))]
        extra = dict(cam=np.array([*cam.eye, *cam.center, *cam.up, cam.fovy_radians], dtype=np.float64), xy=xy)
    else:
        n = dict(BATCHES)[batch]
        m = n + n // 2
        if name == "kdm_grid":
            o, d = batch_grid(seed, m, trans, prims, batch)
        elif batch == "random":
            o, d = G.batch_random(seed, m, vtrans, view)
        elif batch == "near":
            o, d = G.batch_near(seed, m, vtrans, view)
        else:
            o, d = batch_special(seed, m, trans, prims)
        rays = [(o[k], d[k]) for k in range(m)]
    rows = evaluate(ex, exm, rays, workers)
    if batch != "camera":   # as gen_exact_rays: half as many rays again are drawn, and the first n that are well conditioned are kept
        keep = [k for k in range(len(rows)) if G.well_conditioned(rows[k])]
        extra["replaced"] = np.array([sum(1 for k in range(keep[n - 1]) if k not in set(keep))], dtype=np.int32)
        keep = keep[:n]
        o, d, rows = o[keep], d[keep], [rows[k] for k in keep]
    cols = G.columns(o, d, rows)
    for k in KDM_FLAGS:
        cols[k] = np.array([r[k] for r in rows], dtype=np.bool_)
    idx = [k for k, r in enumerate(rows) if r["above_differs"]]   # the flat walk's answers under the upper bound, where they are not the nearest hit
    a = [[k, rows[k]["above"]["hit"], rows[k]["above"]["node"], rows[k]["above"]["sub"], rows[k]["above"]["t"], *rows[k]["above"]["point"], *rows[k]["above"]["normal"]]
         for k in idx]
    cols["above"] = np.array(a, dtype=np.float64).reshape(len(idx), 11)
    cols.update(extra)
    cols["trans"] = np.ascontiguousarray(trans, dtype=np.float64)
    cols["prim_type"] = np.ascontiguousarray(flat["prim_type"], dtype=np.int32)
    for k, v in flat["kd_tree"].items():
        cols["tree_" + k] = np.ascontiguousarray(v)
    return cols


# ---------------------------------------------------------------- the scene builds
def fixture_tree(name):
    """The committed scene tree of a scene: the tree_* arrays of its fixture (tests/golden/exact/ for the four earlier scenes)."""
    if name in BUILD_ONLY:
        with np.load(os.path.join(OUT, name + "_tree.npz")) as z:
            c = {k: z[k] for k in z.files}
    else:
        c = G.load(name, "random") if name in G.SCENES else load(name, "random")
    t = {k[5:]: c[k] for k in c if k.startswith("tree_")}
    return t, c["trans"], c["prim_type"]


def build_report(name, prec=256):
    """The independent build of a scene's tree against the committed one: margin, decidable, structure, plane deviation, and the 53-bit evaluation's."""
    import exact_kd
    tree, trans, _ = fixture_tree(name)
    prims = G.flat_prims(build_scene(name))
    depth = SCATTER_DEPTH if name in BUILD_ONLY else KD_DEPTH
    mine, trace = exact_kd.scene_tree(trans, prims, depth, prec=prec)
    out = dict(nodes=len(mine["kind"]), leaves=int(sum(mine["kind"])), items=len(mine["items"]), depth=mine["depth"], decisions=trace.decisions,
               margin=trace.margin, decidable=bool(trace.margin >= G.FRAGILE))
    if out["decidable"]:
        out["structure_differs_in"] = exact_kd.same_structure(mine, tree)
        assert out["structure_differs_in"] is None, (name, "the committed tree is not the independent build's", out["structure_differs_in"])
        out["plane_deviation"] = exact_kd.plane_deviation(mine, tree)
        f53, _ = exact_kd.scene_tree(trans, prims, depth, prec=53)
        assert exact_kd.same_structure(mine, f53) is None, (name, "the 53-bit evaluation decides a decidable build differently")
        out["plane_deviation53"] = exact_kd.plane_deviation(mine, f53)
    return out


# ---------------------------------------------------------------- conditions (numpy only)
def check_conditions(scene, bs, log=print):
    """bs: {batch: columns} of one ray scene. The conditions of the fixture, asserted from the exact reference's columns alone; returns the counts."""
    kinds = np.asarray(bs["random"]["prim_type"])
    out = {}
    pairs, far, differ, alike, panics = set(), 0, 0, 0, 0
    for batch, c in bs.items():
        n = len(c["hit"])
        left_out = {"flat": c["fragile"], "hier": c["fragile"] | c["hier_fragile"], "kd": c["kd_fragile"],
                    "flat segments": c["fragile"] | c["segment_fragile"], "kd segments": c["kd_fragile"] | c["kd_segment_fragile"]}
        out[batch] = dict(rays=n, hit=int(c["hit"].sum()), panic=int(c["panic"].sum()), replaced=int(c["replaced"][0]) if "replaced" in c else 0,
                          left_out={k: int(v.sum()) for k, v in left_out.items()})
        log("%-10s %-8s %s" % (scene, batch, out[batch]))
        for k, v in left_out.items():
            assert v.sum() <= G.FRAGILE_CAP[batch] * n, (scene, batch, k, "fragile share", float(v.mean()))
        assert not (c["panic"] & ~(c["fragile"] | c["hier_fragile"] | c["kd_fragile"] | c["segment_fragile"] | c["kd_segment_fragile"])).any(), "a panic is left out"
        ok = ~c["fragile"]
        both = ok & ~c["hier_fragile"]
        assert np.array_equal(c["hier_hit"][both], c["hit"][both]), (scene, batch, "hierarchical hit differs")
        both &= c["hit"]
        assert np.array_equal(c["hier_node"][both], c["node"][both]) and np.array_equal(c["hier_sub"][both], c["sub"][both]), (scene, batch, "hierarchical node differs")
        assert np.all(np.abs(c["hier_dt"][both]) <= 2.0 ** -40 * np.maximum(1.0, np.abs(c["t"][both]))), (scene, batch, "hierarchical t differs")
        h = ok & c["hit"]
        on_kdm = h & np.isin(kinds[np.maximum(c["node"], 0)], (KDMESH,))
        pairs |= set(zip(c["node"][on_kdm].tolist(), c["sub"][on_kdm].tolist()))
        far += int((on_kdm & c["far"]).sum())
        differ += int((c["mesh_decidable"] & c["mesh_differs"]).sum())
        alike += int((c["mesh_decidable"] & c["mesh_alike"]).sum())
        panics += int(c["panic"].sum())
    out["totals"] = dict(distinct_triangles_hit=len(pairs), hits_found_on_a_pending_far_side=far, kdmesh_differs_from_mesh=differ,
                         kdmesh_and_mesh_hit_alike=alike, panics=panics)
    log("%-10s %s" % (scene, out["totals"]))
    assert len(pairs) >= MIN_TRIANGLES, (scene, "distinct triangles hit", len(pairs))
    assert far >= MIN_FAR, (scene, "hits found on a pending far side", far)
    if scene == "kdm_far":
        assert differ >= MIN_DIFFER and alike >= MIN_ALIKE, (scene, differ, alike)
    if scene == "kdm_near":
        assert differ == 0, (scene, "KDMesh must answer as Mesh here", differ)
    return out


def tolerances(batches):
    """gen_exact_rays.tolerances, where a deviation may be 0: kdm_grid's normals are (0, 1, 0) or its opposite in every evaluation, so its threshold for
    the normal is 0 and a normal there must be exact."""
    out = {}
    for scene, bs in batches.items():
        dev = np.max([G.deviations(c) for c in bs.values()], axis=0)
        out[scene] = {q: {"deviation": float(v), "threshold": float(G.SLACK * v)} for q, v in zip(("t", "point", "normal"), dev)}
        for q, v in out[scene].items():
            assert 0.0 <= v["threshold"] < G.THRESHOLD_CAP and (v["threshold"] > 0.0 or (scene, q) == ("kdm_grid", "normal")), (scene, q, v)
    return out


def load_tolerances():
    with open(os.path.join(OUT, "tolerances.json")) as fh:
        return json.load(fh)


def load_summary():
    with open(os.path.join(OUT, "summary.json")) as fh:
        return json.load(fh)


def build_tolerance(reports):
    """64 x the largest deviation of the 53-bit evaluation's planes and root bounds from the 256-bit one's over the decidable builds, capped at 2^-32."""
    dev = max(r["plane_deviation53"] for r in reports.values() if r["decidable"])
    thr = G.SLACK * dev
    assert 0.0 < thr < G.THRESHOLD_CAP, thr
    return {"deviation": dev, "threshold": thr}


def summarise(all_batches, reports):
    s = {"scenes": {name: check_conditions(name, bs) for name, bs in all_batches.items()}, "builds": reports,
         "undecidable_builds": sorted(n for n, r in reports.items() if not r["decidable"])}
    assert reports["scatter40"]["decidable"], "scatter40's seed must give a decidable build"
    return s


# ---------------------------------------------------------------- mutants: that the comparisons can fail
def _changed(ex, c, k, mode="flat"):
    """Does the evaluator, as it now stands (ex.mutant), answer ray k of the batch differently from the fixture? Decidable rays only."""
    if c["fragile"][k] or (mode == "kd" and c["kd_fragile"][k]):
        return False
    e = G.expected(c, "kd" if mode == "kd" else "nearest")
    d = c["d"][k]
    if "cam" in c:   # an eye ray's direction is not an f64 vector: its rounding may move t in the last bits, so t is not compared there
        h = ex.cast(c["o"][k], d, mode=mode)
        return bool(h) != bool(e["hit"][k]) or (bool(h) and (h.node, h.sub) != (int(e["node"][k]), int(e["sub"][k])))
    h = ex.cast(c["o"][k], d, mode=mode)
    if bool(h) != bool(e["hit"][k]):
        return True
    return bool(h) and (h.node, h.sub, float(h.t)) != (int(e["node"][k]), int(e["sub"][k]), float(e["t"][k]))


def _walk_mutant_task(task):
    import exact_ref
    mutant, name, stride = task
    inputs = scene_inputs(name)
    ex, _ = exact_scenes(name, inputs)
    ex.mutant = mutant
    out = {}
    for batch in BATCH_NAMES:
        c = load(name, batch)
        ks = [k for k in range(0, len(c["hit"]), 1 if batch == "special" else stride) if _changed(ex, c, k)]
        out[batch] = dict(changed=len(ks), witness=ks[:1])
    return mutant, name, out


def mutant_table(workers, stride=4):
    """Per mutant of the restatement: how many fixtures it changes. A build mutant: the triangle trees of the ray scenes' meshes and the decidable scene trees
    whose arrays change. A walk mutant: the batches in which a decidable ray (every `stride`-th is tried, every one of a `special` batch; flat traversal) is
    answered differently."""
    import exact_kd
    import exact_ref
    import multiprocessing
    table = {}
    meshes = {}
    for name in SCENES:
        for m in meshes_by_first_use([p for p in G.flat_prims(build_scene(name)) if p.kind == KDMESH])[1]:
            meshes[m.name] = m
    summary = load_summary()
    for mutant in exact_kd.MUTANTS:
        tri = sorted(n for n, m in meshes.items() if exact_kd.difference(exact_kd.mesh_tree(m, mutant=mutant), exact_kd.mesh_tree(m)) is not None)
        scn = []
        for name in BUILD_ONLY + G.SCENES + SCENES:
            if not summary["builds"][name]["decidable"]:
                continue
            tree, trans, _ = fixture_tree(name)
            depth = SCATTER_DEPTH if name in BUILD_ONLY else KD_DEPTH
            if exact_kd.same_structure(exact_kd.scene_tree(trans, G.flat_prims(build_scene(name)), depth, mutant=mutant)[0], tree) is not None:
                scn.append(name)
        table[mutant] = dict(kind="build", triangle_trees_changed=tri, scene_trees_changed=scn, fixtures_changed=len(tri) + len(scn))
    tasks = [(m, name, stride) for m in exact_ref.WALK_MUTANTS for name in SCENES]
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        res = pool.map(_walk_mutant_task, tasks, chunksize=1)
    for mutant in exact_ref.WALK_MUTANTS:
        per = {"%s_%s" % (name, b): v for m, name, out in res if m == mutant for b, v in out.items()}
        witness = [[f, v["witness"][0]] for f, v in sorted(per.items()) if v["witness"]]
        table[mutant] = dict(kind="walk", fixtures_changed=sum(1 for v in per.values() if v["changed"]), rays_changed=sum(v["changed"] for v in per.values()),
                             stride=stride, witnesses=witness[:3])
    return table


def load_mutants():
    with open(os.path.join(OUT, "mutants.json")) as fh:
        return json.load(fh)


def _dump(obj, name):
    with open(os.path.join(OUT, name), "w") as fh:
        json.dump(obj, fh, indent=1, sort_keys=True)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--mutants", action="store_true", help="evaluate the mutants of the restatement on the fixtures and write mutants.json")
    a = ap.parse_args()
    if a.mutants:
        table = mutant_table(a.workers)
        for k, v in table.items():
            print(k, v["fixtures_changed"], v)
            assert v["fixtures_changed"] >= 1 or k in EQUIVALENT_MUTANTS, (k, "changes no fixture: the comparisons cannot catch it")
        _dump(table, "mutants.json")
        return
    if a.check:
        scene, batch = CHECK_BATCH
        same = npz_bytes(make_batch(scene, batch, a.workers)) == open(path(scene, batch), "rb").read()
        print("%s_%s regenerated: %s" % (scene, batch, "byte-identical" if same else "DIFFERENT"))
        assert same
    else:
        os.makedirs(OUT, exist_ok=True)
        for name in a.scenes.split(","):
            inputs = scene_inputs(name)
            exs = exact_scenes(name, inputs)
            for batch in BATCH_NAMES:
                cols = make_batch(name, batch, a.workers, exs, inputs)
                with open(path(name, batch), "wb") as fh:
                    fh.write(npz_bytes(cols))
                print(name, batch, G.shares(cols), os.path.getsize(path(name, batch)), flush=True)
        for name in BUILD_ONLY:
            _, trans, prims, flat = scene_inputs(name)
            cols = {"trans": np.ascontiguousarray(trans), "prim_type": np.ascontiguousarray(flat["prim_type"], dtype=np.int32)}
            cols.update({"tree_" + k: np.ascontiguousarray(v) for k, v in flat["kd_tree"].items()})
            with open(os.path.join(OUT, name + "_tree.npz"), "wb") as fh:
                fh.write(_plain_npz(cols))
    allb = {s: {b: load(s, b) for b in BATCH_NAMES} for s in SCENES}
    reports = {name: build_report(name) for name in BUILD_ONLY + G.SCENES + SCENES}
    summary = summarise(allb, reports)
    tol = {"fragile_margin": G.FRAGILE, "slack": G.SLACK, "threshold_cap": G.THRESHOLD_CAP, "scenes": tolerances(allb), "build": build_tolerance(reports)}
    if a.check:
        assert summary == load_summary(), "summary.json is stale"
        assert tol == load_tolerances(), "tolerances.json is stale"
    else:
        _dump(summary, "summary.json")
        _dump(tol, "tolerances.json")
    print(json.dumps(summary["undecidable_builds"]), json.dumps(tol["build"]))
    for s in SCENES:
        print(s, {q: "%.3g" % v["threshold"] for q, v in tol["scenes"][s].items()})


def _plain_npz(cols):
    """An .npz of the arrays as they are, with the fixed member times and order of gen_exact_rays.npz_bytes."""
    import io
    import zipfile
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


if __name__ == "__main__":
    main()
