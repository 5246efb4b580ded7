#!/usr/bin/env python3
"""Generates tests/golden/exact_shading/: lit scenes, ray batches and the exact reference's colours for them (tests/exact_shade.py).

    python tools/gen_exact_shading.py            # regenerate every file (about 5 minutes on 8 workers; deterministic, byte for byte)
    python tools/gen_exact_shading.py --check    # regenerate one batch and compare its bytes, re-assert the input conditions, print shares and coverage

The scene builders, the conditions and what the tests compare with need only numpy and tests/scene_dsl.py; mpmath is needed to evaluate. The fragility
margin (2^-30), the factor on the measured deviation (64), the cap on a threshold (2^-24), the cast limit (96) and the caps on the shares below were fixed
before anything was measured.

A batch keeps every candidate ray up to the one that completes its count of usable rays: a ray whose own 53-bit evaluation strays by more than
cap / 64 / 2, or whose tree needs more than 96 casts, stays in the batch with the `bad` flag and is compared with nothing (a ray's index is its random
stream, so rays cannot be taken out without moving the others). Such rays may be a quarter of the usable count at most.
"""
from __future__ import annotations

import argparse
import io
import json
import math
import os
import sys
import time
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_exact_rays as R  # noqa: E402
from scene_dsl import CONE, CUBE, CYLINDER, SPHERE, Camera, Cube, Light, Material, Node, Plane, Scene, Sphere  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "exact_shading")
SCENES = ("lit15", "lit_nested", "hall", "hall_opaque", "lit_tris", "many65", "tangent")
BATCHES = (("random", 256), ("inside", 128), ("special", 128))   # usable rays per batch
CAM_SIZE = {"many65": (8, 4)}                                  # many65's one batch: 32 eye rays
CAM_W, CAM_H = 16, 12
FRAGILE = 2.0 ** -30
SLACK = 64.0
THRESHOLD_CAP = 2.0 ** -24
ILL = THRESHOLD_CAP / SLACK / 2
MAX_CASTS = 96
REPLACED_CAP = 0.25
FRAGILE_CAP = {"random": 0.02, "camera": 0.15, "inside": 0.15, "special": 0.15}
COVER_MIN = 20
KD_DEPTH = R.KD_DEPTH
CHECK_BATCH = ("lit15", "inside")   # area and glossy draws, recursion, a replaced ray
AMBIENT = (0.1, 0.15, 0.2)
GLASS = 1.51
# material kinds
PLAIN, SPEC_EPS, MIRROR, GLOSSY, GLASS_KIND = 0, 1, 2, 3, 4
KIND_NAMES = ("plain", "specular 1e-5", "opaque mirror", "glossy mirror", "glass")
FLAGS = ("hit", "fragile", "kd_fragile", "hier_fragile", "bad", "depth11", "hier_same")
INFO = ("node", "branch", "kind", "casts", "deepest", "events", "kd_events")
EVENTS = ("shadow_near", "shadow_beyond", "lit_back", "lit_front", "enter", "leave", "tir", "depth11", "miss_deep", "glossy_z", "glossy_xy")   # exact_shade.EVENTS


# what a ray of a `special` batch was built for (column `tag`: kind, side, light): side 0 is inside / below / on, side 1 outside / above / behind
TAG_NONE, TAG_KD, TAG_GLOSSY, TAG_CRITICAL, TAG_SILHOUETTE, TAG_NORMAL, TAG_TANGENT = range(7)


def batches_of(scene):
    if scene == "tangent":
        return ("camera", "special")
    return ("camera",) if scene == "many65" else ("camera",) + tuple(b for b, _ in BATCHES)


def cam_size(scene):
    return CAM_SIZE.get(scene, (CAM_W, CAM_H))


# ---------------------------------------------------------------- scenes
def lit_material(k):
    """Leaf k of the 15: the five kinds cycle so that each kind meets three different primitives; shininess runs from 10 to 250."""
    base = R._material(k)
    kind = (k + 2 * (k // 5)) % 5
    m = Material(diffuse=base.diffuse, specular=(0.4, 0.3, 0.2), shininess=10.0 + 240.0 * k / 14.0)
    if kind == SPEC_EPS:
        m.specular = (1e-5, 1e-5, 1e-5)
    elif kind == MIRROR:
        m.reflectivity = 0.6
    elif kind == GLOSSY:
        m.reflectivity, m.glossy_side_length = 0.6, 0.2
    elif kind == GLASS_KIND:
        m.reflectivity, m.refraction_index = 0.9, GLASS
    return m


def material_kind(m):
    if m.refraction_index > 0 and m.reflectivity > 0:
        return GLASS_KIND
    if m.reflectivity > 0:
        return GLOSSY if m.glossy_side_length > 0 else MIRROR
    return SPEC_EPS if max(m.specular) == 1e-5 else PLAIN


def _relit(root):
    """The 15 leaves carry _material(k), whose shininess 10 + k names the leaf: each gets lit_material(k)."""
    stack = [root]
    while stack:
        n = stack.pop()
        if n.geometry is not None:
            n.geometry = (n.geometry[0], lit_material(int(round(n.geometry[1].shininess - 10.0))))
        stack.extend(n.children)
    return root


def lights15():
    return [Light(position=(9.0, 11.0, 8.0), color=(0.8, 0.8, 0.8)),                                    # outside the cloud, default falloff
            Light(position=(-8.0, 6.0, -7.0), color=(3.0, 2.5, 2.0), falloff=(1.0, 0.05, 0.01)),
            Light(position=(0.25, 0.5, -0.75), color=(0.5, 0.6, 0.7)),                                    # inside the cloud: objects lie beyond it
            Light(position=(-6.0, 10.0, 7.0), color=(0.6, 0.5, 0.4), area_a=(1.5, 0.0, 0.5), area_b=(0.0, 0.5, 1.5))]


def scene_lit15():
    return Scene(_relit(R.scene_flat15().root), lights15(), AMBIENT)


def scene_lit_nested():
    return Scene(_relit(R.scene_nested15().root), lights15(), AMBIENT)


HALL_TURN = (0.25, 0.375)   # the hall is built on its own axes and turned about x, then y: no surface of it is parallel to a world axis


def hall_to_world(v):
    """Rotation about x, then about y, in plain float arithmetic (no library product, whose rounding may differ between machines)."""
    cx, sx, cy, sy = math.cos(HALL_TURN[0]), math.sin(HALL_TURN[0]), math.cos(HALL_TURN[1]), math.sin(HALL_TURN[1])
    x, y, z = (float(c) for c in v)
    y, z = cx * y - sx * z, sx * y + cx * z
    return (cy * x + sy * z, y, -sy * x + cy * z)


def _hall(glass):
    w = hall_to_world
    mirror = lambda: Material(diffuse=(0.05, 0.05, 0.08), specular=(0.3, 0.3, 0.3), shininess=80.0, reflectivity=0.8)
    nodes = [Node.geo(Cube(), mirror()).scaled((16.0, 6.0, 0.6)).translated((0.0, 2.0, 2.0)),
             Node.geo(Cube(), mirror()).scaled((16.0, 6.0, 0.6)).translated((0.0, 2.0, -2.0)),
             Node.geo(Plane(), Material(diffuse=(0.6, 0.5, 0.3), specular=(0.2, 0.2, 0.2), shininess=20.0)).scaled((16.0, 1.0, 8.0)).translated((0.0, -1.0, 0.0))]
    if glass:
        g = lambda d: Material(diffuse=d, specular=(0.5, 0.5, 0.5), shininess=120.0, reflectivity=0.9, refraction_index=GLASS)
        nodes.append(Node.geo(Cube(), g((0.05, 0.1, 0.08))).scaled(0.9).rotated_y(0.5).translated((-1.0, -0.54, 0.2)))
        nodes.append(Node.geo(Sphere(), g((0.1, 0.05, 0.05))).scaled(0.5).translated((1.1, -0.45, -0.3)))
    lights = [Light(position=w((0.5, 3.5, 0.3)), color=(0.9, 0.9, 0.9)),
              Light(position=w((-3.0, 4.0, -0.5)), color=(0.5, 0.5, 0.4), falloff=(1.0, 0.02, 0.005), area_a=w((0.4, 0.0, 0.0)), area_b=w((0.0, 0.0, 0.4)))]
    return Scene(Node.group([Node.group(nodes).rotated_x(HALL_TURN[0]).rotated_y(HALL_TURN[1])]), lights, AMBIENT)


def scene_lit_tris():
    """The `tris` geometry and materials (none reflective) under two point lights. The variant with a mirror on one mesh was left out."""
    lights = [Light(position=(4.0, 6.0, 5.0), color=(0.9, 0.9, 0.8)), Light(position=(-5.0, 3.0, -4.0), color=(1.5, 1.5, 2.0), falloff=(1.0, 0.05, 0.01))]
    return Scene(R.scene_tris().root, lights, AMBIENT)


def scene_many65():
    plain = lambda d, k: Material(diffuse=d, specular=(0.3, 0.3, 0.3), shininess=30.0 + k)
    nodes = [Node.geo(Sphere(), plain((0.7, 0.3, 0.2), 0)).scaled(0.8).translated((-1.2, 1.0, 0.0)),
             Node.geo(Cube(), plain((0.2, 0.6, 0.3), 1)).scaled(1.2).rotated_y(0.4).translated((1.3, 0.9, 0.2)),
             Node.geo(Plane(), plain((0.5, 0.5, 0.6), 2)).scaled((12.0, 1.0, 12.0)).translated((0.0, -0.5, 0.0))]
    lights = []
    for k in range(65):   # a 13 x 5 grid above the objects; every eighth light lies between the objects and the plane
        x, z = -4.5 + 0.75 * (k % 13), -3.0 + 1.5 * (k // 13)
        y = -0.25 if k % 8 == 3 else 3.5 + 0.125 * (k % 5)
        lights.append(Light(position=(x, y, z), color=(0.03 + 0.002 * (k % 7), 0.03, 0.04 - 0.002 * (k % 3)), falloff=(1.0, 0.05, 0.01)))
    return Scene(Node.group(nodes), lights, AMBIENT)


TANGENT_BEHIND = 2.0 ** -20


def scene_tangent():
    """A cube with faces at +-1 and an open plane at y = -1.5, both on the world's axes, under four point lights, all outside the surfaces' extents:
    one 2^-20 behind the plane of the cube's top face (n.l < 0 there, and the cube itself shadows it), one 2^-20 in front of the open plane and one 2^-20
    behind it (n.l > 0 and < 0, the shadow ray runs along the surface, nothing shadows), and one EXACTLY on the plane of the cube's bottom face: there the
    shadow ray's direction has a zero component that the face's test divides by, which the exact reference cannot decide (margin 0), so hits on that
    face are recorded and left out; the few rays aimed at it stay below the cap on fragile rays."""
    plain = lambda d, k: Material(diffuse=d, specular=(0.4, 0.3, 0.2), shininess=20.0 + 10.0 * k)
    nodes = [Node.geo(Cube(), plain((0.6, 0.3, 0.2), 0)).scaled(2.0),
             Node.geo(Plane(), plain((0.3, 0.5, 0.6), 1)).scaled((8.0, 1.0, 8.0)).translated((0.0, -1.5, 0.0))]
    lights = [Light(position=(3.0, -1.0, 0.5), color=(0.9, 0.8, 0.7)),
              Light(position=(-0.5, 1.0 - TANGENT_BEHIND, -3.0), color=(0.7, 0.8, 0.9), falloff=(1.0, 0.05, 0.01)),
              Light(position=(5.0, -1.5 + TANGENT_BEHIND, 0.25), color=(0.8, 0.9, 0.7)),
              Light(position=(-5.0, -1.5 - TANGENT_BEHIND, 0.5), color=(0.9, 0.7, 0.8), falloff=(1.0, 0.05, 0.01))]
    return Scene(Node.group(nodes), lights, AMBIENT)


def build_scene(name):
    return {"lit15": scene_lit15, "lit_nested": scene_lit_nested, "hall": lambda: _hall(True), "hall_opaque": lambda: _hall(False),
            "lit_tris": scene_lit_tris, "many65": scene_many65, "tangent": scene_tangent}[name]()


def scene_camera(name, trans, prims):
    if name.startswith("hall"):
        return Camera(eye=hall_to_world((0.75, 0.75, 1.25)), center=hall_to_world((0.25, 0.0, -1.75)), up=hall_to_world((0.0, 1.0, 0.0)), fovy_degrees=50.0)
    if name == "tangent":
        return Camera(eye=(2.5, 3.5, 6.0), center=(0.0, -0.5, 0.0), up=(0.0, 1.0, 0.0), fovy_degrees=45.0)
    if name == "many65":
        return Camera(eye=(0.5, 3.0, 7.0), center=(0.0, 0.5, 0.0), up=(0.0, 1.0, 0.0), fovy_degrees=40.0)
    return R.scene_camera(trans, prims)


def flat_materials(scene):
    out, queue = [], [scene.root]
    while queue:
        n = queue.pop(0)
        if n.geometry is not None:
            out.append(n.geometry[1])
        queue.extend(n.children)
    return out


def background(i):
    """Ray i's own background colour: exact dyadic fractions, distinct over any 512 consecutive indices."""
    i = np.asarray(i, dtype=np.int64)
    return np.stack([((i * 37 + 11) % 64) / 64.0, ((i * 17 + 5) % 32) / 32.0 * 0.5 + 0.25, ((i * 29 + 3) % 128) / 128.0], axis=-1)


# ---------------------------------------------------------------- rays
def _length(rng, v):
    return v / np.linalg.norm(v) * 2.0 ** rng.uniform(-3.0, 3.0)


def _closed(prims):
    return [i for i, p in enumerate(prims) if p.kind in (SPHERE, CUBE, CYLINDER, CONE, R.MESH)]


def batch_random(rng, m, name, trans, prims):
    """Rays from around the scene aimed into the objects, direction lengths 2^-3 to 2^3."""
    lo, hi, ids = R.regions(trans, prims)[0]
    c, e = (lo + hi) / 2, (hi - lo) / 2
    if name.startswith("hall"):
        c, e = np.array([0.0, 1.0, 0.0]), np.array([5.0, 1.8, 1.5])
    o, d = np.zeros((m, 3)), np.zeros((m, 3))
    for k in range(m):
        if name.startswith("hall"):
            o[k] = hall_to_world(c + e * rng.uniform(-1, 1, 3))
        else:
            o[k] = c + R._unit(rng) * rng.uniform(1.1, 2.0) * np.linalg.norm(e)
        i = ids[rng.integers(len(ids))]
        d[k] = _length(rng, R._to_world(trans[i], R._inside_point(rng, prims[i], 0.8)) - o[k])
    return R._grid(o), d.astype(np.float32).astype(np.float64)


def batch_inside(rng, m, name, trans, prims):
    """Rays that start inside closed objects and, in the halls, between the mirrors and nearly square to them."""
    solid = _closed(prims)
    if name.startswith("hall"):
        solid = solid[2:]   # not inside the mirrors
    o, d = np.zeros((m, 3)), np.zeros((m, 3))
    for k in range(m):
        if name.startswith("hall") and (k % 2 == 0 or not solid):
            o[k] = hall_to_world((rng.uniform(-4, 4), rng.uniform(0.3, 3.5), rng.uniform(-1.5, 1.5)))
            d[k] = _length(rng, np.array(hall_to_world((rng.uniform(-0.12, 0.12), rng.uniform(-0.04, 0.04), rng.choice([-1.0, 1.0])))))
        else:
            i = solid[rng.integers(len(solid))]
            o[k] = R._to_world(trans[i], R._inside_point(rng, prims[i], 0.5))
            d[k] = _length(rng, R._unit(rng))
    return o, d.astype(np.float32).astype(np.float64)


def surface_points(ex, o, d):
    """(node, point, normal) of the nearest hits of the rays, in f64."""
    out = []
    for k in range(len(o)):
        h = ex.cast(o[k], d[k], prec=53)
        if h and all(float(c) == float(c) for c in h.normal):
            out.append((h.node, np.array([float(c) for c in h.point]), np.array([float(c) for c in h.normal]), d[k]))
    return out


def _hits_node(ex, i, o, d):
    import exact_ref
    from mpmath import mpf
    with mp.workprec(53):
        inv = ex.flat_matrices()[i][1]
        om, dm = exact_ref._point(inv, tuple(mpf(float(x)) for x in o)), exact_ref._direction(inv, tuple(mpf(float(x)) for x in d))
        return ex.flat[i].geometry.hit(exact_ref.Trace(), om, dm, mpf(exact_ref.EPS_F64), mp.inf, False) is not None


def silhouette_rays(rng, count, ex, trans, prims, lights):
    """Hits at normal incidence whose shadow ray to a point light passes a closed object's silhouette at relative distance 2^-20, inside and outside
    alternately: the silhouette is bisected along a line across the light's view of the object, the receiver is what lies behind it on that line."""
    o, d, tag = [], [], []
    solid = _closed(prims)
    point = [(k, np.array(l.position, dtype=np.float64)) for k, l in enumerate(lights) if tuple(l.area_a) == (0.0, 0.0, 0.0) or tuple(l.area_b) == (0.0, 0.0, 0.0)]
    for _ in range(40 * count):
        if len(o) >= count or not solid or not point:
            break
        i, (li, light) = solid[rng.integers(len(solid))], point[rng.integers(len(point))]
        lo, hi = R.model_box(prims[i])
        axis = R._to_world(trans[i], (lo + hi) / 2) - light
        wlo, whi = R.world_box(trans[i], prims[i])
        rad = float(np.linalg.norm(whi - wlo)) / 2
        u = R._perp(rng, axis)
        a, b = 0.0, 1.5 * rad
        if not _hits_node(ex, i, light, axis) or _hits_node(ex, i, light, axis + b * u):
            continue
        for _ in range(60):
            mid = (a + b) / 2
            a, b = (mid, b) if _hits_node(ex, i, light, axis + mid * u) else (a, mid)
        outside = len(o) % 2
        way = axis + a * (1.0 + (2.0 ** -20 if outside else -2.0 ** -20)) * u
        way = way / np.linalg.norm(way)
        start, found = light, None
        for _ in range(6):   # the first surface on the line that lies behind the object
            h = ex.cast(start, way, prec=53)
            if not h:
                break
            pt, nr = np.array([float(c) for c in h.point]), np.array([float(c) for c in h.normal])
            if h.node != i and float((pt - light) @ way) > float(np.linalg.norm(axis)) and nr[0] == nr[0]:
                found = (pt, nr)
                break
            start = pt + way * 0.05 * rad
        if found is None:
            continue
        pt, nr = found
        back = ex.cast(pt, light - pt, prec=53)   # what the shadow ray from there meets first: the object on the inside, nothing at all on the outside
        if (not outside and not (back and back.node == i)) or (outside and back):
            continue
        side = 1.0 if float((light - pt) @ nr) > 0 else -1.0   # seen from the side the light is on
        first = ex.cast(pt + side * nr * 2.0 ** -3, -side * nr, prec=53)   # the ray must see that point, and nothing in front of it
        if not first or first.node != h.node or float(max(abs(float(x) - y) for x, y in zip(first.point, pt))) > 2.0 ** -30:
            continue
        o.append(pt + side * nr * 2.0 ** -3); d.append(-side * nr * 2.0 ** int(rng.integers(-3, 4))); tag.append((TAG_SILHOUETTE, outside, li))
    return o, d, tag


def batch_special(rng, m, name, trans, prims, kinds, surf, ex=None, lights=()):
    """Constructed rays: hits at normal incidence; on glossy surfaces, reflected directions within 2^-18 and 2^-22 of the z axis and with one of x, y
    moved to 2^-15, on the other side of the glossy test; in `hall`, incidence from inside the glass cube at the critical angle -+ 2^-20.
    In lit15 and lit_nested, 24 rays of the geometry fixtures (tests/golden/exact, same geometry and k-d tree) that the k-d walk answers differently from
    the flat walk: direction lengths down to 10^-2, where the walk's segment ends short of the hit (quirk Q3).
    32 rays of silhouette_rays(). Returns origins, directions and the tag column. (Lights on a tangent plane: scene_tangent, batch_tangent.)"""
    o, d, tag = [], [], []
    geometry = {"lit15": "flat15", "lit_nested": "nested15"}.get(name)
    if geometry:
        g = R.load(geometry, "random")
        idx = g["kd_idx"][~g["kd_fragile"][g["kd_idx"]] & ~g["fragile"][g["kd_idx"]]][:24]
        o, d, tag = list(g["o"][idx]), list(g["d"][idx]), [(TAG_KD, 0, 0)] * len(idx)
    glossy = [s for s in surf if kinds[s[0]] == GLOSSY and abs(s[2][2]) >= 0.2]
    n_glossy = 3 * m // 8 if glossy else 0
    n_crit = m // 3 if name == "hall" else 0
    small = [(2.0 ** -18, 2.0 ** -22), (2.0 ** -22, 2.0 ** -18), (2.0 ** -15, 2.0 ** -22), (2.0 ** -22, 2.0 ** -15)]
    for k in range(n_glossy):
        node, p, n, _ = glossy[rng.integers(len(glossy))]
        ex_, ey_ = small[k % 4]
        r = np.array([ex_ * rng.choice([-1.0, 1.0]), ey_ * rng.choice([-1.0, 1.0]), 1.0 if n[2] > 0 else -1.0])
        if k % 8 >= 4:
            r *= 2.0 ** int(rng.integers(-2, 3))   # the test is on the direction as given, not on a unit vector
            r[:2] = [ex_ * rng.choice([-1.0, 1.0]), ey_ * rng.choice([-1.0, 1.0])]
        din = r - 2.0 * float(r @ n) * n
        o.append(p - din * 2.0 ** -2 / np.linalg.norm(din)); d.append(din); tag.append((TAG_GLOSSY, k % 4 >= 2, 0))
    cube = 3   # hall's glass cube, scaled 0.9: in its model space the top face has the normal +y, and angles are those of world space
    for k in range(n_crit):
        theta = math.asin(1.0 / GLASS) + (2.0 ** -20 if k % 2 else -2.0 ** -20)
        phi = rng.uniform(0, 2 * math.pi)
        start = R._to_world(trans[cube], np.array([0.1 * rng.uniform(-1, 1), rng.uniform(0.2, 0.35), 0.1 * rng.uniform(-1, 1)]))   # the top face is met first
        v = np.array([math.sin(theta) * math.cos(phi), math.cos(theta), math.sin(theta) * math.sin(phi)])
        v = trans[cube][:3, :3] @ v
        # unit length: refracted_direction decides on the direction as given, so only at length 1 is the angle what decides
        o.append(start); d.append(v / np.linalg.norm(v)); tag.append((TAG_CRITICAL, k % 2, 0))
    so, sd, st = silhouette_rays(rng, 32, ex, trans, prims, lights)
    o, d, tag = o + so, d + sd, tag + st
    while len(o) < m:   # normal incidence, from the side the first ray came from
        node, p, n, din = surf[rng.integers(len(surf))]
        side = -1.0 if float(din @ n) > 0 else 1.0
        o.append(p + side * n * 2.0 ** -3); d.append(-side * n * 2.0 ** int(rng.integers(-3, 4))); tag.append((TAG_NORMAL, 0, 0))
    return np.array(o), np.array(d), np.array(tag, dtype=np.int8).reshape(len(o), 3)


def batch_tangent(rng, m, trans, prims):
    """Oblique rays, direction lengths 2^-3 to 2^3, onto the cube's top face (side 0), onto the open plane beside the cube (side 1) and, one in ten, from
    the gap under the cube onto its bottom face (side 2), on whose plane a light lies exactly (scene_tangent)."""
    o, d, tag = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros((m, 3), dtype=np.int8)
    for k in range(m):
        side = 2 if k % 10 == 9 else k % 2
        if side == 0:
            target = np.array([rng.uniform(-0.9, 0.9), 1.0, rng.uniform(-0.9, 0.9)])
        elif side == 1:
            target = np.array([rng.uniform(1.5, 3.8) * rng.choice([-1.0, 1.0]), -1.5, rng.uniform(-3.8, 3.8)])
        else:
            target = np.array([rng.uniform(-0.8, 0.8), -1.0, rng.uniform(-0.8, 0.8)])
        if side == 2:
            o[k] = R._grid(target + np.array([rng.uniform(-0.5, 0.5), -0.25, rng.uniform(-0.5, 0.5)]))
        else:
            o[k] = R._grid(target + np.array([rng.uniform(-2.0, 2.0), rng.uniform(1.0, 4.0), rng.uniform(-2.0, 2.0)]))
        d[k] = _length(rng, target - o[k])
        tag[k] = (TAG_TANGENT, side, 0)
    return o, d.astype(np.float32).astype(np.float64), tag


# ---------------------------------------------------------------- evaluation
_EX = None
_RAYS = None
EXTRA = None   # a generator built on this one (tools/gen_exact_textures.py) sets it: further entries of a ray's row, from its flat 256-bit evaluation
try:
    from mpmath import mp
except ImportError:   # the tests' numpy-only half
    mp = exact_shade = None
else:
    import exact_shade


def _draws(index):
    import oracle_lib
    k = [2]

    def draw():
        v = oracle_lib.rng_draw(0, index, 0, k[0])
        k[0] += 1
        return v
    return draw


def _run(ex, index, o, d, bg, mode, prec):
    try:
        return ex.color(o, d, bg, _draws(index), mode=mode, prec=prec, max_casts=MAX_CASTS)
    except exact_shade.TooManyCasts:
        return None


def _dev(a, b):
    """max over channels of |a - b| / max(1, |b|), a and b Shaded or None; inf where the decisions differ."""
    if a is None or b is None or a.path != b.path:
        return math.inf
    with mp.workprec(exact_shade.PREC):
        return max(float(abs(x - y)) / max(1.0, abs(float(y))) for x, y in zip(a.color, b.color))


def _evaluate(k):
    ex = _EX
    o, d = _RAYS[k]
    d53 = d
    if isinstance(d, tuple):
        d, d53 = d
    bg = [float(x) for x in background(k)]
    r = dict(bad=True, hit=False, rgb=[0.0] * 3, margin=0.0, kd_margin=0.0, hier_margin=0.0, dev=math.inf, node=-1, branch=0, casts=MAX_CASTS + 1, deepest=0,
             depth11=False, events=0, kd_events=0, shadow=[0, 0, 0, 0], kd_differs=False, kd_rgb=[0.0] * 3, kd_dev=0.0, hier_dev=0.0, hier_rgb=[0.0] * 3, hier_same=False)
    f = _run(ex, k, o, d, bg, "flat", exact_shade.PREC)
    if f is None:
        return r
    mask = (1 << 64) - 1
    r.update(hit=f.node >= 0, rgb=f.rgb(), margin=f.margin, node=f.node, branch=f.branch, casts=f.casts, deepest=f.deepest, depth11=f.depth11, events=f.events,
             shadow=[f.shadowed & mask, f.shadowed_beyond & mask, f.lit_front & mask, f.lit_back & mask],
             any_shadow=[f.shadowed & ~f.shadowed_beyond != 0, f.shadowed_beyond != 0, f.lit_front != 0, f.lit_back != 0])
    if EXTRA is not None:
        r.update(EXTRA(f))
    r["dev"] = _dev(_run(ex, k, o, d53, bg, "flat", 53), f)
    kd = _run(ex, k, o, d, bg, "kd", exact_shade.PREC)
    hier = _run(ex, k, o, d, bg, "hier", exact_shade.PREC)
    if kd is None or hier is None:
        return r
    r["kd_margin"], r["kd_rgb"], r["kd_events"] = kd.margin, kd.rgb(), kd.events
    r["kd_differs"] = kd.rgb() != f.rgb() or kd.path != f.path
    if r["kd_differs"]:
        r["kd_dev"] = _dev(_run(ex, k, o, d53, bg, "kd", 53), kd)
    r["hier_margin"], r["hier_rgb"], r["hier_same"] = hier.margin, hier.rgb(), hier.path == f.path
    r["hier_dev"] = _dev(_run(ex, k, o, d53, bg, "hier", 53), hier)
    ill = ((f.margin >= FRAGILE and r["dev"] > ILL) or (r["kd_differs"] and kd.margin >= FRAGILE and r["kd_dev"] > ILL)
           or (hier.margin >= FRAGILE and r["hier_dev"] > ILL))
    r["bad"] = bool(ill)
    return r


def evaluate(ex, rays, workers):
    global _EX, _RAYS
    _EX, _RAYS = ex, rays
    if workers <= 1:
        return [_evaluate(k) for k in range(len(rays))]
    import multiprocessing
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        return pool.map(_evaluate, range(len(rays)), chunksize=2)


def columns(o, d, rows, kinds):
    n = len(rows)
    c = dict(rays=np.concatenate([np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64), background(np.arange(n))], axis=1))
    c["rgb"] = np.array([r["rgb"] for r in rows], dtype=np.float64).reshape(n, 3)
    flag = dict(hit=[r["hit"] for r in rows], fragile=[r["margin"] < FRAGILE for r in rows], kd_fragile=[r["kd_margin"] < FRAGILE for r in rows],
                hier_fragile=[r["hier_margin"] < FRAGILE for r in rows], bad=[r["bad"] for r in rows], depth11=[r["depth11"] for r in rows], hier_same=[r["hier_same"] for r in rows])
    c["flags"] = sum(np.array(flag[k], dtype=np.uint16) << i for i, k in enumerate(FLAGS)).astype(np.uint16)
    kind = [kinds[r["node"]] if r["node"] >= 0 else -1 for r in rows]
    c["info"] = np.array([[r["node"], r["branch"], kd_, min(r["casts"], 32767), r["deepest"], r["events"], r["kd_events"]] for r, kd_ in zip(rows, kind)],
                         dtype=np.int16).reshape(n, len(INFO))
    c["shadow"] = np.array([r["shadow"] for r in rows], dtype=np.uint64).reshape(n, 4)   # depth 0, per light: shadowed, beyond only, lit n.l > 0, lit n.l < 0
    fin = lambda v: np.float32(v if math.isfinite(v) else 3e38)
    c["dev53"] = np.array([fin(r["dev"]) for r in rows], dtype=np.float32)
    c["hier_dev53"] = np.array([fin(r["hier_dev"]) for r in rows], dtype=np.float32)
    c["hier_rgb"] = np.array([r["hier_rgb"] for r in rows], dtype=np.float64).reshape(n, 3)   # the hierarchical walk composes the builder calls unrounded
    idx = [k for k, r in enumerate(rows) if r["kd_differs"] and not r["bad"]]
    c["kd"] = np.array([[k, *rows[k]["kd_rgb"], float(fin(rows[k]["kd_dev"]))] for k in idx], dtype=np.float64).reshape(len(idx), 5)
    return c


def unpacked(z):
    c = dict(z)
    c["o"], c["d"], c["bg"] = (np.ascontiguousarray(c["rays"][:, 3 * k:3 * k + 3]) for k in range(3))
    for i, k in enumerate(FLAGS):
        c[k] = (c["flags"] >> i & 1).astype(np.bool_)
    for i, k in enumerate(INFO):
        c[k] = np.ascontiguousarray(c["info"][:, i]).astype(np.int32)
    c["kd_idx"], c["kd_rgb"], c["kd_dev53"] = c["kd"][:, 0].astype(np.int32), np.ascontiguousarray(c["kd"][:, 1:4]), c["kd"][:, 4].copy()
    return c


def npz_bytes(cols):
    """An .npz whose bytes depend on nothing but the arrays: fixed member times, sorted names."""
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
        return unpacked({k: z[k] for k in z.files})


def scene_inputs(name):
    import oracle_lib
    scene = build_scene(name)
    ps = oracle_lib.pack(scene)
    flat = oracle_lib.flatten(ps)
    prims = R.flat_prims(scene)
    assert [p.kind for p in prims] == [int(k) for k in flat["prim_type"]] and len(prims) <= 17
    flat["kd_tree"] = oracle_lib.kd_scene_dump(ps, kd_depth=KD_DEPTH)
    return scene, flat["trans"], prims, flat


def exact_scene(inputs):
    ex = exact_shade.ExactScene(inputs[0], inputs[1], inputs[3]["prim_type"])
    ex.set_tree(inputs[3]["kd_tree"])
    return ex


def make_batch(name, batch, workers, ex=None, inputs=None):
    scene, trans, prims, flat = inputs or scene_inputs(name)
    ex = ex or exact_scene((scene, trans, prims, flat))
    kinds = [material_kind(m) for m in flat_materials(scene)]
    rng = np.random.default_rng([23, SCENES.index(name), batches_of("lit15").index(batch)])
    extra = {}
    if batch == "camera":
        import exact_ref
        w, h = cam_size(name)
        cam = scene_camera(name, trans, prims)
        ys, xs = np.mgrid[0:h, 0:w]
        xy = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float64)
        eye, dirs = exact_ref.camera_rays(cam, w, h, xy)
        f = lambda v: [float(x) for x in v]
        o, d = np.array([f(eye)] * len(xy)), np.array([f(v) for v in dirs])   # rounded to f64, as the existing camera batch does: the rays ARE these f64 values
        rays = [(o[k], d[k]) for k in range(len(xy))]
        extra = dict(cam=np.array([*cam.eye, *cam.center, *cam.up, cam.fovy_radians], dtype=np.float64), size=np.array([w, h], dtype=np.int32))
        n = len(rays)
    else:
        n = dict(BATCHES)[batch]
        m = n + int(n * REPLACED_CAP)
        if batch == "random":
            o, d = batch_random(rng, m, name, trans, prims)
        elif batch == "inside":
            o, d = batch_inside(rng, m, name, trans, prims)
        elif name == "tangent":
            o, d, tag = batch_tangent(rng, m, trans, prims)
        else:
            prev = load(name, "random")
            o, d, tag = batch_special(rng, m, name, trans, prims, kinds, surface_points(ex, prev["o"], prev["d"]), ex, scene.lights)
        rays = [(o[k], d[k]) for k in range(m)]
    rows = evaluate(ex, rays, workers)
    if batch != "camera":   # every candidate up to the one that completes the count of usable rays
        good = [k for k in range(len(rows)) if not rows[k]["bad"]]
        assert len(good) >= n, (name, batch, "only %d of %d candidates are usable" % (len(good), len(rows)))
        keep = good[n - 1] + 1
        o, d, rows = o[:keep], d[:keep], rows[:keep]
        if batch == "special":
            extra["tag"] = tag[:keep]
    cols = columns(o, d, rows, kinds)
    cols.update(extra)
    cols["trans"] = np.ascontiguousarray(trans, dtype=np.float64)
    return cols


# ---------------------------------------------------------------- conditions, coverage and tolerances (numpy only)
def decidable(c, mode):
    ok = ~c["bad"]
    if mode == "kd":
        return ok & ~c["kd_fragile"]
    ok &= ~c["fragile"]
    return ok & ~c["hier_fragile"] if mode == "hier" else ok


def expected(c, mode):
    e = c["rgb"].copy()
    if mode == "kd":
        e[c["kd_idx"]] = c["kd_rgb"]
    return c["hier_rgb"].copy() if mode == "hier" else e


def agreement(exp, got, threshold):
    """Per ray: |got - exp| / max(1, |exp|) <= threshold on every channel."""
    with np.errstate(all="ignore"):
        return np.all(np.abs(got - exp) <= threshold * np.maximum(1.0, np.abs(exp)), axis=1)


def first_disagreement(c, exp, got, bad):
    k = int(np.flatnonzero(bad)[0])
    events = [e for i, e in enumerate(EVENTS) if int(c["events"][k]) >> i & 1]
    return ("ray %d o=%s d=%s: exact %s, got %s, error %.3g; depth-0 node %d (%s) branch %d, lights shadowed %#x, %d casts, deepest %d, tree: %s"
            % (k, c["o"][k].tolist(), c["d"][k].tolist(), exp[k].tolist(), got[k].tolist(), float(np.max(np.abs(got[k] - exp[k]))), c["node"][k],
               KIND_NAMES[c["kind"][k]] if c["kind"][k] >= 0 else "miss", c["branch"][k], int(c["shadow"][k, 0]), c["casts"][k], c["deepest"][k], ", ".join(events)))


def shares(batch, c):
    n = len(c["bad"])
    bad = int(c["bad"].sum())
    fragile = int((c["fragile"] & ~c["bad"]).sum())
    return dict(rays=n, bad=bad, replaced=bad / max(1, n - bad), fragile=(fragile + (bad if batch == "camera" else 0)) / n,
                kd_fragile=float((c["kd_fragile"] & ~c["bad"]).mean()), hier_fragile=float((c["hier_fragile"] & ~c["bad"]).mean()), kd_differs=len(c["kd_idx"]))


def check_conditions(scene, bs, log=print):
    for batch, c in bs.items():
        s = shares(batch, c)
        log("%-11s %-8s rays %3d  bad %2d  fragile %.4f  kd fragile %.4f  hier fragile %.4f  kd differs %d"
            % (scene, batch, s["rays"], s["bad"], s["fragile"], s["kd_fragile"], s["hier_fragile"], s["kd_differs"]))
        assert s["fragile"] <= FRAGILE_CAP[batch], (scene, batch, "fragile share", s["fragile"])
        if batch != "camera":
            assert s["replaced"] <= REPLACED_CAP, (scene, batch, "replaced share", s["replaced"])
            assert s["rays"] - s["bad"] == dict(BATCHES)[batch], (scene, batch, "usable rays", s["rays"] - s["bad"])
        ok = decidable(c, "flat")
        assert np.all(c["casts"][~c["bad"]] <= MAX_CASTS) and np.all(c["dev53"][ok] <= ILL), (scene, batch, "a usable ray is badly conditioned")
        hier = decidable(c, "hier")
        assert np.all(c["hier_same"][hier]), (scene, batch, "the hierarchical walk decides a decidable ray differently")
        assert np.all(c["hier_dev53"][hier] <= ILL) and agreement(c["rgb"][hier], c["hier_rgb"][hier], THRESHOLD_CAP).all(), (scene, batch, "hierarchical colours")
        assert np.array_equal(c["bg"], background(np.arange(len(ok)))), (scene, batch, "backgrounds")
        if batch == "special":
            check_constructed(scene, c, log)


def check_constructed(scene, c, log=print):
    """The constructed rays of a `special` batch do what they were built for, on the rays the exact reference can decide."""
    ok, kind, side, light = decidable(c, "flat"), c["tag"][:, 0], c["tag"][:, 1], c["tag"][:, 2].astype(np.uint64)
    crit = ok & (kind == TAG_CRITICAL)
    if scene == "hall":   # below the critical angle the ray leaves the cube (branch 3), above it is reflected (branch 4)
        assert int((crit & (side == 0)).sum()) >= 16 and int((crit & (side == 1)).sum()) >= 16, (scene, "critical-angle rays")
        assert np.all(c["branch"][crit & (side == 0)] == 3) and np.all(c["branch"][crit & (side == 1)] == 4), (scene, "critical-angle rays do not alternate")
        assert np.all(np.abs(np.linalg.norm(c["d"][crit], axis=1) - 1.0) <= 2.0 ** -50), (scene, "critical-angle rays are unit vectors")
    sil = ok & (kind == TAG_SILHOUETTE)
    bit = (c["shadow"][:, 0] >> light & np.uint64(1)) != 0
    assert np.all(bit[sil & (side == 0)]), (scene, "a ray 2^-20 inside a silhouette is not shadowed")
    out = sil & (side == 1)
    assert not np.any(bit[out]), (scene, "a ray 2^-20 outside a silhouette, with nothing else in the way, is shadowed")
    if scene in ("lit15", "lit_nested", "hall", "lit_tris"):
        assert int((sil & (side == 0)).sum()) >= 8 and int((out & ~bit).sum()) >= 8, (scene, "silhouette rays")
    tan = ok & (kind == TAG_TANGENT)
    if scene == "tangent":
        s0 = c["shadow"]
        on = (kind == TAG_TANGENT) & (side == 2) & ~c["bad"]
        assert int(on.sum()) >= 8 and np.all(c["fragile"][on]), (scene, "a light exactly on the tangent plane is not decidable, and is recorded as such")
        top, ground = tan & (side == 0) & (c["node"] == 0), tan & (side == 1) & (c["node"] == 1)
        assert int(top.sum()) >= COVER_MIN and int(ground.sum()) >= COVER_MIN, (scene, "tangent rays", int(top.sum()), int(ground.sum()))
        # behind the cube's face the light is hidden by the cube; behind the open plane it is seen with n.l < 0, in front of it with n.l > 0
        assert np.all(s0[top, 0] >> np.uint64(1) & np.uint64(1)), (scene, "the light behind the top face")
        assert np.all(s0[ground, 3] >> np.uint64(3) & np.uint64(1)), (scene, "the light behind the open plane")
        assert np.all(s0[ground, 2] >> np.uint64(2) & np.uint64(1)), (scene, "the light in front of the open plane")
    log("%-11s constructed: critical %d, silhouette %d inside / %d outside and lit, tangent %d; undecidable among the tagged %d"
        % (scene, int(crit.sum()), int((sil & (side == 0)).sum()), int((out & ~bit).sum()), int(tan.sum()), int((~ok & (kind != TAG_NONE) & (kind != TAG_NORMAL)).sum())))


def coverage(allb):
    """Counts over the decidable rays of all scenes together."""
    cat = lambda key: np.concatenate([c[key][decidable(c, "flat")] for bs in allb.values() for c in bs.values()])
    kind, events, shadow = cat("kind"), cat("events"), cat("shadow")
    out = {"depth-0 hit on " + KIND_NAMES[k]: int((kind == k).sum()) for k in range(5)}
    out["a light shadowed by a nearer occluder (depth 0)"] = int(((shadow[:, 0] & ~shadow[:, 1]) != 0).sum())
    out["a light shadowed only by occluders beyond it (depth 0)"] = int((shadow[:, 1] != 0).sum())
    out["an unshadowed light with n.l > 0 (depth 0)"] = int((shadow[:, 2] != 0).sum())
    out["an unshadowed light with n.l < 0 (depth 0)"] = int((shadow[:, 3] != 0).sum())
    for name, label in (("enter", "entering"), ("leave", "leaving"), ("tir", "total internal reflection"), ("depth11", "depth 11 reached"),
                        ("miss_deep", "a miss at depth >= 1"), ("glossy_z", "glossy offset: z-aligned branch"), ("glossy_xy", "glossy offset: other branch")):
        out[label] = int((events >> EVENTS.index(name) & 1).sum())
    out["a k-d answer that differs from the flat one"] = int(sum((decidable(c, "kd")[c["kd_idx"]]).sum() for bs in allb.values() for c in bs.values()))
    return out


def check_coverage(allb, log=print):
    cov = coverage(allb)
    for k, v in cov.items():
        log("%-58s %5d" % (k, v))
    short = {k: v for k, v in cov.items() if v < COVER_MIN}
    assert not short, "fewer than %d decidable rays: %r" % (COVER_MIN, short)
    return cov


def tolerances(allb):
    out = {}
    for scene, bs in allb.items():
        dev = 0.0
        for c in bs.values():
            ok = decidable(c, "flat")
            dev = max([dev] + c["dev53"][ok].astype(np.float64).tolist())
            okk = decidable(c, "kd")[c["kd_idx"]]
            dev = max([dev] + c["kd_dev53"][okk].tolist() + c["hier_dev53"][decidable(c, "hier")].astype(np.float64).tolist())
        out[scene] = {"deviation": float(dev), "threshold": float(SLACK * dev)}
        assert 0.0 < out[scene]["threshold"] <= THRESHOLD_CAP, (scene, out[scene])
    return out


def load_tolerances():
    with open(os.path.join(OUT, "tolerances.json")) as fh:
        return {k: v["threshold"] for k, v in json.load(fh)["scenes"].items()}


def load_all(scenes=SCENES):
    return {s: {b: load(s, b) for b in batches_of(s)} for s in scenes}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--batches", default="", help="only these batches of the scenes (the others are read from the files)")
    a = ap.parse_args()
    if a.check:
        scene, batch = CHECK_BATCH
        same = npz_bytes(make_batch(scene, batch, a.workers)) == open(path(scene, batch), "rb").read()
        print("%s_%s regenerated: %s" % (scene, batch, "byte-identical" if same else "DIFFERENT"))
        assert same
        allb = load_all()
        for s in SCENES:
            check_conditions(s, allb[s])
        check_coverage(allb)
        tol = tolerances(allb)
        assert tol == json.load(open(os.path.join(OUT, "tolerances.json")))["scenes"], "tolerances.json is stale"
        for s in SCENES:
            print(s, "threshold %.3g" % tol[s]["threshold"])
        return
    os.makedirs(OUT, exist_ok=True)
    t0 = time.time()
    for name in a.scenes.split(","):
        inputs = scene_inputs(name)
        ex = exact_scene(inputs)
        bs = {}
        for batch in batches_of(name):
            if a.batches and batch not in a.batches.split(","):
                bs[batch] = load(name, batch)
                continue
            bs[batch] = unpacked(make_batch(name, batch, a.workers, ex, inputs))
            with open(path(name, batch), "wb") as fh:
                fh.write(npz_bytes({k: v for k, v in make_cols(bs[batch]).items()}))
            print(name, batch, shares(batch, bs[batch]), os.path.getsize(path(name, batch)), "%.0f s" % (time.time() - t0), flush=True)
        check_conditions(name, bs)
    have = [s for s in SCENES if all(os.path.exists(path(s, b)) for b in batches_of(s))]
    allb = load_all(have)
    tol = tolerances(allb)
    with open(os.path.join(OUT, "tolerances.json"), "w") as fh:
        json.dump({"fragile_margin": FRAGILE, "slack": SLACK, "threshold_cap": THRESHOLD_CAP, "max_casts": MAX_CASTS, "scenes": tol}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(tol, indent=1))
    if have == list(SCENES):
        check_coverage(allb)
    print("generated in %.0f s with %d workers" % (time.time() - t0, a.workers))


STORED = ("rays", "rgb", "flags", "info", "shadow", "dev53", "hier_dev53", "hier_rgb", "kd", "trans", "cam", "size", "tag")


def make_cols(c):
    return {k: c[k] for k in STORED if k in c}


if __name__ == "__main__":
    main()
