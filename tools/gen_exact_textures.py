#!/usr/bin/env python3
"""Generates tests/golden/exact_textures/: textured and normal-mapped scenes, ray batches and the exact reference's colours for them.

    python tools/gen_exact_textures.py            # regenerate every file (deterministic, byte for byte)
    python tools/gen_exact_textures.py --check    # regenerate one batch and compare its bytes, re-assert the conditions, print shares and coverage

Built on tools/gen_exact_shading.py: its evaluation (every ray in the flat, k-d and hierarchical walks at 256 and at 53 bits), its columns, flags, caps,
tolerance rule and .npz writer are imported, not restated. What is new here: the textures (small byte images from an integer recurrence, kept in
textures.npz so that nothing depends on a random generator's version), five scenes whose materials carry textures, normal maps and uv_trans, the
constructed rays of the `special` batches, what is recorded of a ray's depth-0 lookups, and the coverage of the maps' branches.

Per ray, beside gen_exact_shading's columns: `tex_uv` (the depth-0 hit's tex_coord before and after uv_trans, rounded to f64), `texel` (indices and
bytes of the texture's texel, indices of the normal map's, the cube face), `to_top` (x and z of a normal-mapped sphere's or cube's to_top), `bary`
(a triangle's beta and gamma), `tex_margin` (the smallest margin of the depth-0 lookups' truncations) and `tex_events` (bits of exact_shade.TEX_EVENTS
over the whole ray tree).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_exact_rays as R  # noqa: E402
import gen_exact_shading as G  # noqa: E402
from scene_dsl import CUBE, MESH, PLANE, SPHERE, TRIANGLE, Camera, Cube, Light, Material, Mesh, MeshData, Node, Plane, Scene, Sphere, Texture, Triangle  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "exact_textures")
SCENES = ("tex_prims", "tex_nested", "tex_tris", "tex_mirror", "tex_glass")
BATCH_NAMES = ("camera", "random", "special")
COUNTS = {"random": 256, "special": 128}   # usable rays (gen_exact_shading.BATCHES has the same two)
CHECK_BATCH = ("tex_tris", "camera")
FRAGILE, SLACK, THRESHOLD_CAP, ILL, MAX_CASTS = G.FRAGILE, G.SLACK, G.THRESHOLD_CAP, G.ILL, G.MAX_CASTS
REPLACED_CAP, FRAGILE_CAP, COVER_MIN, KD_DEPTH = G.REPLACED_CAP, G.FRAGILE_CAP, G.COVER_MIN, G.KD_DEPTH
EPSILON = 0.00001
OFFSET = 2.0 ** -12                         # how far a constructed lookup lies from what it was aimed at, in texel units
TEX_EVENTS = ("tex_sphere", "tex_cube", "tex_plane", "tex_triangle", "tex_mesh", "nmap_sphere", "nmap_cube", "nmap_plane", "nmap_triangle", "nmap_mesh",
              "face_right", "face_left", "face_top", "face_bottom", "face_near", "face_far", "to_top_special", "to_top_general",
              "trunc_negative", "last_texel_from_above", "wrap_above", "mapped_deep", "nmap_faces_away")   # exact_shade.TEX_EVENTS
TEXEL = ("ix", "iy", "r", "g", "b", "nix", "niy", "face")
# what a ray of a `special` batch was built for; column `tag`: (kind, code, index). code: axis | side << 1 | image << 2 (image 1: the normal map's size)
TAG_FILL, TAG_EDGE, TAG_SEAM, TAG_BORDER, TAG_NEG, TAG_WRAP, TAG_TOP, TAG_TRI = 16, 17, 18, 19, 20, 21, 22, 23
TAG_NAMES = {TAG_EDGE: "texel edge", TAG_SEAM: "sphere seam", TAG_BORDER: "cube face border", TAG_NEG: "negative coordinate", TAG_WRAP: "wrap", TAG_TOP: "to-top",
             TAG_TRI: "triangle corner or edge"}

# ---------------------------------------------------------------- textures
TEXTURE_SIZES = (("t0", 7, 5), ("t1", 14, 12), ("t2", 16, 9), ("n0", 11, 6), ("n1", 10, 8))   # (w - 1) % 4 != 0 and (h - 1) % 3 != 0: no cube-map cell
                                                                                              # border falls on a texel edge


def make_textures():
    """Random bytes from a 64-bit linear congruential recurrence (plain integers). n0 is a normal map whose blue byte is at least 140 (its normals point
    out of the surface); n1's bytes are unconstrained: normals that point into the surface are legal in the reference."""
    out, state = {}, 0x9E3779B97F4A7C15
    for name, w, h in TEXTURE_SIZES:
        assert (w - 1) % 4 != 0 and (h - 1) % 3 != 0
        px = np.zeros((h, w, 3), dtype=np.uint8)
        for y in range(h):
            for x in range(w):
                for ch in range(3):
                    state = (state * 6364136223846793005 + 1442695040888963407) % (1 << 64)
                    byte = state >> 56
                    px[y, x, ch] = 140 + byte % 116 if name == "n0" and ch == 2 else byte
        out[name] = px
    return out


def textures_path():
    return os.path.join(OUT, "textures.npz")


def load_textures():
    with np.load(textures_path()) as z:
        return {k: Texture(np.ascontiguousarray(z[k])) for k in z.files}


# ---------------------------------------------------------------- scenes
U_ID = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
U_SCALE = (3.0, 0.0, -0.4, 0.0, 2.0, 0.3, 0.0, 0.0, 1.0)        # coordinates go negative and above 1
U_SKEW = (0.9, 0.35, -0.15, -0.4, 1.3, -0.1, 0.0, 0.0, 1.0)    # non-zero off-diagonals; both coordinates go negative
U_ROW3 = (1.25, 0.0, -0.1, 0.0, 0.75, 0.2, 0.5, -2.0, 3.0)     # a third row that must change nothing
TURN = G.HALL_TURN
to_world = G.hall_to_world


def _mat(diffuse, texture=None, normals=None, uv=U_ID, k=0, **kw):
    return Material(diffuse=diffuse, specular=(0.3, 0.25, 0.2), shininess=20.0 + 15.0 * k, texture=texture, normals=normals, uv_trans=uv, **kw)


def _turned(nodes, lights, ambient):
    """The scene is built on its own axes and turned about x, then y (gen_exact_shading's `hall`): no surface is parallel to a world axis."""
    return Scene(Node.group([Node.group(nodes).rotated_x(TURN[0]).rotated_y(TURN[1])]), lights, ambient)


def _two_lights():
    return [Light(position=to_world((2.5, 5.0, 4.0)), color=(0.9, 0.85, 0.8)),
            Light(position=to_world((-4.0, 3.0, -2.5)), color=(1.2, 1.3, 1.5), falloff=(1.0, 0.05, 0.01))]


def _prims_leaves(tx):
    m0 = _mat((0.5, 0.5, 0.5), tx["t0"], None, U_ID, 0)
    m1 = _mat((0.6, 0.3, 0.2), tx["t1"], tx["n0"], U_SCALE, 1)
    m2 = _mat((0.2, 0.5, 0.6), tx["t2"], tx["n1"], U_SKEW, 2)
    m3 = _mat((0.4, 0.6, 0.3), tx["t1"], tx["n0"], U_ROW3, 3)
    return [Node.geo(Plane(), m0).scaled((9.0, 1.0, 7.0)).rotated_y(0.3).translated((0.0, -1.2, 0.0)),
            Node.geo(Cube(), m1).scaled((1.6, 1.1, 0.9)).rotated_xzy((0.4, 0.7, -0.3)).translated((-1.8, 0.2, 0.3)),
            Node.geo(Sphere(), m2).scaled((1.0, 0.7, 1.3)).rotated_xzy((-0.5, 0.2, 0.6)).translated((1.6, 0.3, -0.4)),
            Node.geo(Cube(), m3).scaled((0.8, 1.4, 1.0)).rotated_xzy((-0.2, -0.9, 0.5)).translated((0.2, 0.4, -2.4)),
            Node.geo(Sphere(), m3).scaled((0.7, 0.9, 0.6)).rotated_xzy((0.8, -0.4, 0.1)).translated((-0.3, 0.1, 1.9)),
            Node.geo(Plane(), m2).scaled((1.8, 1.0, 1.4)).rotated_xzy((0.5, 0.0, -0.4)).translated((3.2, 0.6, 1.4))]


def scene_tex_prims(tx, lights=True):
    return _turned(_prims_leaves(tx), _two_lights() if lights else [], G.AMBIENT if lights else (1.0, 1.0, 1.0))


def scene_tex_nested(tx, lights=True):
    """The leaves of tex_prims, each placed as there, under two levels of transformed groups: the hierarchical walk transforms the ray three times."""
    lv = _prims_leaves(tx)
    g2 = Node.group([lv[2], lv[3]]).scaled((1.1, 0.9, 1.2)).rotated_xzy((0.3, -0.5, 0.2)).translated((0.4, 0.3, -0.2))
    g1 = Node.group([lv[0], lv[1], g2, lv[4], lv[5]]).scaled((0.9, 1.15, 1.05)).rotated_xzy((-0.15, 0.4, 0.1)).translated((-0.2, 0.1, 0.3))
    return _turned([g1], _two_lights() if lights else [], G.AMBIENT if lights else (1.0, 1.0, 1.0))


def grid_mesh():
    """A hand-written height field of 4 x 4 cells (32 triangles, 25 vertices) with texture coordinates and normals."""
    pos, nrm, tex, tris = [], [], [], []
    for j in range(5):
        for i in range(5):
            x, z = i / 4.0 - 0.5, j / 4.0 - 0.5
            pos.append((x, 0.3 * math.sin(3.0 * x) * math.cos(2.0 * z), z))
            n = np.array([-0.9 * math.cos(3.0 * x) * math.cos(2.0 * z), 1.0, 0.6 * math.sin(3.0 * x) * math.sin(2.0 * z)])
            nrm.append(tuple(n / np.linalg.norm(n)))
            tex.append((0.1 + 0.2 * i + 0.02 * j, 0.05 + 0.21 * j - 0.015 * i))
    for j in range(4):
        for i in range(4):
            a, b, c, d = 5 * j + i, 5 * j + i + 1, 5 * j + i + 6, 5 * j + i + 5
            tris += [(a, c, b), (a, d, c)]
    return MeshData(np.array(pos, dtype=np.float64), np.array(tris, dtype=np.uint32), np.array(nrm, dtype=np.float64), "grid", np.array(tex, dtype=np.float64))


def scene_tex_tris(tx, lights=True):
    grid = grid_mesh()
    both = Triangle((-1.0, 0.0, 0.4), (1.1, 0.1, 0.5), (0.1, 1.5, -0.2), normals=[(-0.3, 0.2, 1.0), (0.3, 0.1, 1.0), (0.0, 0.5, 0.9)],
                    tex_coords=[(0.05, 0.1), (0.95, 0.15), (0.45, 0.9)])
    coords = Triangle((-0.9, 0.0, 0.0), (0.8, -0.2, 0.3), (0.2, 1.2, 0.1), tex_coords=[(0.9, 0.2), (0.1, 0.3), (0.6, 0.85)])
    beyond = Triangle((-1.0, -0.1, 0.0), (1.2, 0.0, -0.3), (0.0, 1.4, 0.2), tex_coords=[(-0.6, -0.4), (1.7, 0.2), (0.4, 1.8)])   # beyond [0, 1] on both axes
    nodes = [Node.geo(both, _mat((0.5, 0.4, 0.3), tx["t1"], tx["n0"], U_ID, 0)).scaled((1.3, 0.9, 1.0)).rotated_xzy((0.2, 0.5, -0.1)).translated((-2.2, 0.2, 0.4)),
             Node.geo(coords, _mat((0.3, 0.5, 0.4), tx["t2"], tx["n1"], U_SKEW, 1)).scaled((1.1, 1.2, 0.8)).rotated_xzy((-0.3, -0.4, 0.2)).translated((0.1, 0.0, 1.2)),
             Node.geo(Mesh(grid), _mat((0.4, 0.4, 0.6), tx["t0"], tx["n1"], U_SCALE, 2)).scaled((2.4, 1.3, 1.9)).rotated_xzy((0.7, 0.3, 0.2)).translated((2.2, 0.3, -0.3)),
             Node.geo(Mesh(grid, smooth=True), _mat((0.6, 0.4, 0.4), tx["t1"], tx["n0"], U_ROW3, 3)).scaled((2.1, 1.6, 2.3)).rotated_xzy((0.9, -0.6, -0.2))
             .translated((-0.4, 0.5, -2.3)),
             Node.geo(beyond, _mat((0.5, 0.5, 0.2), tx["t0"], tx["n0"], U_ID, 4)).scaled((1.2, 1.0, 0.9)).rotated_xzy((0.1, 0.8, 0.3)).translated((0.3, 1.9, 0.2)),
             Node.geo(Plane(), _mat((0.5, 0.5, 0.5), tx["t2"], None, U_ID, 5)).scaled((10.0, 1.0, 8.0)).rotated_y(-0.2).translated((0.0, -1.3, 0.0))]
    return _turned(nodes, _two_lights() if lights else [], G.AMBIENT if lights else (1.0, 1.0, 1.0))


def scene_tex_mirror(tx, lights=True):
    """An opaque, textured, normal-mapped mirror (a plane on edge) facing textured objects: one secondary ray per hit."""
    mirror = _mat((0.1, 0.1, 0.12), tx["t0"], tx["n0"], U_SCALE, 0, reflectivity=0.7)
    nodes = [Node.geo(Plane(), mirror).scaled((7.0, 1.0, 4.5)).rotated_x(1.45).translated((0.0, 0.8, -2.2)),
             Node.geo(Sphere(), _mat((0.5, 0.3, 0.3), tx["t2"], tx["n1"], U_SKEW, 1)).scaled((0.9, 0.7, 0.8)).rotated_xzy((0.3, 0.2, -0.5)).translated((-1.4, 0.2, 0.1)),
             Node.geo(Cube(), _mat((0.3, 0.5, 0.3), tx["t1"], tx["n0"], U_ROW3, 2)).scaled((1.2, 0.9, 1.0)).rotated_xzy((-0.3, 0.6, 0.2)).translated((1.3, 0.0, 0.3)),
             Node.geo(Plane(), _mat((0.5, 0.5, 0.5), tx["t1"], None, U_ID, 3)).scaled((9.0, 1.0, 8.0)).rotated_y(0.4).translated((0.0, -1.0, 0.5))]
    return _turned(nodes, _two_lights() if lights else [], G.AMBIENT if lights else (1.0, 1.0, 1.0))


def scene_tex_glass(tx, lights=True):
    """A textured, normal-mapped glass cube and sphere over a textured floor, under one light (a glass hit casts twice, so the ray trees grow fast)."""
    glass = lambda d, t, n, uv, k: _mat(d, t, n, uv, k, reflectivity=0.9, refraction_index=G.GLASS)
    nodes = [Node.geo(Cube(), glass((0.05, 0.1, 0.08), tx["t1"], tx["n0"], U_SCALE, 0)).scaled((1.1, 0.9, 1.0)).rotated_xzy((0.2, 0.5, -0.1)).translated((-1.1, -0.2, 0.2)),
             Node.geo(Sphere(), glass((0.1, 0.05, 0.05), tx["t2"], tx["n0"], U_ROW3, 1)).scaled((0.7, 0.6, 0.65)).rotated_xzy((-0.4, 0.3, 0.2)).translated((1.1, 0.3, -0.3)),
             Node.geo(Plane(), _mat((0.5, 0.5, 0.5), tx["t0"], tx["n1"], U_SKEW, 2)).scaled((8.0, 1.0, 7.0)).rotated_y(0.25).translated((0.0, -1.0, 0.0))]
    light = [Light(position=to_world((1.5, 4.5, 3.0)), color=(0.9, 0.9, 0.85))]
    return _turned(nodes, light if lights else [], G.AMBIENT if lights else (1.0, 1.0, 1.0))


def build_scene(name, lights=True, textures=None):
    """lights=False: the same scene with ambient (1, 1, 1) and no lights, in which a non-reflective hit's colour is its diffuse colour."""
    tx = textures or load_textures()
    return {"tex_prims": scene_tex_prims, "tex_nested": scene_tex_nested, "tex_tris": scene_tex_tris, "tex_mirror": scene_tex_mirror,
            "tex_glass": scene_tex_glass}[name](tx, lights)


def scene_camera():
    """Every scene is seen from the same place on its own axes, turned with it; most eye rays meet a mapped surface."""
    return Camera(eye=to_world((3.0, 2.6, 6.5)), center=to_world((0.0, -0.2, 0.0)), up=to_world((0.0, 1.0, 0.0)), fovy_degrees=45.0)


def image_sizes(scene):
    """Per flattened node: ((w, h) of the texture or None, (w, h) of the normal map or None)."""
    size = lambda t: None if t is None else (int(t.pixels.shape[1]), int(t.pixels.shape[0]))
    return [(size(m.texture), size(m.normals)) for m in G.flat_materials(scene)]


# ---------------------------------------------------------------- constructed rays (plain f64: what they reach is asserted from the exact values)
CUBE_FACES = ((0, 1.0, (-1.0, 1.0), (1.0 / 2.0, 1.0 / 3.0)), (0, -1.0, (1.0, 1.0), (0.0, 1.0 / 3.0)), (1, 1.0, (1.0, -1.0), (1.0 / 4.0, 0.0)),
              (1, -1.0, (1.0, 1.0), (1.0 / 4.0, 2.0 / 3.0)), (2, 1.0, (1.0, 1.0), (1.0 / 4.0, 1.0 / 3.0)), (2, -1.0, (-1.0, 1.0), (3.0 / 4.0, 1.0 / 3.0)))


def _triangle_of(prim, sub):
    if prim.kind == TRIANGLE:
        return prim.tri, prim.tri_tex_coords
    ids = [int(q) for q in prim.mesh.triangles[sub]]
    return prim.mesh.positions[ids], prim.mesh.tex_coords[ids]


def point_from_uv(prim, ctx, u, v):
    """The model-space point and normal with tex_coord (u, v) on the face or triangle `ctx`, or None outside the surface."""
    if prim.kind == SPHERE:
        if not (0.0 < u < 1.0 and 0.0 < v < 1.0):
            return None
        th, y, r = 2.0 * math.pi * u - math.pi, math.cos(math.pi * v), math.sin(math.pi * v)
        p = np.array([r * math.cos(th), y, -r * math.sin(th)])
        return p, p.copy()
    if prim.kind == PLANE:
        if not (0.0 <= u <= 1.0 and 0.0 <= v <= 1.0):
            return None
        return np.array([u - 0.5, 0.0, v - 0.5]), np.array([0.0, 1.0, 0.0])
    if prim.kind == CUBE:
        axis, s, ax, off = CUBE_FACES[ctx]
        nu, nv = (u - off[0]) * 4.0, (v - off[1]) * 3.0
        if not (0.0 < nu < 1.0 and 0.0 < nv < 1.0):
            return None
        fu, fv = (nu - 0.5) / ax[0], (0.5 - nv) / ax[1]
        p = (np.array([s / 2, fv, fu]), np.array([fu, s / 2, fv]), np.array([fu, fv, s / 2]))[axis]
        n = np.zeros(3)
        n[axis] = s
        return p, n
    tri, tc = _triangle_of(prim, ctx)
    m = np.array([[tc[1][0] - tc[0][0], tc[2][0] - tc[0][0]], [tc[1][1] - tc[0][1], tc[2][1] - tc[0][1]]])
    beta, gamma = np.linalg.solve(m, np.array([u - tc[0][0], (1.0 - v) - tc[0][1]]))
    if beta < 0.0 or gamma < 0.0 or beta + gamma > 1.0:
        return None
    return from_bary(prim, ctx, beta, gamma)[:2]


def from_bary(prim, ctx, beta, gamma):
    tri, tc = _triangle_of(prim, ctx)
    p = tri[0] + beta * (tri[1] - tri[0]) + gamma * (tri[2] - tri[0])
    uv = tc[0] * (1.0 - beta - gamma) + tc[1] * beta + tc[2] * gamma
    return p, np.cross(tri[1] - tri[0], tri[2] - tri[0]), (float(uv[0]), 1.0 - float(uv[1]))


def random_surface(rng, prim):
    """(ctx, u, v) of a random point of the surface."""
    if prim.kind in (SPHERE, PLANE):
        return 0, float(rng.uniform(0.01, 0.99)), float(rng.uniform(0.01, 0.99))
    if prim.kind == CUBE:
        f = int(rng.integers(6))
        off = CUBE_FACES[f][3]
        return f, off[0] + float(rng.uniform(0.01, 0.99)) / 4.0, off[1] + float(rng.uniform(0.01, 0.99)) / 3.0
    sub = int(rng.integers(len(prim.mesh.triangles))) if prim.kind == MESH else 0
    b, g = sorted(rng.uniform(0.02, 0.98, 2))
    _, _, uv = from_bary(prim, sub, float(b), float(g - b))
    return sub, uv[0], uv[1]


def transformed(uvt, u, v):
    return uvt[0] * u + uvt[1] * v + uvt[2], uvt[3] * u + uvt[4] * v + uvt[5]


def untransformed(uvt, tu, tv):
    return tuple(np.linalg.solve(np.array([[uvt[0], uvt[1]], [uvt[3], uvt[4]]]), np.array([tu - uvt[2], tv - uvt[5]])))


class Builder:
    def __init__(self, rng, ex, scene, trans, prims):
        self.rng, self.ex, self.trans, self.prims = rng, ex, trans, prims
        self.mats = G.flat_materials(scene)
        self.sizes = image_sizes(scene)

    def ray_to(self, i, ctx, p, n):
        """A ray that meets node i first, at model point p: from a point off the surface along its normal, tilted; either side of an open surface."""
        rng, t = self.rng, self.trans[i]
        world = R._to_world(t, p)
        wn = np.linalg.inv(t[:3, :3]).T @ n
        wn = wn / np.linalg.norm(wn)
        for side in ((1.0,) if self.prims[i].kind in (SPHERE, CUBE) else (1.0, -1.0)):
            rho = float(rng.uniform(0.3, 0.8))
            o = world + side * wn * rho + R._perp(rng, wn) * rho * float(rng.uniform(0.0, 0.4))
            d = (world - o) * 2.0 ** int(rng.integers(-2, 3))
            h = self.ex.cast(o, d, prec=53)
            if h and h.node == i and (self.prims[i].kind != CUBE or h.part == ctx) and (self.prims[i].kind != MESH or h.sub == ctx):
                return o, d
        return None

    def size(self, i, image):
        return self.sizes[i][1] if image and self.sizes[i][1] else (self.sizes[i][0] or self.sizes[i][1])

    def find(self, i, accept, tries=1500):
        """A random surface point of node i whose transformed coordinates pass accept(tu, tv)."""
        for _ in range(tries):
            ctx, u, v = random_surface(self.rng, self.prims[i])
            if accept(*transformed(self.mats[i].uv_trans, u, v)):
                return ctx, u, v
        return None

    def at(self, i, ctx, u, v):
        got = point_from_uv(self.prims[i], ctx, u, v)
        return None if got is None else self.ray_to(i, ctx, got[0], got[1])

    def edge(self, i, axis, side, image):
        """A lookup 2^-12 below (side 0) or above (side 1) an integer of the untruncated coordinate on `axis`, the other coordinate away from one."""
        w = self.size(i, image)
        ctx, u, v = random_surface(self.rng, self.prims[i])
        t = list(transformed(self.mats[i].uv_trans, u, v))
        f = [t[0] * (w[0] - 1), t[1] * (w[1] - 1)]
        f[axis] = round(f[axis]) + (OFFSET if side else -OFFSET)
        other = f[1 - axis] - math.floor(f[1 - axis])
        if other < 0.1 or other > 0.9:
            return None
        uu, vv = untransformed(self.mats[i].uv_trans, f[0] / (w[0] - 1), f[1] / (w[1] - 1))
        return self.at(i, ctx, uu, vv)

    def seam(self, i, side):
        return self.at(i, 0, 2.0 ** -14 if side else 1.0 - 2.0 ** -14, float(self.rng.uniform(0.2, 0.8)))

    def border(self, i, face, axis, side):
        """2^-12 texels (of the texture, under an identity uv_trans) inside a cube face's border in the cube map."""
        w = self.size(i, 0)
        n = [float(self.rng.uniform(0.1, 0.9)), float(self.rng.uniform(0.1, 0.9))]
        eps = OFFSET * (4.0, 3.0)[axis] / (w[axis] - 1)
        n[axis] = 1.0 - eps if side else eps
        off = CUBE_FACES[face][3]
        return self.at(i, face, off[0] + n[0] / 4.0, off[1] + n[1] / 3.0)

    def window(self, i, axis, lo, hi):
        """The untruncated coordinate on `axis` in [lo + 0.1, hi - 0.1], the other away from an integer."""
        w = self.size(i, 0)

        def accept(tu, tv):
            f = (tu * (w[0] - 1), tv * (w[1] - 1))
            other = f[1 - axis] - math.floor(f[1 - axis])
            return lo + 0.1 <= f[axis] <= hi - 0.1 and 0.1 <= other <= 0.9
        got = self.find(i, accept)
        return None if got is None else self.at(i, *got)

    def top(self, i, side):
        """A normal-mapped sphere or cube hit whose to_top has |x|, |z| < EPSILON (side 0: near the sphere's lower pole, the centre of the cube's top or
        bottom face), or a sphere hit with to_top.x 2^-12 (relative) above EPSILON (side 1)."""
        rng, prim = self.rng, self.prims[i]
        if prim.kind == CUBE:
            s = 1.0 if rng.random() < 0.5 else -1.0
            dist = 0.5 if s > 0 else 1.5
            p = np.array([rng.uniform(-0.6, 0.6) * EPSILON * dist, s / 2, rng.uniform(-0.6, 0.6) * EPSILON * dist])
            return self.ray_to(i, 2 if s > 0 else 3, p, np.array([0.0, s, 0.0]))
        if side == 0:
            x, z = rng.uniform(-1.2, 1.2, 2) * EPSILON   # to_top = (-x, 1 - y, -z) / about 2
        else:
            x, z = 2.0 * EPSILON * (1.0 + OFFSET) * (1.0 if rng.random() < 0.5 else -1.0), float(rng.uniform(-1.0, 1.0)) * EPSILON
        y = -math.sqrt(1.0 - x * x - z * z)
        p = np.array([x, y, z])
        if side == 1:   # |to_top.x| = |x| / |(0, 1, 0) - p|: solved for x
            length = math.sqrt(x * x + (1.0 - y) ** 2 + z * z)
            p[0] = math.copysign(EPSILON * (1.0 + OFFSET) * length, x)
            p[1] = -math.sqrt(1.0 - p[0] * p[0] - z * z)
        return self.ray_to(i, 0, p, p.copy())

    def corner_or_edge(self, i, which):
        """Within 2^-12 (barycentric) of corner a, b, c (0-2) or of the edge beta = 0, gamma = 0, alpha = 0 (3-5)."""
        prim = self.prims[i]
        sub = int(self.rng.integers(len(prim.mesh.triangles))) if prim.kind == MESH else 0
        e, r = OFFSET / 2, float(self.rng.uniform(0.2, 0.6))
        beta, gamma = ((e, e), (1.0 - 2 * e, e), (e, 1.0 - 2 * e), (e, r), (r, e), (r, 1.0 - r - e))[which]
        p, n, _ = from_bary(prim, sub, beta, gamma)
        return self.ray_to(i, sub, p, n)


def batch_special(rng, m, ex, scene, trans, prims):
    """Constructed rays, tagged; what each reaches is asserted by check_tags from the exact values."""
    b = Builder(rng, ex, scene, trans, prims)
    n = len(prims)
    kinds = [p.kind for p in prims]
    nmapped = [i for i in range(n) if b.sizes[i][1]]
    plan = []
    for i in range(n):   # both axes, both sides, on every primitive; with the normal map's size too where there is one
        for image in ((0, 1) if b.sizes[i][0] and b.sizes[i][1] else (0,)):
            for axis in (0, 1):
                for side in (0, 1):
                    plan.append((TAG_EDGE, axis | side << 1 | image << 2, i, lambda i=i, a=axis, s=side, im=image: b.edge(i, a, s, im)))
    for i in [i for i in range(n) if kinds[i] == SPHERE]:
        for side in (0, 1, 0, 1):
            plan.append((TAG_SEAM, side << 1, i, lambda i=i, s=side: b.seam(i, s)))
    for i in [i for i in range(n) if kinds[i] == CUBE][:1]:
        for face in range(6):
            for axis in (0, 1):
                for side in (0, 1):
                    plan.append((TAG_BORDER, axis | side << 1, face, lambda i=i, f=face, a=axis, s=side: b.border(i, f, a, s)))
    for rep in range(5):
        for axis in (0, 1):
            for i in range(n):
                w = b.size(i, 0)
                plan.append((TAG_NEG, axis, i, lambda i=i, a=axis: b.window(i, a, -1.0, 0.0)))
                plan.append((TAG_WRAP, axis, i, lambda i=i, a=axis, w=w: b.window(i, a, w[a] - 1.0, float(w[a]))))
                plan.append((TAG_WRAP, axis | 2, i, lambda i=i, a=axis, w=w: b.window(i, a, float(w[a]), w[a] + 1.0)))
    tops = [i for i in nmapped if kinds[i] in (SPHERE, CUBE)]
    for rep in range(8):
        for i in tops:
            plan.append((TAG_TOP, 0, i, lambda i=i: b.top(i, 0)))
            if kinds[i] == SPHERE and rep < 3:
                plan.append((TAG_TOP, 2, i, lambda i=i: b.top(i, 1)))
    for i in [i for i in range(n) if kinds[i] in (TRIANGLE, MESH)]:
        for which in range(6):
            plan.append((TAG_TRI, which, i, lambda i=i, w=which: b.corner_or_edge(i, w)))
    # the constructed kinds take turns, so that every kind is in the batch whatever its length
    order, by_kind = [], {}
    for item in plan:
        by_kind.setdefault(item[0], []).append(item)
    budget = {TAG_EDGE: 40, TAG_SEAM: 8, TAG_BORDER: 24, TAG_NEG: 14, TAG_WRAP: 24, TAG_TOP: 22, TAG_TRI: 30}
    o, d, tag = [], [], []
    for kind in sorted(by_kind):
        made = 0
        for item in by_kind[kind]:
            if made >= budget[kind] or len(o) >= m:
                break
            for _ in range(3):
                ray = item[3]()
                if ray is not None:
                    o.append(ray[0]); d.append(ray[1]); tag.append((item[0], item[1], item[2]))
                    made += 1
                    break
    mapped = [i for i in range(n) if b.sizes[i][0] or b.sizes[i][1]]
    while len(o) < m:   # the rest: texel edges on random primitives
        i, axis, side = mapped[int(rng.integers(len(mapped)))], int(rng.integers(2)), int(rng.integers(2))
        image = int(rng.integers(2)) if b.sizes[i][0] and b.sizes[i][1] else 0
        ray = b.edge(i, axis, side, image)
        if ray is not None:
            o.append(ray[0]); d.append(ray[1]); tag.append((TAG_EDGE, axis | side << 1 | image << 2, i))
    p = rng.permutation(len(o))   # a ray left out as badly conditioned is made up for by the candidates behind the count: no kind sits at the end
    return np.array(o)[p], np.array(d)[p], np.array(tag, dtype=np.int8).reshape(len(o), 3)[p]


def batch_random(rng, m, trans, prims):
    """Rays from around the scene aimed into the objects, direction lengths 2^-3 to 2^3 (gen_exact_shading.batch_random without the halls' case)."""
    return G.batch_random(rng, m, "", trans, prims)


# ---------------------------------------------------------------- evaluation
def extra(f):
    """What is recorded of the flat 256-bit evaluation's maps (gen_exact_shading.EXTRA)."""
    t = f.tex0
    nan = float("nan")
    r = dict(tex_events=int(f.tex_events), tex_uv=[nan] * 4, texel=[-1] * 8, to_top=[nan, nan], bary=[nan, nan], tex_margin=nan)
    if t is not None:
        r["tex_margin"] = min(float(t["margin"]), 1.0)
        r["tex_uv"] = [float(t["uv"][0]), float(t["uv"][1]), float(t["tuv"][0]), float(t["tuv"][1])]
        tx, nm = t["texel"] or (-1,) * 5, t["nmap_texel"] or (-1,) * 5
        r["texel"] = [*tx, nm[0], nm[1], t["face"]]
        if t["to_top"] is not None:
            r["to_top"] = [float(t["to_top"][0]), float(t["to_top"][2])]
        if t.get("bary") is not None:
            r["bary"] = [float(t["bary"][0]), float(t["bary"][1])]
    return r


def columns(o, d, rows, kinds):
    c = G.columns(o, d, rows, kinds)
    n = len(rows)
    nan = float("nan")
    c["tex_events"] = np.array([r.get("tex_events", 0) for r in rows], dtype=np.int32)
    c["tex_uv"] = np.array([r.get("tex_uv", [nan] * 4) for r in rows], dtype=np.float64).reshape(n, 4)
    c["texel"] = np.array([r.get("texel", [-1] * 8) for r in rows], dtype=np.int16).reshape(n, 8)
    c["to_top"] = np.array([r.get("to_top", [nan] * 2) for r in rows], dtype=np.float64).reshape(n, 2)
    c["bary"] = np.array([r.get("bary", [nan] * 2) for r in rows], dtype=np.float64).reshape(n, 2)
    c["tex_margin"] = np.array([r.get("tex_margin", nan) for r in rows], dtype=np.float32)
    return c


STORED = G.STORED + ("tex_events", "tex_uv", "texel", "to_top", "bary", "tex_margin")


def path(scene, batch):
    return os.path.join(OUT, "%s_%s.npz" % (scene, batch))


def load(scene, batch):
    with np.load(path(scene, batch)) as z:
        return G.unpacked({k: z[k] for k in z.files})


def load_all(scenes=SCENES):
    return {s: {b: load(s, b) for b in BATCH_NAMES} for s in scenes}


def scene_inputs(name, textures=None):
    import oracle_lib
    scene = build_scene(name, textures=textures)
    ps = oracle_lib.pack(scene)
    flat = oracle_lib.flatten(ps)
    prims = R.flat_prims(scene)
    assert [p.kind for p in prims] == [int(k) for k in flat["prim_type"]] and len(prims) <= 12
    flat["kd_tree"] = oracle_lib.kd_scene_dump(ps, kd_depth=KD_DEPTH)
    return scene, flat["trans"], prims, flat


def make_batch(name, batch, workers, ex=None, inputs=None):
    scene, trans, prims, flat = inputs or scene_inputs(name)
    ex = ex or G.exact_scene((scene, trans, prims, flat))
    kinds = [G.material_kind(m) for m in G.flat_materials(scene)]
    rng = np.random.default_rng([29, SCENES.index(name), BATCH_NAMES.index(batch)])
    more = {}
    if batch == "camera":
        import exact_ref
        w, h = G.CAM_W, G.CAM_H
        cam = scene_camera()
        ys, xs = np.mgrid[0:h, 0:w]
        xy = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float64)
        eye, dirs = exact_ref.camera_rays(cam, w, h, xy)
        o = np.array([[float(x) for x in eye]] * len(xy))
        d = np.array([[float(x) for x in v] for v in dirs])   # the rays ARE these f64 values
        more = dict(cam=np.array([*cam.eye, *cam.center, *cam.up, cam.fovy_radians], dtype=np.float64), size=np.array([w, h], dtype=np.int32))
        n = len(o)
    else:
        n = COUNTS[batch]
        m = n + int(n * REPLACED_CAP)
        if batch == "random":
            o, d = batch_random(rng, m, trans, prims)
        else:
            o, d, tag = batch_special(rng, m, ex, scene, trans, prims)
    G.EXTRA = extra
    try:
        rows = G.evaluate(ex, [(o[k], d[k]) for k in range(len(o))], workers)
    finally:
        G.EXTRA = None
    if batch != "camera":   # every candidate up to the one that completes the count of usable rays
        good = [k for k in range(len(rows)) if not rows[k]["bad"]]
        assert len(good) >= n, (name, batch, "only %d of %d candidates are usable" % (len(good), len(rows)))
        keep = good[n - 1] + 1
        o, d, rows = o[:keep], d[:keep], rows[:keep]
        if batch == "special":
            more["tag"] = tag[:keep]
    cols = columns(o, d, rows, kinds)
    cols.update(more)
    cols["trans"] = np.ascontiguousarray(trans, dtype=np.float64)
    return cols


# ---------------------------------------------------------------- conditions and coverage (numpy only)
def texel_bytes(c):
    """Per ray: the exact texel's three bytes at the depth-0 hit, and whether that hit is textured."""
    t = c["texel"]
    return t[:, 2:5].astype(np.int32), t[:, 2] >= 0


def check_tags(scene_name, c, scene=None, log=print):
    """Every constructed ray that the exact reference can decide reached what it was built for, by the exact values."""
    scene = scene or build_scene(scene_name)
    sizes, kinds = image_sizes(scene), [p.kind for p in R.flat_prims(scene)]
    ok = G.decidable(c, "flat")
    tag, uv, texel, ev = c["tag"], c["tex_uv"], c["texel"], c["tex_events"]
    bit = lambda name: (ev >> TEX_EVENTS.index(name) & 1) != 0
    seen = {}
    near = lambda x, lo=OFFSET / 2, hi=OFFSET * 2: lo <= x <= hi
    for k in np.flatnonzero(ok & (tag[:, 0] > TAG_FILL)):
        kind, code, index = (int(x) for x in tag[k])
        node = int(c["node"][k])
        what = (scene_name, k, TAG_NAMES[kind], code, index)
        axis, side, image = code & 1, code >> 1 & 1, code >> 2 & 1
        if kind in (TAG_EDGE, TAG_NEG, TAG_WRAP, TAG_SEAM, TAG_TOP, TAG_TRI):
            assert node == index, what + ("hit node", node)
            w = sizes[node][1] if image and sizes[node][1] else (sizes[node][0] or sizes[node][1])
            f = float(uv[k, 2 + axis]) * (w[axis] - 1)
            # the index recorded is the texture's where there is one, else the normal map's (the size used above)
            idx = int(texel[k, axis]) if sizes[node][0] else int(texel[k, 5 + axis])
        if kind == TAG_EDGE:
            assert near(f - round(f)) if side else near(round(f) - f), what + (f,)
            seen[kind, kinds[node], axis, side] = seen.get((kind, kinds[node], axis, side), 0) + 1
        elif kind == TAG_SEAM:
            assert kinds[node] == SPHERE and (0.0 < uv[k, 0] < 2.0 ** -13 if side else 1.0 - 2.0 ** -13 < uv[k, 0] < 1.0), what + (uv[k, 0],)
            seen[kind, side] = seen.get((kind, side), 0) + 1
        elif kind == TAG_BORDER:
            assert kinds[node] == CUBE and int(texel[k, 7]) == index and bit(TEX_EVENTS[10 + index])[k], what + ("face", int(texel[k, 7]))
            off, w = CUBE_FACES[index][3], sizes[node][0]
            nrm = ((uv[k, 0] - off[0]) * 4.0, (uv[k, 1] - off[1]) * 3.0)[axis] * (w[axis] - 1) / (4.0, 3.0)[axis]   # in texels from the face's border
            full = (w[axis] - 1) / (4.0, 3.0)[axis]
            assert near(full - nrm) if side else near(nrm), what + (nrm, full)
            seen[kind, index] = seen.get((kind, index), 0) + 1
        elif kind == TAG_NEG:   # truncation is not floor: (-1, 0) is texel 0, not w - 1
            assert -1.0 < f < 0.0 and idx == 0 and bit("trunc_negative")[k], what + (f, idx)
            seen[kind, axis] = seen.get((kind, axis), 0) + 1
        elif kind == TAG_WRAP:  # the wrap is modulo w: [w - 1, w) is texel w - 1, [w, w + 1) is texel 0
            if side == 0:
                assert w[axis] - 1 <= f < w[axis] and idx == w[axis] - 1 and bit("last_texel_from_above")[k], what + (f, idx)
            else:
                assert w[axis] <= f < w[axis] + 1 and idx == 0 and bit("wrap_above")[k], what + (f, idx)
            seen[kind, axis, side] = seen.get((kind, axis, side), 0) + 1
        elif kind == TAG_TOP:
            x, z = abs(float(c["to_top"][k, 0])), abs(float(c["to_top"][k, 1]))
            if side == 0:
                assert x < EPSILON and z < EPSILON and bit("to_top_special")[k], what + (x, z)
            else:
                assert kinds[node] == SPHERE and near(x / EPSILON - 1.0) and bit("to_top_general")[k], what + (x, z)
            seen[kind, side] = seen.get((kind, side), 0) + 1
        elif kind == TAG_TRI:
            beta, gamma = (float(x) for x in c["bary"][k])
            alpha = 1.0 - beta - gamma
            small = lambda x: 0.0 < x < OFFSET
            assert kinds[node] in (TRIANGLE, MESH) and ((small(beta) and small(gamma)), (small(alpha) and small(gamma)), (small(alpha) and small(beta)),
                                                        small(beta), small(gamma), small(alpha))[code], what + (beta, gamma)
            seen[kind, code] = seen.get((kind, code), 0) + 1
    have = set(kinds)
    want = [(TAG_EDGE, kd, a, s) for kd in have for a in (0, 1) for s in (0, 1)] + [(TAG_NEG, a) for a in (0, 1)] + [(TAG_WRAP, a, s) for a in (0, 1) for s in (0, 1)]
    if SPHERE in have:
        want += [(TAG_SEAM, 0), (TAG_SEAM, 1)]
        if any(kinds[i] == SPHERE and sizes[i][1] for i in range(len(kinds))):
            want += [(TAG_TOP, 0), (TAG_TOP, 1)]
    if CUBE in have:
        want += [(TAG_BORDER, f) for f in range(6)]   # every face index is reached
    if TRIANGLE in have or MESH in have:
        want += [(TAG_TRI, q) for q in range(6)]
    missing = [w for w in want if not seen.get(w)]
    assert not missing, (scene_name, "no decidable constructed ray for", [(TAG_NAMES[w[0]],) + w[1:] for w in missing])
    # by construction the offsets lie far above the fragile limit: a tagged ray is left out only for other reasons (recursion, a silhouette)
    tagged = tag[:, 0] > TAG_FILL
    aimed = tagged & ~c["bad"] & (texel[:, 0] >= 0)
    assert int(aimed.sum()) >= 0.9 * int(tagged.sum()) and np.all(c["tex_margin"][aimed] >= OFFSET / 64), (scene_name, "a constructed lookup is not decidable",
                                                                                                         float(np.min(c["tex_margin"][aimed])))
    log("%-11s constructed: %s; undecidable among the tagged %d of %d"
        % (scene_name, ", ".join("%s %d" % (TAG_NAMES[kd], sum(v for q, v in seen.items() if q[0] == kd)) for kd in sorted(TAG_NAMES)),
           int((tagged & ~ok).sum()), int(tagged.sum())))


def check_conditions(scene_name, bs, log=print):
    G.check_conditions(scene_name, bs, log)   # the caps, the counts, the conditioning, the hierarchical walk, the backgrounds
    scene = build_scene(scene_name)
    for batch, c in bs.items():
        assert len(c["o"]) <= 540
        hit_mapped = c["texel"][:, 0] >= 0
        assert np.all(np.isfinite(c["tex_uv"][hit_mapped & ~c["bad"] & ~c["fragile"]])), (scene_name, batch)
    check_tags(scene_name, bs["special"], scene, log)


def coverage(allb):
    """Decidable rays per branch of the maps, over all scenes together."""
    ev = np.concatenate([c["tex_events"][G.decidable(c, "flat")] for bs in allb.values() for c in bs.values()])
    return {name: int((ev >> k & 1).sum()) for k, name in enumerate(TEX_EVENTS)}


def check_coverage(allb, log=print):
    cov = coverage(allb)
    for k, v in cov.items():
        log("%-24s %5d" % (k, v))
    short = {k: v for k, v in cov.items() if v < COVER_MIN}
    assert not short, "fewer than %d decidable rays: %r" % (COVER_MIN, short)
    return cov


def load_tolerances():
    with open(os.path.join(OUT, "tolerances.json")) as fh:
        return {k: v["threshold"] for k, v in json.load(fh)["scenes"].items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--batches", default="", help="only these batches of the scenes (the others are read from the files)")
    a = ap.parse_args()
    if a.check:
        scene, batch = CHECK_BATCH
        same = G.npz_bytes({k: v for k, v in make_batch(scene, batch, a.workers).items() if k in STORED}) == open(path(scene, batch), "rb").read()
        print("%s_%s regenerated: %s" % (scene, batch, "byte-identical" if same else "DIFFERENT"))
        assert same
        allb = load_all()
        for s in SCENES:
            check_conditions(s, allb[s])
        check_coverage(allb)
        tol = G.tolerances(allb)
        assert tol == json.load(open(os.path.join(OUT, "tolerances.json")))["scenes"], "tolerances.json is stale"
        for s in SCENES:
            print(s, "threshold %.3g" % tol[s]["threshold"])
        return
    os.makedirs(OUT, exist_ok=True)
    t0 = time.time()
    tx = make_textures()
    with open(textures_path(), "wb") as fh:
        fh.write(G.npz_bytes(tx))
    for name in a.scenes.split(","):
        inputs = scene_inputs(name)
        ex = G.exact_scene(inputs)
        bs = {}
        for batch in BATCH_NAMES:
            if a.batches and batch not in a.batches.split(","):
                bs[batch] = load(name, batch)
                continue
            cols = {k: v for k, v in make_batch(name, batch, a.workers, ex, inputs).items() if k in STORED}
            with open(path(name, batch), "wb") as fh:
                fh.write(G.npz_bytes(cols))
            bs[batch] = load(name, batch)
            print(name, batch, G.shares(batch, bs[batch]), os.path.getsize(path(name, batch)), "%.0f s" % (time.time() - t0), flush=True)
        check_conditions(name, bs)
    have = [s for s in SCENES if all(os.path.exists(path(s, b)) for b in BATCH_NAMES)]
    allb = load_all(have)
    tol = G.tolerances(allb)
    with open(os.path.join(OUT, "tolerances.json"), "w") as fh:
        json.dump({"fragile_margin": FRAGILE, "slack": SLACK, "threshold_cap": THRESHOLD_CAP, "max_casts": MAX_CASTS, "scenes": tol}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(tol, indent=1))
    if have == list(SCENES):
        check_coverage(allb)
    print("generated in %.0f s with %d workers" % (time.time() - t0, a.workers))


if __name__ == "__main__":
    main()
