"""The reference's k-d tree BUILD restated (test infrastructure): KDLeaf::partitioned and what it stands on.

Written from the Rust sources - kdtree/leaf.rs:89-231, kdtree/kdmesh.rs:37-58, kdtree/kdscene.rs:19-43, bounding_box.rs:23-37 and :57-99 and
:123-148, primitive/infinite_plane.rs:27-35, the `bounds()` of primitive/*.rs and flat_scene.rs:63-69 - not from oracle/ or the host layer: this is
the independent reading that those two (po_kd_partition_boxes and kd_partition, which come from one reading) are compared with.

Triangle trees (KDMesh) are built in plain Python floats and must equal the reference's in every bit. Why that holds without knowing how the `vek`
crate orders its operations: a triangle's box is the minimum and maximum of its vertices' coordinates, and a list's box the minimum and maximum of its
members' (bounding_box.rs:23-37), so every box coordinate is a vertex coordinate, selected, never computed. Every later operation is written out in
leaf.rs itself, in its order: `min + (max - min) / 2.0` for the first plane, `p + (hi - p) / 2.0` and `lo + (p - lo) / 2.0` for the retried ones, and
comparisons. They are applied to Vec3s of the form axis * v, whose two other components are zeros of either sign and stay zeros. which_side is
`(p - point).dot(normal) >= 0.0` with a unit axis as the normal: one term is (p_a - plane) * 1.0, the other two are a finite number times 0.0, so the
sum is p_a - plane, or a zero of either sign where that is zero, in whatever order the three terms are added - and `>= 0.0` takes both zeros. IEEE
subtraction gives a zero only for equal operands, so the decision is p_a >= plane exactly. Nothing depends on the crate's order of operations.

Scene trees are different: a node's box is `trans * prim.bounds()`, eight corners through a matrix, and its last bit is `vek`'s. There only the
DECISIONS are restated: the boxes are evaluated with mpmath at 256 bits from the flattened f64 matrices (taken as exact rationals, as tests/exact_ref.py
takes them), and every which_side decision of every try records its relative margin |coordinate - plane| / max(1, |coordinate|, |plane|). A build whose
smallest margin is at least 2^-30 (exact_ref.FRAGILE) is decidable: a correct f64 build must then have the same topology, axes and leaf lists; planes and
root bounds agree to rounding.

A tree is a dict in the layout of the oracle's dump and the host's ph_scene_kdtree: nodes in pre-order (a split, its front subtree, its back subtree),
kind (0 split, 1 leaf), axis (-1 on a leaf), plane, front, back (-1 on a leaf), first, count (0 on a split), items in leaf order, root_bounds (min then
max), depth (levels of splits on the longest path). MUTANTS names deliberate misreadings, for showing that the comparisons can fail."""
from __future__ import annotations

import math

from scene_dsl import CONE, CUBE, CYLINDER, KDMESH, MESH, PLANE, SPHERE, TRIANGLE

MUTANTS = ("side_gt", "front_ge_back", "range_not_narrowed", "shared_to_front_only", "axis_rotated_back", "child_bounds_from_parent")
CONF = (3, 3, 10)   # target_max_nodes, target_max_merit, max_tries: kdmesh.rs:44-48 and kdscene.rs:29-33 alike
MESH_DEPTH = SCENE_DEPTH = 10


class BuildTrace:
    """Smallest relative margin of the which_side decisions of a build (every try of every split, and the final partition)."""

    def __init__(self):
        self.margin = math.inf
        self.decisions = 0

    def side(self, coordinate, plane):
        fa, fb = float(coordinate), float(plane)
        m = abs(float(coordinate - plane)) / max(1.0, abs(fa), abs(fb))
        self.decisions += 1
        if m < self.margin:
            self.margin = m


def _list_bounds(boxes, ids, zero):
    """bounding_box.rs:23-37: an empty list's box is (0, 0); else a fold of minima and maxima from the first member's."""
    if not ids:
        return (zero, zero, zero), (zero, zero, zero)
    mn, mx = list(boxes[ids[0]][0]), list(boxes[ids[0]][1])
    for i in ids[1:]:
        for q in range(3):
            if boxes[i][0][q] < mn[q]:
                mn[q] = boxes[i][0][q]
            if boxes[i][1][q] > mx[q]:
                mx[q] = boxes[i][1][q]
    return tuple(mn), tuple(mx)


def partition(boxes, max_depth, conf=CONF, mutant=None, trace=None, zero=0.0):
    """KDLeaf::partitioned from unit_x over `boxes`, a list of (min, max) triples of numbers of one kind (floats, or mpf at the caller's precision)."""
    assert mutant is None or mutant in MUTANTS, mutant
    target_max_nodes, target_max_merit, max_tries = conf
    t = dict(kind=[], axis=[], plane=[], front=[], back=[], first=[], count=[], items=[])
    deepest = [0]

    def front_of(plane, x):   # infinite_plane.rs:27-35 with a positive unit axis as the normal
        if trace is not None:
            trace.side(x, plane)
        return x - plane > 0 if mutant == "side_gt" else x - plane >= 0

    def side(box, axis, plane):   # leaf.rs:114-131
        lo, hi = front_of(plane, box[0][axis]), front_of(plane, box[1][axis])
        return "front" if lo and hi else ("back" if not lo and not hi else "shared")

    def add(kind, axis, plane, first, count):
        for k, v in zip(("kind", "axis", "plane", "front", "back", "first", "count"), (kind, axis, plane, -1, -1, first, count)):
            t[k].append(v)
        return len(t["kind"]) - 1

    def build(ids, bounds, axis, depth_left, level):
        if depth_left == 0 or len(ids) <= target_max_nodes:   # leaf.rs:91-93
            me = add(1, -1, zero, len(t["items"]), len(ids))
            t["items"].extend(ids)
            return me
        deepest[0] = max(deepest[0], level + 1)
        lo, hi = bounds[0][axis], bounds[1][axis]
        plane = lo + (hi - lo) / 2                              # leaf.rs:140-143
        for _ in range(max_tries):                              # leaf.rs:156-201
            front = back = shared = 0
            for i in ids:
                s = side(boxes[i], axis, plane)
                front, back, shared = front + (s == "front"), back + (s == "back"), shared + (s == "shared")
            if abs(front - back) + shared <= target_max_merit:
                break
            forward = front >= back if mutant == "front_ge_back" else front > back
            if forward:
                if mutant != "range_not_narrowed":
                    lo = plane
                plane = plane + (hi - plane) / 2
            else:
                if mutant != "range_not_narrowed":
                    hi = plane
                plane = lo + (plane - lo) / 2
        fi, bi = [], []
        for i in ids:                                           # leaf.rs:204-215: a shared item goes to both sides, in the list's order
            s = side(boxes[i], axis, plane)
            if s != "back":
                fi.append(i)
            if s == "back" or (s == "shared" and mutant != "shared_to_front_only"):
                bi.append(i)
        nxt = (axis + 2) % 3 if mutant == "axis_rotated_back" else (axis + 1) % 3   # leaf.rs:97-103: x -> y -> z -> x
        me = add(0, axis, plane, 0, 0)
        fb, bb = (bounds, bounds) if mutant == "child_bounds_from_parent" else (_list_bounds(boxes, fi, zero), _list_bounds(boxes, bi, zero))
        t["front"][me] = build(fi, fb, nxt, depth_left - 1, level + 1)
        t["back"][me] = build(bi, bb, nxt, depth_left - 1, level + 1)
        return me

    root = _list_bounds(boxes, list(range(len(boxes))), zero)
    build(list(range(len(boxes))), root, 0, max_depth, 0)
    t["root_bounds"] = list(root[0]) + list(root[1])
    t["depth"] = deepest[0]
    return t


def triangle_boxes(positions, triangles):
    """triangle.rs:29-36 for every triangle of a mesh: the boxes KDMesh::new partitions (kdmesh.rs:39-43). Python floats."""
    out = []
    for ia, ib, ic in triangles:
        v = [[float(x) for x in positions[int(k)]] for k in (ia, ib, ic)]
        out.append((tuple(min(v[0][q], v[1][q], v[2][q]) for q in range(3)), tuple(max(v[0][q], v[1][q], v[2][q]) for q in range(3))))
    return out


def mesh_tree(mesh, max_depth=MESH_DEPTH, mutant=None):
    """KDMesh::new (kdmesh.rs:37-58) in plain f64: equal to the reference's tree in every bit (see the header)."""
    return partition(triangle_boxes(mesh.positions, mesh.triangles), max_depth, mutant=mutant)


# ---- scene trees: boxes at 256 bits, decisions with margins
def model_bounds(prim, mpf):
    """Bounds for a primitive (primitive/*.rs; mesh.rs:69-86; kdmesh.rs:26-30: the root node's bounds, the fold over the triangles' boxes)."""
    k = prim.kind
    if k == SPHERE:
        return (mpf(-1),) * 3, (mpf(1),) * 3
    if k == CUBE or k == CYLINDER or k == CONE:
        return (mpf(-0.5),) * 3, (mpf(0.5),) * 3
    if k == PLANE:
        return (mpf(-0.5), mpf(0), mpf(-0.5)), (mpf(0.5), mpf(0), mpf(0.5))
    if k == TRIANGLE:
        v = [[mpf(float(x)) for x in p] for p in prim.tri]
    elif k == MESH:
        v = [[mpf(float(x)) for x in p] for p in prim.mesh.positions]
    elif k == KDMESH:
        v = [[mpf(float(x)) for x in prim.mesh.positions[int(i)]] for t in prim.mesh.triangles for i in t]
    else:
        raise ValueError(k)
    return tuple(min(p[q] for p in v) for q in range(3)), tuple(max(p[q] for p in v) for q in range(3))


def world_bounds(trans, prim, mpf):
    """flat_scene.rs:63-69 over bounding_box.rs:123-148: the eight corners of the model box through the node's matrix, then minima and maxima."""
    lo, hi = model_bounds(prim, mpf)
    m = [[mpf(float(trans[r][c])) for c in range(4)] for r in range(3)]
    pts = [tuple(m[r][0] * x + m[r][1] * y + m[r][2] * z + m[r][3] for r in range(3)) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]
    return tuple(min(p[q] for p in pts) for q in range(3)), tuple(max(p[q] for p in pts) for q in range(3))


def scene_tree(flat_trans, prims, max_depth=SCENE_DEPTH, prec=256, mutant=None):
    """KDTreeScene::from (kdscene.rs:19-43) over the flattened nodes' f64 matrices: (tree with planes and root bounds rounded to f64, BuildTrace)."""
    from mpmath import mp, mpf
    old = mp.prec
    mp.prec = prec
    try:
        boxes = [world_bounds(t, p, mpf) for t, p in zip(flat_trans, prims)]
        trace = BuildTrace()
        t = partition(boxes, max_depth, mutant=mutant, trace=trace, zero=mpf(0))
        t["plane"] = [float(x) for x in t["plane"]]
        t["root_bounds"] = [float(x) for x in t["root_bounds"]]
        return t, trace
    finally:
        mp.prec = old


STRUCTURE = ("kind", "axis", "front", "back", "first", "count", "items")


def same_structure(a, b):
    """Topology, axes and every leaf's item list in order: the first differing array's name, or None."""
    a, b = _canonical(a), _canonical(b)
    for k in STRUCTURE:
        if a[k] != b[k]:
            return k
    return None


def _canonical(t):
    """The host's arrays name a leaf by axis -1 and have no `kind`; what a leaf's front / back and a split's first / count hold is not part of a tree."""
    axis = [int(x) for x in t["axis"]]
    leaf = [x < 0 for x in axis]
    if "kind" in t:
        assert [int(k) == 1 for k in t["kind"]] == leaf, "kind and axis disagree"
    out = dict(kind=[int(x) for x in leaf], axis=axis, items=[int(x) for x in t["items"]])
    for k in ("front", "back"):
        out[k] = [-1 if l else int(x) for l, x in zip(leaf, t[k])]
    for k in ("first", "count"):
        out[k] = [int(x) if l else 0 for l, x in zip(leaf, t[k])]
    return out


def difference(a, b):
    """Array for array, planes and root bounds bit for bit (signed zeros and all): the first differing array's name, or None."""
    import struct
    k = same_structure(a, b)
    if k is not None:
        return k
    bits = lambda v: [struct.pack("<d", float(x)) for x in v]
    split = [i for i, axis in enumerate(a["axis"]) if int(axis) >= 0]
    if bits([a["plane"][i] for i in split]) != bits([b["plane"][i] for i in split]):
        return "plane"
    if "root_bounds" in a and "root_bounds" in b and bits(a["root_bounds"]) != bits(b["root_bounds"]):   # (po_kd_partition_boxes reports none)
        return "root_bounds"
    if "depth" in a and "depth" in b and int(a["depth"]) != int(b["depth"]):
        return "depth"
    return None


def plane_deviation(a, b):
    """Largest |a - b| / max(1, |a|) over the split planes and the root bounds of two trees of one structure."""
    dev = 0.0
    for k, idx in (("plane", [i for i, axis in enumerate(a["axis"]) if int(axis) >= 0]), ("root_bounds", range(6))):
        for i in idx:
            dev = max(dev, abs(float(a[k][i]) - float(b[k][i])) / max(1.0, abs(float(a[k][i]))))
    return dev
