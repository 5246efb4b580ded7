"""KDMesh and the k-d tree's build against an independent reading of the reference (tests/exact_kd.py, tests/exact_ref.py), on tests/golden/exact_kdmesh/.

The build (kdtree/leaf.rs:89-231) is restated twice from one reading: po_kd_partition_boxes in oracle/ and kd_partition in the host layer. tests/exact_kd.py
is a second reading. For triangle trees (KDMesh) it runs in plain f64 and must equal both in every array and every plane bit (why that is possible is
argued in its header); for scene trees, whose boxes come out of a matrix product, it decides at 256 bits and records the margin of every which_side
decision, and a build whose smallest margin is at least 2^-30 must have the same topology, axes and leaf lists, with planes and root bounds within the
measured threshold (tolerances.json: 64 x the 53-bit evaluation's deviation, below 2^-32).

The walk (kdtree/kdmesh.rs:62-74 over node.rs:66-203) is restated in tests/exact_ref.py over the independently built tree; tools/gen_exact_kdmesh.py
committed its answers for four scenes. The oracle is held to them here and the kernels in tests/test_gpu_exact_kdmesh.py. The oracle's po_cast_rays
reports no triangle index: on the CPU a triangle is pinned by t, point and normal within the thresholds, on the device by `sub` exactly.

What the fixtures found: nothing disagreed. mutants.json records, for twelve deliberate misreadings of the restatement, how many
fixtures each changes; eleven change at least one, and the twelfth (the root box test skipped) cannot change an answer at all."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import exact_kd  # noqa: E402
import gen_exact_kdmesh as K  # noqa: E402
import gen_exact_rays as G  # noqa: E402
import host_glue  # noqa: E402
from scene_dsl import KDMESH, KDMesh, Material, MeshData, Node, Scene  # noqa: E402
from test_exact_reference import check_against_exact, oracle_answer  # noqa: E402

TOL = K.load_tolerances()
SUMMARY = K.load_summary()
BUILD_SCENES = K.BUILD_ONLY + G.SCENES + K.SCENES
_cache = {}


def batch(scene, name):
    if (scene, name) not in _cache:
        _cache[scene, name] = K.load(scene, name)
    return _cache[scene, name]


def host_tree(t):
    return dict(t, depth=t["max_depth"])


# ---- the build: triangle trees
@pytest.mark.parametrize("scene", K.SCENES)
def test_triangle_trees_equal_the_oracle_and_the_host_in_every_bit(oracle, scene):
    sc = K.build_scene(scene)
    prims = G.flat_prims(sc)
    ids, meshes = K.meshes_by_first_use(prims)
    hs = host_glue.host_scene(sc)
    used = sorted({ids[i] for i, p in enumerate(prims) if p.kind == KDMESH})
    assert used, "the scene has no KDMesh"
    for mi in used:
        boxes = exact_kd.triangle_boxes(meshes[mi].positions, meshes[mi].triangles)
        mine = exact_kd.partition(boxes, exact_kd.MESH_DEPTH)
        ref = oracle.kd_partition_boxes([b[0] for b in boxes], [b[1] for b in boxes], exact_kd.MESH_DEPTH)
        got = host_tree(hs.kdmesh_tree(mi))
        print("%s mesh %d (%s): %d triangles, %d nodes, %d leaf items, depth %d" % (scene, mi, meshes[mi].name, len(boxes), len(mine["kind"]), len(mine["items"]), mine["depth"]))
        assert exact_kd.difference(mine, ref) is None, (scene, mi, "the oracle's tree differs in", exact_kd.difference(mine, ref))
        assert exact_kd.difference(mine, got) is None, (scene, mi, "the host's tree differs in", exact_kd.difference(mine, got))
        assert got["depth"] == mine["depth"] <= exact_kd.MESH_DEPTH


def test_kdmesh_tree_entry_numbers_meshes_by_first_use_and_refuses_others():
    from portrayer_amd import host
    sc = K.build_scene("kdm_nested")
    hs = host_glue.host_scene(sc)
    assert K.meshes_by_first_use(G.flat_prims(sc))[0].count(0) == 3, "three nodes share the one mesh"
    assert len(hs.kdmesh_tree(0)["axis"]) > 1 and hs.kdmesh_tree(0, kd_mesh_depth=0)["axis"].tolist() == [-1]
    with pytest.raises(host.PortrayerHostError):
        hs.kdmesh_tree(1)


# ---- the build: scene trees
@pytest.mark.parametrize("scene", BUILD_SCENES)
def test_scene_tree_is_the_independent_builds(oracle, scene):
    pytest.importorskip("mpmath", reason="mpmath is needed to decide a scene tree's build at 256 bits")
    sc = K.build_scene(scene)
    depth = K.SCATTER_DEPTH if scene in K.BUILD_ONLY else K.KD_DEPTH
    ps = oracle.pack(sc)
    flat = oracle.flatten(ps)
    dump = oracle.kd_scene_dump(ps, kd_depth=depth)
    fixture, trans, _ = K.fixture_tree(scene)
    assert flat["trans"].tobytes() == trans.tobytes() and all(np.array_equal(dump[k], fixture[k]) for k in dump), "%s is not the scene of the fixture" % scene
    got = host_tree(host_glue.host_scene(sc).kdtree(depth))
    mine, trace = exact_kd.scene_tree(flat["trans"], G.flat_prims(sc), depth)
    rec = SUMMARY["builds"][scene]
    print("%s: %d nodes, %d which_side decisions, smallest margin %.3g" % (scene, len(mine["kind"]), trace.decisions, trace.margin))
    assert (trace.margin, trace.decisions, trace.margin >= G.FRAGILE) == (rec["margin"], rec["decisions"], rec["decidable"])
    if not rec["decidable"]:
        assert scene in SUMMARY["undecidable_builds"] and scene != "scatter40"
        return
    thr = TOL["build"]["threshold"]
    for who, t in (("the oracle", dump), ("the host", got)):
        assert exact_kd.same_structure(mine, t) is None, (scene, who, "differs in", exact_kd.same_structure(mine, t))
        assert exact_kd.plane_deviation(mine, t) <= thr, (scene, who, exact_kd.plane_deviation(mine, t), thr)
    assert got["depth"] == mine["depth"]


def test_build_threshold_is_the_measured_deviation():
    dev = max(r["plane_deviation53"] for r in SUMMARY["builds"].values() if r["decidable"])
    assert TOL["build"] == {"deviation": dev, "threshold": G.SLACK * dev} and 0.0 < TOL["build"]["threshold"] < G.THRESHOLD_CAP
    assert SUMMARY["builds"]["scatter40"]["decidable"] and SUMMARY["builds"]["scatter40"]["depth"] >= 4


# ---- the build: edges, on hand-made lists of boxes
def slabs(xs):
    """Boxes [lo, hi] x [-0.5, 0.5]^2 along x."""
    return [((float(lo), -0.5, -0.5), (float(hi), 0.5, 0.5)) for lo, hi in xs]


def points(xs):
    return slabs([(x, x) for x in xs])


EDGES = {
    # leaf.rs:248-300 and :302-360, the reference's own two tests
    "reference_centre": (points([-8, -5, 3, 5, 8]), 5, (3, 3, 10)),
    "reference_uneven": (points([-8, 0, 3, 5, 8]), 5, (3, 2, 10)),
    "depth_zero": (points(range(9)), 0, (3, 3, 10)),
    "three_items": (points([1, 2, 3]), 5, (3, 3, 10)),
    "one_item": (points([7]), 5, (3, 3, 10)),
    "no_items": ([], 5, (3, 3, 10)),
    "eight_identical": ([((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))] * 8, 3, (3, 3, 10)),
    "one_side_empty_after_ten_tries": (points([1, 1, 1, 1, 1]), 2, (3, 3, 10)),
    "touching_the_plane": (slabs([(-4, 0), (0, 4), (-4, -2), (2, 4), (-3, -1)]), 1, (3, 3, 10)),
    "merit_on_the_last_try": (slabs([(0, 0.5)] * 3 + [(1.5, 1.75)] * 3 + [(1024, 1024)]), 1, (3, 3, 10)),
    "merit_never": (slabs([(0, 0.25)] * 3 + [(0.75, 0.875)] * 3 + [(1024, 1024)]), 1, (3, 3, 10)),
    "shared_at_every_level": ([((0.0, 0.0, 0.0), (8.0, 8.0, 8.0))] * 2 + [((float(x), float(x), float(x)), (x + 1.0, x + 1.0, x + 1.0)) for x in range(8)], 6, (3, 3, 10)),
}


def leaves(t):
    return [list(t["items"][f:f + n]) for k, f, n in zip(t["kind"], t["first"], t["count"]) if k == 1]


@pytest.mark.parametrize("case", sorted(EDGES))
def test_build_edges_against_the_oracle_and_the_host(oracle, case):
    boxes, depth, conf = EDGES[case]
    mine = exact_kd.partition(boxes, depth, conf=conf)
    if boxes:
        ref = oracle.kd_partition_boxes([b[0] for b in boxes], [b[1] for b in boxes], depth, *conf)
        assert exact_kd.difference(mine, ref) is None, (case, "the oracle differs in", exact_kd.difference(mine, ref))
    if boxes and conf == exact_kd.CONF:   # the host builds with KDMesh's settings only: a mesh of one thin triangle per box, (min, max, min)
        pos = np.array([p for b in boxes for p in b], dtype=np.float64)
        mesh = MeshData(pos, np.array([(2 * i, 2 * i + 1, 2 * i) for i in range(len(boxes))], dtype=np.uint32), None, case)
        hs = host_glue.host_scene(Scene(Node.group([Node.geo(KDMesh(mesh), Material())]), [], (0.0, 0.0, 0.0)))
        got = host_tree(hs.kdmesh_tree(0, kd_mesh_depth=depth))
        assert exact_kd.difference(mine, got) is None, (case, "the host differs in", exact_kd.difference(mine, got))
    split = [(a, p) for k, a, p in zip(mine["kind"], mine["axis"], mine["plane"]) if k == 0]
    if case == "reference_centre":
        assert split == [(0, 0.0)] and leaves(mine) == [[2, 3, 4], [0, 1]]
    elif case == "reference_uneven":
        assert split == [(0, 4.0)] and leaves(mine) == [[3, 4], [0, 1, 2]]
    elif case in ("depth_zero", "three_items", "one_item", "no_items"):
        assert mine["kind"] == [1] and leaves(mine) == [list(range(len(boxes)))] and mine["depth"] == 0
        assert case != "no_items" or mine["root_bounds"] == [0.0] * 6
    elif case == "eight_identical":   # never separable: every try shares all eight, the plane halves towards the minimum, the full depth is reached
        assert mine["depth"] == 3 and leaves(mine) == [list(range(8))] * 8 and split[0] == (0, 2.0 ** -11)
    elif case == "one_side_empty_after_ten_tries":   # a list of zero thickness is split at its own coordinate: all in front (>= 0), nothing behind
        # (the empty side is a leaf of no items; the full side, identical in y, is shared ten times over and split 2^-11 above its minimum)
        assert split == [(0, 1.0), (1, -0.5 + 2.0 ** -11)] and leaves(mine) == [[0, 1, 2, 3, 4], [0, 1, 2, 3, 4], []]
    elif case == "touching_the_plane":   # max == plane is in front at that corner, so shared; min == plane is in front
        assert split == [(0, 0.0)] and leaves(mine) == [[0, 1, 3], [0, 2, 4]]
    elif case == "merit_on_the_last_try":   # 512, 256, .., 2 are too far forward; the tenth try, at 1, is good and is kept
        assert split == [(0, 1.0)] and leaves(mine) == [[3, 4, 5, 6], [0, 1, 2]]
    elif case == "merit_never":   # the tenth try, at 1, fails too: the plane moves once more and is taken unseen
        assert split == [(0, 0.5)] and leaves(mine) == [[3, 4, 5, 6], [0, 1, 2]]
    elif case == "shared_at_every_level":
        assert mine["depth"] == 6 and all(l[:2] == [0, 1] for l in leaves(mine) if l)


# ---- the walk: the oracle against the exact answers
@pytest.fixture(scope="module")
def packed(oracle):
    out = {}
    for s in K.SCENES:
        scene = K.build_scene(s)
        ps = oracle.pack(scene)
        flat = oracle.flatten(ps)
        c = batch(s, "random")
        assert flat["trans"].tobytes() == c["trans"].tobytes() and np.array_equal(flat["prim_type"], c["prim_type"]), "%s is not the scene of the fixture" % s
        out[s] = (scene, ps, flat)
    return out


@pytest.mark.parametrize("mode", ["flat", "kd", "hier"])
@pytest.mark.parametrize("name", K.BATCH_NAMES)
@pytest.mark.parametrize("scene", K.SCENES)
def test_oracle_walks_kdmesh_as_the_exact_reference(oracle, packed, scene, name, mode):
    c = batch(scene, name)
    om = {"flat": oracle.MODE_FLAT, "kd": oracle.MODE_KD, "hier": oracle.MODE_HIER}[mode]
    o, d = c["o"], c["d"]
    if name == "camera":
        o, d = oracle.camera_rays(list(c["cam"]), G.CAM_W, G.CAM_H, c["xy"])
        # (kdm_grid's threshold for the normal is 0, its normals being exact: the directions are held to 2^-48 there)
        assert np.array_equal(o, c["o"]) and np.all(np.linalg.norm(d - c["d"], axis=1) <= max(TOL["scenes"][scene]["normal"]["threshold"], 2.0 ** -48)), "eye rays"
    got = oracle_answer(oracle, packed[scene][1], o, d, om, with_id=mode != "hier")
    compared, left_out, _ = check_against_exact("%s %s %s" % (scene, name, mode), c, got, TOL["scenes"][scene], mode)
    assert left_out <= G.FRAGILE_CAP[name] * len(c["hit"]) and compared + left_out == len(c["hit"])


# ---- the fixture itself
@pytest.mark.parametrize("scene", K.SCENES)
def test_fixture_meets_its_conditions(scene):
    bs = {b: batch(scene, b) for b in K.BATCH_NAMES}
    for b, n in K.BATCHES:
        assert len(bs[b]["hit"]) == n
    assert len(bs["camera"]["hit"]) == G.CAM_W * G.CAM_H
    assert K.check_conditions(scene, bs) == SUMMARY["scenes"][scene]
    tot = SUMMARY["scenes"][scene]["totals"]
    assert tot["distinct_triangles_hit"] >= 20 and tot["hits_found_on_a_pending_far_side"] >= 20
    if scene == "kdm_far":
        assert tot["kdmesh_differs_from_mesh"] >= 100 and tot["kdmesh_and_mesh_hit_alike"] >= 100
    if scene == "kdm_near":
        assert tot["kdmesh_differs_from_mesh"] == 0


def test_special_batches_hold_what_they_must():
    """Origins inside the root box and on split planes, zero components, lengths 2^-6 to 2^6, rays that graze the root box (counted in model space)."""
    for scene in K.SCENES:
        c = batch(scene, "special")
        prims = G.flat_prims(K.build_scene(scene))
        i = [k for k, p in enumerate(prims) if p.kind == KDMESH][0]
        tree = exact_kd.mesh_tree(prims[i].mesh)
        inv = np.linalg.inv(c["trans"][i])
        om = c["o"] @ inv[:3, :3].T + inv[:3, 3]
        rb = np.array(tree["root_bounds"])
        inside = np.all((om >= rb[:3] - 1e-9) & (om <= rb[3:] + 1e-9), axis=1)
        planes = {(a, p) for k, a, p in zip(tree["kind"], tree["axis"], tree["plane"]) if k == 0}
        on_plane = np.array([any(abs(om[k][a] - p) <= 1e-12 * max(1.0, abs(p)) for a, p in planes) for k in range(len(om))])
        length = np.linalg.norm(c["d"] @ inv[:3, :3].T if scene == "kdm_grid" else c["d"], axis=1)   # the grid's rays are made in model space
        zero = (c["d"] == 0.0).any(axis=1)
        print("%s special: %d inside the root box, %d on a split plane, %d with a zero component, lengths %.3g to %.3g" %
              (scene, inside.sum(), on_plane.sum(), zero.sum(), length.min(), length.max()))
        assert inside.sum() >= 32 and on_plane.sum() >= 32 and zero.sum() >= 16
        assert 2.0 ** -6.01 <= length.min() <= 2.0 ** -4 and 2.0 ** 4 <= length.max() <= 2.0 ** 6.01
        if scene == "kdm_grid":   # the node's matrix is exact there: on the plane means on it
            assert np.array([any(om[k][a] == p for a, p in planes) for k in range(len(om))]).sum() >= 32


def test_tolerances_and_sizes():
    assert (TOL["fragile_margin"], TOL["slack"], TOL["threshold_cap"]) == (G.FRAGILE, G.SLACK, G.THRESHOLD_CAP) == (2.0 ** -30, 64.0, 2.0 ** -32)
    assert TOL["scenes"] == K.tolerances({s: {b: batch(s, b) for b in K.BATCH_NAMES} for s in K.SCENES})
    for s in K.SCENES:
        for q, v in TOL["scenes"][s].items():
            print("%s %s: deviation %.3g, threshold %.3g" % (s, q, v["deviation"], v["threshold"]))
            assert 0.0 <= v["threshold"] == G.SLACK * v["deviation"] < G.THRESHOLD_CAP
            assert v["threshold"] > 0.0 or (s, q) == ("kdm_grid", "normal")   # (0, 1, 0) or its opposite in every evaluation: exact
    earlier = max(os.path.getsize(os.path.join(G.OUT, f)) for f in os.listdir(G.OUT))
    sizes = {f: os.path.getsize(os.path.join(K.OUT, f)) for f in os.listdir(K.OUT)}
    assert max(sizes.values()) <= earlier and sum(sizes.values()) < 1 << 20, (max(sizes.values()), earlier, sum(sizes.values()))


def test_generator_reproduces_a_batch_byte_for_byte():
    pytest.importorskip("mpmath", reason="mpmath is needed to re-evaluate the exact reference")
    scene, name = K.CHECK_BATCH
    with open(K.path(scene, name), "rb") as fh:
        assert K.npz_bytes(K.make_batch(scene, name, workers=4)) == fh.read()


# ---- the tests can fail
def test_every_mutant_of_the_restatement_changes_a_fixture():
    """mutants.json (tools/gen_exact_kdmesh.py --mutants) lists all twelve, eleven with at least one fixture changed; the build mutants are recomputed here on the
    triangle trees, and a recorded witness ray of every walk mutant is evaluated again: the mutant answers it differently from the fixture, the
    restatement as it stands answers it as the fixture does."""
    exact_ref = pytest.importorskip("exact_ref", reason="mpmath is needed to evaluate the exact reference")
    table = K.load_mutants()
    assert sorted(table) == sorted(exact_kd.MUTANTS + exact_ref.WALK_MUTANTS) and len(table) == 12
    meshes = {}
    for s in K.SCENES:
        for m in K.meshes_by_first_use([p for p in G.flat_prims(K.build_scene(s)) if p.kind == KDMESH])[1]:
            meshes[m.name] = m
    exs = {}
    for mutant, rec in sorted(table.items()):
        print("%-26s %-5s changes %d fixtures" % (mutant, rec["kind"], rec["fixtures_changed"]))
        if mutant in K.EQUIVALENT_MUTANTS:   # no triangle lies outside its root box: the box test cannot change an answer (see gen_exact_kdmesh.py)
            assert rec["fixtures_changed"] == 0
            continue
        assert rec["fixtures_changed"] >= 1
        if rec["kind"] == "build":
            changed = sorted(n for n, m in meshes.items() if exact_kd.difference(exact_kd.mesh_tree(m, mutant=mutant), exact_kd.mesh_tree(m)) is not None)
            assert changed == rec["triangle_trees_changed"]
            continue
        fixture, k = rec["witnesses"][0]
        scene, name = fixture.rsplit("_", 1)
        if scene not in exs:
            exs[scene] = K.exact_scenes(scene, K.scene_inputs(scene))[0]
        ex, c = exs[scene], batch(scene, name)
        assert not c["fragile"][k]
        ex.mutant = None
        assert not K._changed(ex, c, k), (mutant, fixture, k, "the restatement does not reproduce the fixture")
        ex.mutant = mutant
        try:
            assert K._changed(ex, c, k), (mutant, fixture, k, "the witness is not changed")
        finally:
            ex.mutant = None
