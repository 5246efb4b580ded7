"""KDMesh on the device (pt_kdmesh_hit, pt_kdmesh_hit_filtered) against the exact-arithmetic reference's answers in tests/golden/exact_kdmesh/.

Reads the fixtures and tolerances.json only (tools/gen_exact_kdmesh.py wrote them from tests/exact_ref.py over the independently built trees of
tests/exact_kd.py; tests/test_exact_kdtree.py says what they hold). On every ray the exact reference can decide, in all three traversals, nearest hit
and any_hit, whole rays and bounded segments: the exact hit, flattened node, triangle (`sub`) and material, and t, position and normal within the scene's
thresholds. A KDMesh does not answer as a Mesh (the squared extent, quirk Q3; the last EPSILON of a clipped range), and under a bound just above the hit it
may not answer as without one: the exact answers for both bounds are in the fixture. The device still equals the oracle bit for bit on these batches."""
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
from scene_dsl import KDMESH  # noqa: E402
from test_gpu_aov import compare, first_use_order, packed_tri_off  # noqa: E402
from test_gpu_exact_rays import as_exact, decidable, joined, traversal  # noqa: E402
from test_gpu_rays import as_aov, oracle_rays, same  # noqa: E402

pytestmark = pytest.mark.gpu

RAY_BATCHES = tuple(b for b, _ in K.BATCHES)
TOL = K.load_tolerances()["scenes"]
MODES = ("flat", "kd", "hier")


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


@pytest.fixture(scope="module")
def scenes(oracle):
    out = {}
    for s in K.SCENES:
        scene = K.build_scene(s)
        ps = oracle.pack(scene)
        flat = oracle.flatten(ps)
        flat["_mesh_tri_off"] = packed_tri_off(ps.arrays)
        flat["material_expected"] = first_use_order(flat["material"])
        bs = [K.load(s, b) for b in RAY_BATCHES]
        assert flat["trans"].tobytes() == bs[0]["trans"].tobytes(), "%s is not the scene of the fixture" % s
        assert len(set(flat["material_expected"].tolist())) == len(flat["material_expected"]), "a material per node"
        out[s] = dict(scene=scene, host=host_glue.host_scene(scene), ps=ps, flat=flat, rays=joined(bs), camera=K.load(s, "camera"),
                      caps=sum(G.FRAGILE_CAP[b] * n for b, n in K.BATCHES))
    return out


def check(tag, c, which, got, flat, tol, ok, exp=None):
    """got (a device record) against the exact answer `which` of the fixture (or `exp`) on the rays `ok`; prints what was compared."""
    exp = K.expected(c, which) if exp is None else exp
    rec = as_exact(got)
    bad = ok & ~G.agreement(exp, rec, tol)
    h = ok & exp["hit"]
    on_kdm = h & (flat["prim_type"][np.maximum(exp["node"], 0)] == KDMESH)
    print("%s: %d rays compared, %d hits, %d of them on a KDMesh (%d triangles), %d left out as fragile"
          % (tag, int(ok.sum()), int(h.sum()), int(on_kdm.sum()), len(set(zip(exp["node"][on_kdm].tolist(), exp["sub"][on_kdm].tolist()))), int((~ok).sum())))
    assert not bad.any(), "%s: %d rays disagree with the exact reference; %s" % (tag, int(bad.sum()), G.first_disagreement(exp, rec, bad))
    assert np.array_equal(got["material"][h], flat["material_expected"][exp["node"][h]]), "%s: material is not the exact node's" % tag
    meshy = np.isin(flat["prim_type"][exp["node"][h]], (2, 3))
    assert np.all(got["sub"][h][~meshy] == 0), "%s: sub must be 0 on anything but a mesh" % tag


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene", K.SCENES)
def test_nearest_hits_on_kdmesh_are_the_exact_ones(oracle, host, H, scenes, scene, mode):
    s, tol = scenes[scene], TOL[scene]
    c = s["rays"]
    tr, om = traversal(H, oracle, mode)
    r = host.Renderer(s["host"], tr, kd_depth=K.KD_DEPTH)
    got = r.rays(c["o"], c["d"])
    again = r.rays(c["o"], c["d"], reorder=True)
    occ = [r.rays(c["o"], c["d"], any_hit=True, reorder=ro)["occluded"] for ro in (False, True)]
    r.close()
    ok = decidable(c, mode)
    assert int((~ok).sum()) <= s["caps"], "too many rays left out as fragile"
    which = "kd" if mode == "kd" else "nearest"
    check("%s %s" % (scene, mode), c, which, got, s["flat"], tol, ok)
    same(got, again)
    exp = K.expected(c, which)
    for ro, x in zip((False, True), occ):
        assert np.array_equal(x[ok], exp["hit"][ok].astype(np.uint8)), "%s %s: any_hit (reorder=%s) is not the exact 'anything in range'" % (scene, mode, ro)
    # the device's arrays still equal the oracle's bit for bit on these batches
    ref = oracle_rays(oracle, s["ps"], c["o"], c["d"], om, K.KD_DEPTH, workers=4)
    compare("%s %s vs the oracle" % (scene, mode), as_aov(got), ref, s["flat"], hier=mode == "hier")
    if mode != "hier":
        assert np.array_equal(got["node"], ref["id"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene", K.SCENES)
def test_segments_on_kdmesh_end_a_millionth_before_and_after_the_hit(oracle, host, H, scenes, scene, mode):
    """t_max = t (1 + 2^-20) and t (1 - 2^-20), 1000 on a miss; nearest hit and any_hit: the filtered walk (pt_kdmesh_hit_filtered).
    The device's contract for a segment is `the ray's answer restricted to t < t_max`: a KDMesh is walked without the bound and its hit
    counts iff t < t_max, where the reference's own bounded cast ends the walk's segment EPSILON before the bound and loses hits behind planes in that
    last sliver. The fixture holds the exact BOUNDED answers; they are the contract's wherever no KDMesh answers differently under the bound:
      above the hit  the contract's answer is the exact nearest hit itself; how often the exact bounded cast loses it is printed;
      below the hit  the exact bounded answer, except on the rays where that is a hit on a KDMesh (another triangle of a mesh whose unbounded walk stops
                     at the nearest hit: the filter reports none); they are counted, printed and left out."""
    s, tol = scenes[scene], TOL[scene]
    c = s["rays"]
    r = host.Renderer(s["host"], traversal(H, oracle, mode)[0], kd_depth=K.KD_DEPTH)
    ok = decidable(c, mode, segment=True)
    assert int((~ok).sum()) <= s["caps"], "too many rays left out as fragile"
    kd = "kd" if mode == "kd" else "nearest"
    for side, which in ((1, kd), (0, "kd_below" if mode == "kd" else "below")):
        t_max = np.ascontiguousarray(c["t_max"][:, side])
        exp = K.expected(c, which)
        use = ok.copy()
        if side == 1:
            beyond = exp["hit"] & ~(exp["t"] < t_max)   # the bounds are the flat walk's hit's: the k-d walk's own hit may lie beyond them (Q1, Q3)
            exp["hit"][beyond], exp["t"][beyond], exp["node"][beyond], exp["sub"][beyond] = False, np.inf, -1, -1
            exp["point"][beyond], exp["normal"][beyond] = 0.0, 0.0
            assert mode == "kd" or not beyond.any()
            bounded = K.expected(c, "kd_above" if mode == "kd" else "above")
            print("%s %s: the reference's bounded cast loses or changes %d of %d hits under the upper bound" %
                  (scene, mode, int((ok & ((bounded["hit"] != exp["hit"]) | (bounded["sub"] != exp["sub"]))).sum()), int((ok & exp["hit"]).sum())))
        else:
            on_kdm = exp["hit"] & (s["flat"]["prim_type"][np.maximum(exp["node"], 0)] == KDMESH)
            print("%s %s: %d rays whose exact bounded answer below the hit is on a KDMesh are left out" % (scene, mode, int((ok & on_kdm).sum())))
            use &= ~on_kdm
        for ro in (False, True):
            got = r.rays(c["o"], c["d"], t_max=t_max, reorder=ro)
            check("%s %s t_max %s reorder=%d" % (scene, mode, ("below", "above")[side], ro), c, which, got, s["flat"], tol, use, exp)
            occ = r.rays(c["o"], c["d"], any_hit=True, t_max=t_max, reorder=ro)["occluded"]
            assert np.array_equal(occ[use], exp["hit"][use].astype(np.uint8)), "%s %s: any_hit with t_max %s the hit" % (scene, mode, ("below", "above")[side])
    r.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene", K.SCENES)
def test_primary_visibility_of_kdmesh_is_the_exact_eye_rays_hit(oracle, host, H, scenes, scene, mode):
    s, tol = scenes[scene], TOL[scene]
    c = s["camera"]
    r = host.Renderer(s["host"], traversal(H, oracle, mode)[0], kd_depth=K.KD_DEPTH)
    aov = r.aov(c["cam"], G.CAM_W, G.CAM_H)
    r.close()
    got = {k: np.ascontiguousarray(aov[ka].reshape((G.CAM_W * G.CAM_H,) + aov[ka].shape[2:]))
           for k, ka in (("t", "depth"), ("position", "position"), ("normal", "normal"), ("node", "node"), ("sub", "sub"), ("material", "material"))}
    ok = decidable(c, mode)
    assert int((~ok).sum()) <= G.FRAGILE_CAP["camera"] * len(ok)
    check("%s %s camera" % (scene, mode), c, "kd" if mode == "kd" else "nearest", got, s["flat"], tol, ok)


@pytest.mark.parametrize("cull", ["0", "1", "2", "3"])
def test_f32_culls_never_change_an_answer(oracle, host, H, scenes, monkeypatch, cull):
    """kdm_far in the k-d traversal with the f32 cull boxes of tree nodes (bit 0) and leaf references (bit 1) off and on."""
    s, c = scenes["kdm_far"], scenes["kdm_far"]["rays"]
    monkeypatch.setenv("PORTRAYER_KD_CULL", cull)
    r = host.Renderer(s["host"], H.TRAVERSE_KD, kd_depth=K.KD_DEPTH)   # (a new renderer: the switch acts at upload)
    got = r.rays(c["o"], c["d"])
    r.close()
    check("kdm_far kd PORTRAYER_KD_CULL=%s" % cull, c, "kd", got, s["flat"], TOL["kdm_far"], decidable(c, "kd"))


@pytest.mark.parametrize("scene", K.SCENES)
def test_the_uploaded_tree_is_the_independent_builds(host, scenes, scene):
    """Through ph_scene_kdmesh_tree, which calls what the upload calls; needs no kernel."""
    prims = G.flat_prims(scenes[scene]["scene"])
    ids, meshes = K.meshes_by_first_use(prims)
    for mi in sorted({ids[i] for i, p in enumerate(prims) if p.kind == KDMESH}):
        got = scenes[scene]["host"].kdmesh_tree(mi)
        diff = exact_kd.difference(exact_kd.mesh_tree(meshes[mi]), dict(got, depth=got["max_depth"]))
        assert diff is None, (scene, mi, "the host's tree differs in", diff)
