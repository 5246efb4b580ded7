"""Ray queries on the device (Renderer.rays, Renderer.aov) against the exact-arithmetic reference's answers in tests/golden/exact/.

Reads the fixtures and tolerances.json only (tools/gen_exact_rays.py wrote them from tests/exact_ref.py; see tests/test_exact_reference.py for what they
hold and how the thresholds were measured). On every ray the exact reference can decide, in all three traversals: occluded and node >= 0 are the exact hit,
`node` is the exact flattened index - in the hierarchical traversal too - `sub` the exact triangle, `material` that node's (every node of these scenes
has a material of its own), and t, position and normal lie within the scene's thresholds. Fragile rays are left out and counted against the caps. In the k-d
traversal the exact answer is the exact walk of the scene's k-d tree, which on a few rays is not the flat walk's (quirks Q1 and Q3 of SURVEY App. D)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import gen_exact_rays as G  # noqa: E402
import host_glue  # noqa: E402
from test_gpu_aov import compare, first_use_order, packed_tri_off  # noqa: E402
from test_gpu_rays import as_aov, oracle_rays, same  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH_NAMES = tuple(b for b, _ in G.BATCHES)
TOL = G.load_tolerances()
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
    """Per scene: the host scene, the oracle's packed scene and flattened arrays, the three batches as one of 2,560 rays, and the camera batch."""
    out = {}
    for s in G.SCENES:
        scene = G.build_scene(s)
        ps = oracle.pack(scene)
        flat = oracle.flatten(ps)
        flat["_mesh_tri_off"] = packed_tri_off(ps.arrays)
        flat["material_expected"] = first_use_order(flat["material"])
        bs = [G.load(s, b) for b in BATCH_NAMES]
        assert flat["trans"].tobytes() == bs[0]["trans"].tobytes(), "%s is not the scene of the fixture" % s
        assert len(set(flat["material_expected"].tolist())) == len(flat["material_expected"]) <= 17, "a material per node, at most 17 nodes"
        out[s] = dict(host=host_glue.host_scene(scene), ps=ps, flat=flat, rays=joined(bs), camera=G.load(s, "camera"), caps=sum(
            G.FRAGILE_CAP[b] * n for b, n in G.BATCHES))
    return out


def joined(bs):
    """The batches of a scene as one: per-ray arrays concatenated, the indices of the sparse k-d answers shifted."""
    c, off = {}, np.cumsum([0] + [len(b["hit"]) for b in bs])
    for k in bs[0]:
        if k.endswith("_idx"):
            c[k] = np.concatenate([b[k] + o for b, o in zip(bs, off)])
        elif k.startswith(("trans", "prim_type", "tree_", "dev53", "replaced")):
            c[k] = bs[0][k]
        else:
            c[k] = np.concatenate([b[k] for b in bs])
    assert len(c["hit"]) == 2560
    return c


def traversal(H, oracle, mode):
    return {"flat": (H.TRAVERSE_FLAT, oracle.MODE_FLAT), "kd": (H.TRAVERSE_KD, oracle.MODE_KD), "hier": (H.TRAVERSE_HIER, oracle.MODE_HIER)}[mode]


def decidable(c, mode, segment=False):
    if mode == "kd":
        return ~c["kd_fragile"] & (~c["kd_segment_fragile"] if segment else True)
    ok = ~c["fragile"] & (~c["segment_fragile"] if segment else True)
    return ok & ~c["hier_fragile"] if mode == "hier" else ok


def as_exact(got):
    """A device record in the terms of the exact answer; the miss values are checked on the way: +inf, -1, +0."""
    hit = got["node"] >= 0
    assert np.array_equal(hit, np.isfinite(got["t"])) and np.all(np.isposinf(got["t"][~hit]))
    assert np.all(got["node"][~hit] == -1) and np.all(got["sub"][~hit] == -1) and np.all(got["material"][~hit] == -1)
    assert not np.ascontiguousarray(got["position"][~hit]).view(np.uint64).any() and not np.ascontiguousarray(got["normal"][~hit]).view(np.uint64).any()
    if "occluded" in got:
        assert np.array_equal(got["occluded"], hit.astype(np.uint8)), "occluded != (node >= 0)"
    return dict(hit=hit, t=got["t"], node=got["node"], sub=got["sub"], point=got["position"], normal=got["normal"])


def check(tag, c, which, got, flat, tol, ok):
    """got (a device record) against the exact answer `which` of the fixture on the rays `ok`; prints what was compared."""
    exp = G.expected(c, which)
    rec = as_exact(got)
    bad = ok & ~G.agreement(exp, rec, tol)
    other = np.zeros(len(ok), dtype=bool)
    if which.startswith("kd"):
        other[c[which + "_idx"]] = True
    via_alt = other & c["q1"] & G.agreement(G.expected(c, "alt"), rec, tol) if which == "kd" else np.zeros(len(ok), dtype=bool)
    print("%s: %d rays compared (%d hits), %d left out as fragile, %d answered by the Q1 alternative, %d more not as the flat walk"
          % (tag, int(ok.sum()), int((ok & exp["hit"]).sum()), int((~ok).sum()), int((via_alt & ok).sum()), int((other & ok & ~via_alt).sum())))
    assert not bad.any(), "%s: %d rays disagree with the exact reference; %s" % (tag, int(bad.sum()), G.first_disagreement(exp, rec, bad))
    h = ok & exp["hit"]
    assert np.array_equal(got["material"][h], flat["material_expected"][exp["node"][h]]), "%s: material is not the exact node's" % tag
    mesh = np.isin(flat["prim_type"][exp["node"][h]], (2,))
    assert np.all(got["sub"][h][~mesh] == 0), "%s: sub must be 0 on anything but a mesh" % tag


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene", G.SCENES)
def test_nearest_hits_are_the_exact_ones(oracle, host, H, scenes, scene, mode):
    s, tol = scenes[scene], TOL[scene]
    c = s["rays"]
    tr, om = traversal(H, oracle, mode)
    r = host.Renderer(s["host"], tr, kd_depth=G.KD_DEPTH)
    got = r.rays(c["o"], c["d"])
    again = r.rays(c["o"], c["d"], reorder=True)
    occ = [r.rays(c["o"], c["d"], any_hit=True, reorder=ro)["occluded"] for ro in (False, True)]
    r.close()
    ok = decidable(c, mode)
    assert int((~ok).sum()) <= s["caps"], "too many rays left out as fragile"
    which = "kd" if mode == "kd" else "nearest"
    check("%s %s" % (scene, mode), c, which, got, s["flat"], tol, ok)
    same(got, again)
    exp = G.expected(c, which)
    for ro, x in zip((False, True), occ):
        assert np.array_equal(x[ok], exp["hit"][ok].astype(np.uint8)), "%s %s: any_hit (reorder=%s) is not the exact 'anything in range'" % (scene, mode, ro)
    # the device's arrays still equal the oracle's bit for bit on these batches
    ref = oracle_rays(oracle, s["ps"], c["o"], c["d"], om, G.KD_DEPTH, workers=4)
    compare("%s %s vs the oracle" % (scene, mode), as_aov(got), ref, s["flat"], hier=mode == "hier")
    if mode != "hier":
        assert np.array_equal(got["node"], ref["id"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene", G.SCENES)
def test_segments_end_a_millionth_before_and_after_the_hit(oracle, host, H, scenes, scene, mode):
    """t_max = t (1 + 2^-20): occluded, and the nearest hit unchanged. t_max = t (1 - 2^-20): only what the exact reference finds below that bound."""
    s, tol = scenes[scene], TOL[scene]
    c = s["rays"]
    r = host.Renderer(s["host"], traversal(H, oracle, mode)[0], kd_depth=G.KD_DEPTH)
    ok = decidable(c, mode, segment=True)
    assert int((~ok).sum()) <= s["caps"], "too many rays left out as fragile"
    for side, which in ((1, "kd_above" if mode == "kd" else "nearest"), (0, "kd_below" if mode == "kd" else "below")):
        t_max = np.ascontiguousarray(c["t_max"][:, side])
        exp = G.expected(c, which)
        for ro in (False, True):
            got = r.rays(c["o"], c["d"], t_max=t_max, reorder=ro)
            check("%s %s t_max %s reorder=%d" % (scene, mode, ("below", "above")[side], ro), c, which, got, s["flat"], tol, ok)
            occ = r.rays(c["o"], c["d"], any_hit=True, t_max=t_max, reorder=ro)["occluded"]
            assert np.array_equal(occ[ok], exp["hit"][ok].astype(np.uint8)), "%s %s: any_hit with t_max %s the hit" % (scene, mode, ("below", "above")[side])
    r.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene", G.SCENES)
def test_primary_visibility_is_the_exact_eye_rays_hit(oracle, host, H, scenes, scene, mode):
    s, tol = scenes[scene], TOL[scene]
    c = s["camera"]
    r = host.Renderer(s["host"], traversal(H, oracle, mode)[0], kd_depth=G.KD_DEPTH)
    aov = r.aov(c["cam"], G.CAM_W, G.CAM_H)
    r.close()
    got = {k: np.ascontiguousarray(aov[ka].reshape((G.CAM_W * G.CAM_H,) + aov[ka].shape[2:]))
           for k, ka in (("t", "depth"), ("position", "position"), ("normal", "normal"), ("node", "node"), ("sub", "sub"), ("material", "material"))}
    ok = decidable(c, mode)
    assert int((~ok).sum()) <= G.FRAGILE_CAP["camera"] * len(ok)
    check("%s %s camera" % (scene, mode), c, "kd" if mode == "kd" else "nearest", got, s["flat"], tol, ok)
