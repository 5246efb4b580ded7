"""The oracle's ray queries against an exact-arithmetic reading of the reference (tests/exact_ref.py), on the fixtures of tests/golden/exact/.

The oracle and the kernels were written from one reading of the Rust sources; tests/exact_ref.py is a second one, in 256-bit arithmetic, and its answers
for four scenes and 2,560 rays each are committed (tools/gen_exact_rays.py). On every ray the exact reference can decide (its smallest comparison margin
is at least 2^-30) the oracle's hit / node must be the exact one, and t, point and unit normal must lie within the scene's thresholds: 64 times what the
reference's own plain-f64 evaluation strays from its 256-bit one (tolerances.json; measured from the reference alone, capped at 2^-32). The margin, the
factor 64 and the caps on the shares of fragile rays were fixed before anything was measured.

The comparisons need numpy only. The tests that re-evaluate the exact reference need mpmath and skip without it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import gen_exact_rays as G  # noqa: E402
from scene_dsl import CONE, CUBE, CYLINDER, Cone, Cube, Cylinder, Material, Node, Plane, Scene, Sphere, Triangle  # noqa: E402

BATCH_NAMES = tuple(b for b, _ in G.BATCHES)
TOL = G.load_tolerances()
_cache = {}


def batch(scene, name):
    if (scene, name) not in _cache:
        _cache[scene, name] = G.load(scene, name)
    return _cache[scene, name]


@pytest.fixture(scope="module")
def packed(oracle):
    out = {}
    for s in G.SCENES:
        scene = G.build_scene(s)
        ps = oracle.pack(scene)
        flat = oracle.flatten(ps)
        c = batch(s, "random")
        assert flat["trans"].tobytes() == c["trans"].tobytes() and np.array_equal(flat["prim_type"], c["prim_type"]), "%s is not the scene of the fixture" % s
        assert len(set(flat["material"].tolist())) == len(flat["material"]), "every node has a material of its own"
        tree = oracle.kd_scene_dump(ps, kd_depth=G.KD_DEPTH)
        assert all(np.array_equal(tree[k], c["tree_" + k]) for k in tree), "%s: the k-d tree is not the fixture's" % s
        out[s] = (scene, ps, flat)
    return out


def oracle_answer(oracle, ps, o, d, mode, with_id):
    t, ids, pt, nr = oracle.cast_rays(ps, o, d, mode=mode, kd_depth=6)
    hit = np.isfinite(t)
    assert np.array_equal(hit, ids >= 0)
    with np.errstate(all="ignore"):
        n = nr / np.linalg.norm(nr, axis=1)[:, None]
    n[~hit] = 0.0
    got = dict(hit=hit, t=t, point=pt, normal=n)
    if with_id:
        got["node"] = ids
    return got


def check_against_exact(tag, c, got, tol, mode):
    """mode: "flat", "hier", or "kd": there the exact answer is the exact walk of the scene's k-d tree, which on some rays is not the flat walk's
    (quirks Q1 and Q3 of SURVEY App. D); how many, and how many of those are the Q1 alternative, is printed. Returns (compared, left out, Q1 alternatives)."""
    exp = G.expected(c, "kd" if mode == "kd" else "nearest")
    decidable = ~c["kd_fragile"] if mode == "kd" else ~c["fragile"] & (~c["hier_fragile"] if mode == "hier" else True)
    agree = G.agreement(exp, got, tol)
    other = np.zeros(len(agree), dtype=bool)
    other[c["kd_idx"]] = mode == "kd"
    via_alt = other & c["q1"] & G.agreement(G.expected(c, "alt"), got, tol)
    bad = decidable & ~agree
    n = (int(decidable.sum()), int((~decidable).sum()), int((via_alt & decidable).sum()))
    print("%s: %d rays compared, %d left out as fragile, %d answered by the Q1 alternative, %d more not as the flat walk (Q3)"
          % ((tag,) + n + (int((other & decidable & ~via_alt).sum()),)))
    assert not bad.any(), "%s: %d rays disagree with the exact reference; %s" % (tag, int(bad.sum()), G.first_disagreement(exp, got, bad))
    return n


@pytest.mark.parametrize("mode", ["flat", "kd", "hier"])
@pytest.mark.parametrize("name", BATCH_NAMES)
@pytest.mark.parametrize("scene", G.SCENES)
def test_oracle_agrees_with_the_exact_reference(oracle, packed, scene, name, mode):
    c = batch(scene, name)
    om = {"flat": oracle.MODE_FLAT, "kd": oracle.MODE_KD, "hier": oracle.MODE_HIER}[mode]
    # the hierarchical walk of the oracle reports no flattened index: hit, t, point and normal are what it is held to
    got = oracle_answer(oracle, packed[scene][1], c["o"], c["d"], om, with_id=mode != "hier")
    compared, left_out, _ = check_against_exact("%s %s %s" % (scene, name, mode), c, got, TOL[scene], mode)
    assert left_out <= G.FRAGILE_CAP[name] * len(c["hit"]) and compared + left_out == len(c["hit"])


@pytest.mark.parametrize("scene", G.SCENES)
def test_oracle_camera_agrees_with_the_exact_eye_rays(oracle, packed, scene):
    c = batch(scene, "camera")
    tol = TOL[scene]
    o, d = oracle.camera_rays(list(c["cam"]), G.CAM_W, G.CAM_H, c["xy"])
    assert np.array_equal(o, c["o"]), "the eye"
    assert np.all(np.linalg.norm(d - c["d"], axis=1) <= tol["normal"]["threshold"]), "eye ray directions"
    for mode, om in (("flat", oracle.MODE_FLAT), ("kd", oracle.MODE_KD), ("hier", oracle.MODE_HIER)):
        got = oracle_answer(oracle, packed[scene][1], o, d, om, with_id=mode != "hier")
        check_against_exact("%s camera %s" % (scene, mode), c, got, tol, mode)


# ---- the fixture itself
@pytest.mark.parametrize("scene", G.SCENES)
def test_fixture_meets_the_input_conditions(scene):
    bs = {b: batch(scene, b) for b in BATCH_NAMES + ("camera",)}
    for b, n in G.BATCHES:
        assert len(bs[b]["hit"]) == n
    G.check_conditions(scene, bs)


def test_tolerances_are_the_measured_deviations():
    assert G.FRAGILE == 2.0 ** -30 and G.SLACK == 64.0 and G.THRESHOLD_CAP == 2.0 ** -32
    for scene in G.SCENES:
        dev = np.zeros(3)
        for b in BATCH_NAMES + ("camera",):
            c = batch(scene, b)
            m = c["hit"] & ~c["fragile"] & c["hit53"] & (c["node53"] == c["node"])
            assert np.array_equal(c["hit53"][~c["fragile"]], c["hit"][~c["fragile"]]) and np.array_equal(c["node53"][~c["fragile"]], c["node"][~c["fragile"]])
            # the stored 53-bit columns (differences from the exact values, f32) give the recorded figures
            dt = np.max(np.abs(c["dt53"][m].astype(np.float64)) / np.maximum(1.0, np.abs(c["t"][m])))
            dn = np.max(np.linalg.norm(c["dnormal53"][m].astype(np.float64), axis=1))
            mk = c["kd_hit"] & ~c["kd_fragile"][c["kd_idx"]]
            if mk.any():
                dt = max(dt, np.max(np.abs(c["kd_dt53"][mk].astype(np.float64)) / np.maximum(1.0, np.abs(c["kd_t"][mk]))))
                dn = max(dn, np.max(np.linalg.norm(c["kd_dnormal53"][mk].astype(np.float64), axis=1)))
            assert dt == pytest.approx(c["dev53"][0], rel=1e-6) and dn == pytest.approx(c["dev53"][2], rel=1e-6), (scene, b)
            dev = np.maximum(dev, c["dev53"])
        for k, q in enumerate(("t", "point", "normal")):
            print("%s %s: deviation %.3g, threshold %.3g" % (scene, q, dev[k], TOL[scene][q]["threshold"]))
            assert TOL[scene][q]["deviation"] == dev[k] and TOL[scene][q]["threshold"] == G.SLACK * dev[k]
            assert 0.0 < TOL[scene][q]["threshold"] < G.THRESHOLD_CAP


@pytest.mark.parametrize("name", BATCH_NAMES + ("camera",))
@pytest.mark.parametrize("scene", G.SCENES)
def test_fixture_equals_the_evaluator_on_a_slice(packed, scene, name):
    """Every 16th ray recomputed; each hit point the exact reference can decide satisfies its surface's equation to 2^-200."""
    exact_ref = pytest.importorskip("exact_ref", reason="mpmath is needed to re-evaluate the exact reference")
    from mpmath import mp
    c = batch(scene, name)
    ex = exact_ref.ExactScene(packed[scene][0], c["trans"], c["prim_type"])
    dirs = None
    if name == "camera":
        cam = G.scene_camera(c["trans"], G.flat_prims(packed[scene][0]))
        assert [*cam.eye, *cam.center, *cam.up, cam.fovy_radians] == c["cam"].tolist()
        dirs = exact_ref.camera_rays(cam, G.CAM_W, G.CAM_H, c["xy"])[1]
        dirs53 = exact_ref.camera_rays(cam, G.CAM_W, G.CAM_H, c["xy"], prec=53)[1]
    for k in range(0, len(c["hit"]), 16):
        d = c["d"][k] if dirs is None else dirs[k]
        h = ex.cast(c["o"][k], d)
        assert bool(h) == bool(c["hit"][k]) and (h.margin < G.FRAGILE) == bool(c["fragile"][k]) and h.q1 == bool(c["q1"][k]), (scene, name, k)
        if not h:
            continue
        assert (float(h.t), h.node, h.sub, h.part) == (c["t"][k], c["node"][k], c["sub"][k], c["part"][k]), (scene, name, k)
        assert [float(x) for x in h.point] == c["point"][k].tolist() and [float(x) for x in h.normal] == c["normal"][k].tolist(), (scene, name, k)
        if not c["fragile"][k]:
            mp.prec = exact_ref.PREC
            try:
                res = exact_ref.implicit_residual(h.kind, h.part, h.model_point, ex.flat[h.node].geometry, h.sub)
                assert res < mp.mpf(2) ** -200, (scene, name, k, res)
                h53 = ex.cast(c["o"][k], dirs53[k] if name == "camera" else d, prec=53)
                dp = mp.sqrt(sum((a - b) ** 2 for a, b in zip(h53.point, h.point))) / max(1, mp.sqrt(sum(a * a for a in h.point)))
                assert float(dp) <= TOL[scene]["point"]["deviation"]
            finally:
                mp.prec = 53


def test_generator_reproduces_a_batch_byte_for_byte():
    pytest.importorskip("exact_ref", reason="mpmath is needed to re-evaluate the exact reference")
    scene, name = G.CHECK_BATCH
    with open(G.path(scene, name), "rb") as fh:
        assert G.npz_bytes(G.make_batch(scene, name, workers=1)) == fh.read()


# ---- the evaluator: closed forms worked by hand
def single(prim):
    exact_ref = pytest.importorskip("exact_ref", reason="mpmath is needed to evaluate the exact reference")
    return exact_ref.ExactScene(Scene(Node.group([Node.geo(prim, Material())]), [], (0.0, 0.0, 0.0)), np.eye(4)[None])


def values(h):
    return float(h.t), [float(x) for x in h.point], [float(x) for x in h.normal]


def test_closed_form_sphere():
    s = single(Sphere())
    assert values(s.cast((0, 0, 5), (0, 0, -1))) == (4.0, [0.0, 0.0, 1.0], [0.0, 0.0, 1.0])
    assert values(s.cast((0, 0, 5), (0, 0, -4)))[0] == 1.0                      # t is in units of the direction
    assert values(s.cast((0, 0, 1), (0, 0, -1)))[0] == 2.0                      # the root at 0 is below EPSILON: the far side
    assert values(s.cast((0, 0, 0), (0, 1, 0))) == (1.0, [0.0, 1.0, 0.0], [0.0, 1.0, 0.0])   # from inside
    assert not s.cast((0, 0, 5), (0, 0, -1), t_max=4.0) and s.cast((0, 0, 5), (0, 0, -1), t_max=4.0 + 2.0 ** -40)   # the range is half open
    assert not s.cast((0, 2, 5), (0, 0, -1)) and not s.cast((0, 0, 5), (0, 0, 1))
    graze = s.cast((0, 1, 5), (0, 0, -1))                                       # tangent: one root, and nothing safe about it
    assert values(graze)[0] == 5.0 and graze.margin == 0.0


def test_closed_form_cylinder():
    c = single(Cylinder())
    h = c.cast((0, 5, 0), (0, -1, 0))                                          # down the axis: the top cap
    assert values(h) == (4.5, [0.0, 0.5, 0.0], [0.0, 1.0, 0.0]) and h.part == 1
    h = c.cast((0.25, -5, 0), (0, 1, 0))
    assert values(h) == (4.5, [0.25, -0.5, 0.0], [0.0, -1.0, 0.0]) and h.part == 2
    h = c.cast((5, 0.25, 0), (-1, 0, 0))
    assert values(h) == (4.5, [0.5, 0.25, 0.0], [1.0, 0.0, 0.0]) and h.part == 0
    assert not c.cast((5, 0.75, 0), (-1, 0, 0))
    h = c.cast((0, 0, 0), (0, 0, 2))                                           # from inside: the body's far root
    assert values(h) == (0.25, [0.0, 0.0, 0.5], [0.0, 0.0, 1.0])
    # Q1: the first body root is above the top cap, so the body reports a miss although the second root is on it; the caps still answer
    h = c.cast((1.0, 1.25, 0), (-1, -1, 0))
    assert h.q1 and h.part == 1 and values(h)[0] == 0.75
    assert c.cast((1.0, 1.25, 0), (-1, -1, 0), alt=True).part == 1             # the cap is nearer than the second root here


def test_closed_form_cone():
    c = single(Cone())
    apex = c.cast((0, 5, 0), (0, -1, 0))                                       # onto the apex: a double root, a normal of length 0
    assert float(apex.t) == 4.5 and apex.part == 0 and apex.margin == 0.0
    h = c.cast((5, 0.25, 0), (-1, 0, 0))                                       # from the side: radius 0.125 at y = 0.25
    t, p, n = values(h)
    assert (t, p) == (4.875, [0.125, 0.25, 0.0]) and h.part == 0 and not h.q1
    assert n == pytest.approx([2 / 5 ** 0.5, 1 / 5 ** 0.5, 0.0], abs=1e-15)    # outward: the gradient of x^2 + z^2 - (y - 1/2)^2 / 4
    h = c.cast((0.125, -5, 0), (0, 1, 0))
    assert values(h) == (4.5, [0.125, -0.5, 0.0], [0.0, -1.0, 0.0]) and h.part == 2
    # Q1: from above through the mirror nappe (y = 0.75 at radius 0.125): the body reports a miss, the cap answers; the alternative is the body
    h = c.cast((0.125, 2, 0), (0, -1, 0))
    assert h.q1 and h.part == 2 and float(h.t) == 2.5
    a = c.cast((0.125, 2, 0), (0, -1, 0), alt=True)
    assert a.part == 0 and float(a.t) == 1.75
    h = c.cast((0.125, 0.6, 0), (0, -1, 0))                                    # started below the mirror nappe's crossing: only the real cone is ahead
    assert not h.q1 and h.part == 0 and float(h.t) == pytest.approx(0.35, abs=1e-15)


def test_closed_form_cube_and_plane():
    c = single(Cube())
    h = c.cast((2, 2, 2), (-1, -1, -1))                                        # a corner: three faces tie and the first in the reference's order wins
    assert values(h) == (1.5, [0.5, 0.5, 0.5], [1.0, 0.0, 0.0]) and h.part == 0 and h.margin == 0.0
    for k, (o, n) in enumerate((((3, 0.25, 0.125), (1, 0, 0)), ((-3, 0.25, 0.125), (-1, 0, 0)), ((0.25, 3, 0.125), (0, 1, 0)), ((0.25, -3, 0.125), (0, -1, 0)),
                                ((0.25, 0.125, 3), (0, 0, 1)), ((0.25, 0.125, -3), (0, 0, -1)))):
        h = c.cast(o, tuple(-x for x in n))
        assert float(h.t) == 2.5 and h.part == k and [float(x) for x in h.normal] == [float(x) for x in n]
    assert c.cast((3, 0.5 + 5e-6, 0), (-1, 0, 0)) and not c.cast((3, 0.5 + 2e-5, 0), (-1, 0, 0))   # `contains` is padded by EPSILON
    assert float(c.cast((0, 0, 0), (0, 0, 1)).t) == 0.5                       # from inside: planes are two-sided
    p = single(Plane())
    assert values(p.cast((0.25, 1, 0.25), (0, -2, 0))) == (0.5, [0.25, 0.0, 0.25], [0.0, 1.0, 0.0])
    assert values(p.cast((0.25, -1, 0.25), (0, 2, 0)))[2] == [0.0, 1.0, 0.0]   # from below: the same normal
    assert p.cast((0.5 + 5e-6, 1, 0), (0, -1, 0)) and not p.cast((0.5 + 2e-5, 1, 0), (0, -1, 0))
    assert not p.cast((0, 1, 0), (1, 0, 0))                                    # parallel: a division by zero, no hit


def test_closed_form_triangle():
    t = single(Triangle((0, 0, 0), (1, 0, 0), (0, 1, 0)))
    h = t.cast((1, 0, 1), (0, 0, -1))                                          # the vertex b: beta = 1 and gamma = 0 are inside the bounds as written
    assert values(h) == (1.0, [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]) and h.margin == 0.0
    assert t.cast((0.5, 0.5, 1), (0, 0, -1)) and not t.cast((0.5, 0.5 + 2.0 ** -40, 1), (0, 0, -1))   # the edge beta = 1 - gamma
    assert values(t.cast((0.25, 0.25, -1), (0, 0, 1)))[2] == [0.0, 0.0, 1.0]   # from behind: the same flat normal, (b - a) x (c - a)
    s = single(Triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), normals=[(0, 0, 1), (1, 0, 0), (0, 1, 0)]))
    h = s.cast((0.25, 0.5, 1), (0, 0, -1))                                     # alpha, beta, gamma = 1/4, 1/4, 1/2
    assert [float(x) for x in h.normal] == pytest.approx([0.25 / 0.375 ** 0.5, 0.5 / 0.375 ** 0.5, 0.25 / 0.375 ** 0.5], abs=1e-15) and h.part == 1


def test_hierarchy_equals_the_composed_matrices():
    """Three levels with a mirroring scale: descending level by level picks the leaf, t and normal that the composed matrix gives."""
    exact_ref = pytest.importorskip("exact_ref", reason="mpmath is needed to evaluate the exact reference")
    from mpmath import mp
    scene = G.build_scene("nested15")
    c = batch("nested15", "random")
    ex = exact_ref.ExactScene(scene, c["trans"], c["prim_type"])
    assert [n.geometry.kind for n in ex.flat].count(CUBE) == 3 and {CONE, CYLINDER} <= set(ex.kinds())
    mp.prec = exact_ref.PREC
    try:
        for i in range(len(ex.flat)):   # the f64 matrices of the flattened scene are the per-level products, rounded
            m = ex.composed(i)
            assert all(abs(float(m[r][q]) - c["trans"][i][r][q]) <= 2.0 ** -48 * max(1.0, abs(c["trans"][i][r][q])) for r in range(3) for q in range(4))
    finally:
        mp.prec = 53
    for k in range(0, 256, 8):
        f, h = ex.cast(c["o"][k], c["d"][k]), ex.cast(c["o"][k], c["d"][k], mode="hier")
        assert bool(f) == bool(h)
        if f:
            assert (f.node, f.sub, f.part) == (h.node, h.sub, h.part) and float(h.t) == pytest.approx(float(f.t), rel=2.0 ** -40)
            assert [float(x) for x in h.normal] == pytest.approx([float(x) for x in f.normal], abs=2.0 ** -40)
