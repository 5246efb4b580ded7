"""The oracle's colours against an exact-arithmetic reading of the reference's shading (tests/exact_shade.py), on the fixtures of
tests/golden/exact_shading/.

tests/exact_shade.py restates material.rs, light.rs and ray.rs:139-148 in 256-bit arithmetic on top of exact_ref's cast(); its colours for six lit scenes
are committed (tools/gen_exact_shading.py). On every ray the exact reference can decide (the smallest comparison margin of its whole ray tree is at least
2^-30, its tree needs at most 96 casts and its own plain-f64 evaluation strays by less than 2^-31) the oracle's colour must lie within the scene's
threshold per channel, |d| / max(1, |c|): 64 times what the reference's own 53-bit evaluation strays from its 256-bit one, capped at 2^-24
(tolerances.json). po_color_rays draws ray i's random numbers from stream (0, i, 0) and takes one background per call, so each ray is handed over
behind i placeholder rays with its own background.

The comparisons need numpy only. The tests that re-evaluate the exact reference need mpmath and skip without it."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import gen_exact_shading as G  # noqa: E402
from scene_dsl import Cube, Light, Material, Node, Plane, Scene, Sphere  # noqa: E402

TOL = G.load_tolerances()
MODES = ("flat", "kd", "hier")
CASES = [(s, b) for s in G.SCENES for b in G.batches_of(s)]
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
        assert oracle.flatten(ps)["trans"].tobytes() == batch(s, "camera")["trans"].tobytes(), "%s is not the scene of the fixture" % s
        out[s] = (scene, ps)
    return out


FAR_O, FAR_D = np.array([3e7, 5e7, 7e7]), np.array([0.267, 0.535, 0.802])


def oracle_colors(oracle, ps, o, d, bg, mode):
    """po_color_rays with a background per ray: ray i behind i placeholder rays that start far outside every scene and point away from it."""
    om = {"flat": oracle.MODE_FLAT, "kd": oracle.MODE_KD, "hier": oracle.MODE_HIER}[mode]
    out = np.zeros((len(o), 3))
    for i in range(len(o)):
        oo = np.concatenate([np.tile(FAR_O, (i, 1)), o[i:i + 1]])
        dd = np.concatenate([np.tile(FAR_D, (i, 1)), d[i:i + 1]])
        out[i] = oracle.color_rays(ps, oo, dd, background=bg[i], mode=om, kd_depth=G.KD_DEPTH)[i]
    return out


def check_against_exact(tag, c, got, threshold, mode):
    exp = G.expected(c, mode)
    ok = G.decidable(c, mode)
    bad = ok & ~G.agreement(exp, got, threshold)
    with np.errstate(all="ignore"):
        err = np.max(np.abs(got - exp) / np.maximum(1.0, np.abs(exp)), axis=1)
    print("%s: %d rays compared, %d left out; largest error %.3g of %.3g allowed" % (tag, int(ok.sum()), int((~ok).sum()), float(np.max(err[ok], initial=0.0)), threshold))
    assert not bad.any(), "%s: %d rays disagree with the exact reference; %s" % (tag, int(bad.sum()), G.first_disagreement(c, exp, got, bad))
    return int(ok.sum())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene,name", CASES)
def test_oracle_colours_agree_with_the_exact_reference(oracle, packed, scene, name, mode):
    c = batch(scene, name)
    got = oracle_colors(oracle, packed[scene][1], c["o"], c["d"], c["bg"], mode)
    assert check_against_exact("%s %s %s" % (scene, name, mode), c, got, TOL[scene], mode) >= len(c["o"]) // 2


@pytest.mark.parametrize("scene", G.SCENES)
def test_oracle_camera_rays_are_the_fixtures(oracle, scene):
    c = batch(scene, "camera")
    w, h = (int(x) for x in c["size"])
    ys, xs = np.mgrid[0:h, 0:w]
    o, d = oracle.camera_rays(list(c["cam"]), w, h, np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float64))
    assert np.array_equal(o, c["o"]) and np.all(np.linalg.norm(d - c["d"], axis=1) <= 2.0 ** -48), "eye rays"


# ---- the fixtures themselves
@pytest.mark.parametrize("scene", G.SCENES)
def test_fixture_meets_the_input_conditions(scene):
    G.check_conditions(scene, {b: batch(scene, b) for b in G.batches_of(scene)})


def test_every_branch_is_covered_twenty_times():
    G.check_coverage({s: {b: batch(s, b) for b in G.batches_of(s)} for s in G.SCENES})


def test_tolerances_are_the_measured_deviations():
    assert G.FRAGILE == 2.0 ** -30 and G.SLACK == 64.0 and G.THRESHOLD_CAP == 2.0 ** -24 and G.MAX_CASTS == 96 and G.ILL == 2.0 ** -31
    tol = G.tolerances({s: {b: batch(s, b) for b in G.batches_of(s)} for s in G.SCENES})
    for s in G.SCENES:
        print("%s: deviation %.3g, threshold %.3g" % (s, tol[s]["deviation"], tol[s]["threshold"]))
        assert TOL[s] == tol[s]["threshold"] == G.SLACK * tol[s]["deviation"] and 0.0 < TOL[s] <= G.THRESHOLD_CAP


def test_the_recorded_events_are_the_evaluators():
    pytest.importorskip("mpmath", reason="mpmath is needed to evaluate the exact reference")
    import exact_shade
    assert exact_shade.EVENTS == G.EVENTS and [1 << k for k in range(len(G.EVENTS))] == [getattr(exact_shade, "EV_" + e.upper()) for e in G.EVENTS]
    assert (exact_shade.FRAGILE, exact_shade.PREC) == (G.FRAGILE, 256)


def test_generator_reproduces_a_batch_byte_for_byte():
    pytest.importorskip("mpmath", reason="mpmath is needed to re-evaluate the exact reference")
    scene, name = G.CHECK_BATCH
    with open(G.path(scene, name), "rb") as fh:
        assert G.npz_bytes(G.make_batch(scene, name, workers=min(8, os.cpu_count() or 1))) == fh.read()


@pytest.mark.parametrize("scene,name", CASES)
def test_fixture_equals_the_evaluator_on_a_slice(scene, name):
    """Every 24th ray recomputed in the flat walk: colour, fragility and what is recorded of the depth-0 hit."""
    pytest.importorskip("mpmath", reason="mpmath is needed to re-evaluate the exact reference")
    c = batch(scene, name)
    inputs = G.scene_inputs(scene)
    G._EX, G._RAYS = G.exact_scene(inputs), [(c["o"][k], c["d"][k]) for k in range(len(c["o"]))]
    for k in range(0, len(c["o"]), 24):
        r = G._evaluate(k)
        assert r["bad"] == bool(c["bad"][k]), (scene, name, k)
        if r["casts"] <= G.MAX_CASTS:
            assert r["rgb"] == c["rgb"][k].tolist() and (r["margin"] < G.FRAGILE) == bool(c["fragile"][k]), (scene, name, k)
            assert (r["node"], r["branch"], r["casts"], r["deepest"], r["events"]) == tuple(int(c[q][k]) for q in ("node", "branch", "casts", "deepest", "events"))


# ---- the evaluator: closed forms worked by hand, independent of the scenes
def exact(nodes, lights=(), ambient=(0.0, 0.0, 0.0)):
    pytest.importorskip("mpmath", reason="mpmath is needed to evaluate the exact reference")
    import exact_shade
    import oracle_lib
    scene = Scene(Node.group(list(nodes)), list(lights), ambient)
    return exact_shade.ExactScene(scene, oracle_lib.flatten(oracle_lib.pack(scene))["trans"])


KD, KS, AMB, LC = (0.5, 0.25, 0.125), (0.25, 0.5, 0.75), (0.5, 0.25, 1.0), (1.0, 0.5, 0.25)


def test_closed_form_one_sphere_one_light_at_normal_incidence():
    """Hit (0, 0, 1), normal, view and light direction all +z: n.l = n.h = 1, the light 4 away, falloff 1 + 4/2 + 16/4 = 7."""
    ex = exact([Node.geo(Sphere(), Material(diffuse=KD, specular=KS, shininess=8.0))], [Light(position=(0, 0, 5), color=LC, falloff=(1.0, 0.5, 0.25))], AMB)
    s = ex.color((0, 0, 3), (0, 0, -1), (9, 9, 9))
    assert s.rgb() == [a * kd + (kd * lc + ks * lc) / 7.0 for a, kd, ks, lc in zip(AMB, KD, KS, LC)]
    assert (s.node, s.branch, s.shadowed, s.casts, s.deepest, s.depth11) == (0, 0, 0, 2, 0, False)
    assert ex.color((0, 0, 3), (0, 0, 1), (0.25, 0.5, 0.75)).rgb() == [0.25, 0.5, 0.75]           # a miss is the background
    # an occluder beyond the light still shadows (material.rs:176): a second sphere behind the light leaves the ambient term only
    ex = exact([Node.geo(Sphere(), Material(diffuse=KD, specular=KS, shininess=8.0)), Node.geo(Sphere(), Material()).translated((0, 0, 9))],
               [Light(position=(0, 0, 5), color=LC, falloff=(1.0, 0.5, 0.25))], AMB)
    s = ex.color((0, 0, 3), (0, 0, -1), (9, 9, 9))
    assert s.rgb() == [a * kd for a, kd in zip(AMB, KD)] and (s.shadowed, s.shadowed_beyond) == (1, 1)


def test_closed_form_specular_of_exactly_epsilon_gives_none():
    light = [Light(position=(0, 0, 5), color=LC)]
    colour = lambda ks: exact([Node.geo(Sphere(), Material(diffuse=KD, specular=(ks, 0.0, 0.0), shininess=8.0))], light).color((0, 0, 3), (0, 0, -1), (0, 0, 0)).rgb()
    assert colour(1e-5) == [kd * lc for kd, lc in zip(KD, LC)]
    above = math.nextafter(1e-5, 1.0)
    assert colour(above) == [KD[0] * LC[0] + above * LC[0], KD[1] * LC[1], KD[2] * LC[2]] != colour(1e-5)


def test_closed_form_mirror_facing_mirror_reaches_depth_11_and_returns_the_background():
    mirror = lambda z: Node.geo(Cube(), Material(reflectivity=0.5)).scaled((4.0, 4.0, 0.5)).translated((0, 0, z))
    s = exact([mirror(2.0), mirror(-2.0)]).color((0, 0, 0), (0, 0, 1), (0.25, 0.5, 1.0))
    assert s.rgb() == [0.25 * 2.0 ** -11, 0.5 * 2.0 ** -11, 2.0 ** -11]                           # eleven hits at depths 0..10, each halves; depth 11 is the background
    assert (s.casts, s.deepest, s.depth11, s.branch) == (12, 10, True, 1)


def test_closed_form_schlick_at_normal_incidence_is_r0():
    """A glass plane under a self-lit sphere (ambient 1, no lights): reflected colour A = the sphere's diffuse, refracted colour B = the background."""
    a, b = (0.25, 0.5, 0.75), (0.5, 0.125, 0.0625)
    ex = exact([Node.geo(Plane(), Material(reflectivity=0.75, refraction_index=1.5)).scaled((4.0, 1.0, 4.0)),
                Node.geo(Sphere(), Material(diffuse=a)).translated((0, 5, 0))], [], (1.0, 1.0, 1.0))
    s = ex.color((0, 1, 0), (0, -1, 0), b)
    r0 = 0.25 / 6.25
    assert s.rgb() == pytest.approx([0.75 * (r0 * x + (1.0 - r0) * y) for x, y in zip(a, b)], rel=1e-15) and s.branch == 2
    # leaving, from below: -normal and 1/eta; at normal incidence the refracted direction is the ray's, cos_incident 1 again
    s = ex.color((0, -1, 0), (0, 1, 0), b)
    assert s.rgb() == pytest.approx([0.75 * (r0 * y + (1.0 - r0) * x) for x, y in zip(a, b)], rel=1e-15) and s.branch == 3
    # beyond the critical angle from below (sin > 1/1.5): total internal reflection adds reflectivity * reflected colour
    s = ex.color((0, -1, 0), (0.8, 0.6, 0), b)
    assert s.rgb() == [0.75 * y for y in b] and s.branch == 4
    # ... by the direction as given: (1, 1, 0) is steeper still, but its ray_dir.dot(normal) is 1, so 1 - dot^2 is 0 and the ray leaves
    assert ex.color((0, -1, 0), (1, 1, 0), b).branch == 3


def test_closed_form_a_direction_scaled_by_two_changes_the_specular_term_only():
    light = [Light(position=(3, 4, 5), color=LC, falloff=(1.0, 0.25, 0.125))]
    def colours(ks):
        ex = exact([Node.geo(Sphere(), Material(diffuse=KD, specular=ks, shininess=8.0))], light, AMB)
        return [ex.color((0, 0, 3), (0, 0, -length), (0, 0, 0)).rgb() for length in (1.0, 2.0)]
    one, two = colours((0.0, 0.0, 0.0))
    assert one == two
    s1, s2 = colours(KS)
    assert s1 != s2
    # by hand: hit (0, 0, 1), l = (3, 4, 4) / sqrt(41), half = normalize((0, 0, length) + l), n.h = half.z, exponent 32
    r = math.sqrt(41.0)
    for length, got in ((1.0, s1), (2.0, s2)):
        hz = (length + 4.0 / r) / math.sqrt(9.0 / 41.0 + 16.0 / 41.0 + (length + 4.0 / r) ** 2)
        att = 1.0 + 0.25 * r + 0.125 * 41.0
        assert got == pytest.approx([a * kd + (kd * lc * 4.0 / r + ks * lc * hz ** 32) / att for a, kd, ks, lc in zip(AMB, KD, KS, LC)], rel=1e-14)
