"""The direct-light pass (pt_direct / pt_direct_device / Renderer.direct / direct_camera / direct_chart) on the GPU, bit for bit.

The yardstick is what exists: the numpy restatement of the contract (tests/direct_restate.py, equal to the host replay in every bit by tests/test_direct_contract.py)
makes each point's shadow rays and terms, Renderer.rays(o, d, any_hit=True, t_max=...) - pinned to the oracle by tests/test_gpu_segments.py - answers the rays,
numpy adds the terms in contract order. `sum`, `lit` and `valid` are compared exactly. The points are what Renderer.aov finds under a 67 x 37 image (2,479
points, 39 wavefronts, the last ragged; misses are invalid points), the normals turned towards the camera's eye."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import host_glue  # noqa: E402
from direct_restate import accumulate, restate  # noqa: E402
from scene_dsl import ASSETS, Camera, Cube, Light, Material, Node, Plane, Scene, Sphere, default_background  # noqa: E402

pytestmark = pytest.mark.gpu

W, HT = 67, 37
NPTS = W * HT
SEED = 7
TRAVERSALS = ("flat", "hier", "kd")
SAMPLES = {"big-scene": 1, "macho-cows": 1, "soft-shadows": 16, "many65": 1}
# macho-cows from the side of its one light's shadows (the example's own camera sees 5 % of its points shadowed): eye, centre, up, fovy
COWS_CAM = np.array([-8.0, 3.0, 10.0, 0.0, -1.0, 0.0, 0.0, 1.0, 0.0, np.radians(50.0)])
WANT = ("sum", "lit", "valid")


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def traversal(H, mname):
    return {"flat": H.TRAVERSE_FLAT, "kd": H.TRAVERSE_KD, "hier": H.TRAVERSE_HIER}[mname]


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def close_renderers():
    yield
    for c in _CASES.values():
        c["r"].close()
    _CASES.clear()


def scene_of(host, which):
    """(host scene, cam10)"""
    if which == "many65":
        import gen_exact_shading as G
        return host_glue.host_scene(G.build_scene("many65")), host_glue.cam10(G.scene_camera("many65", None, None))
    sc = host.Scene.example(which, assets=ASSETS)
    return sc, (COWS_CAM if which == "macho-cows" else np.array(sc.camera, dtype=np.float64))


def lights_of(hs):
    """the scene's light records, n_lights x 15 (the export pads an empty list)"""
    ex = hs.export()
    return np.ascontiguousarray(np.asarray(ex["lights"], dtype=np.float64).reshape(-1, 15)[:int(ex["n_lights"])])


def points_of(host, r, cam):
    aov = r.aov(cam, W, HT, want=("position", "normal", "node"))
    P, N = np.ascontiguousarray(aov["position"].reshape(-1, 3)), np.ascontiguousarray(aov["normal"].reshape(-1, 3))
    eye = np.array(list(host.camera(cam, W, HT).eye))
    return P, N, eye, aov["node"].ravel() >= 0


def case(host, H, which, mname, make=None):
    """A renderer of the scene in one traversal, its lights, the points under its image and the camera's eye: made once, shared, never written to."""
    key = (which, mname)
    if key not in _CASES:
        sc, cam = make() if make else scene_of(host, which)
        r = host.Renderer(sc, traversal(H, mname), kd_depth=10)
        P, N, eye, hit = points_of(host, r, cam)
        lights = lights_of(sc)
        for a in (P, N, eye, lights):
            a.setflags(write=False)
        _CASES[key] = dict(sc=sc, cam=cam, r=r, P=P, N=N, eye=eye, hit=hit, lights=lights, refs={})
    return _CASES[key]


def reference(r, P, N, lights, S, to_light=False, seed=SEED, pas=0, first=0, bias=0.0, eye=None, normalise=True):
    """What the contract says, from the existing pass: (sum f64, lit u32, valid u8, casts (n, L, S) bool, occluded (n, L, S) u8)."""
    O, D, T, E, valid = restate(P, N, lights, S, seed, pas, first, bias, eye, to_light, normalise)
    n, L, _ = T.shape
    occ = np.zeros((n, L, S), dtype=np.uint8)
    if n and L:
        oo = np.ascontiguousarray(np.repeat(O, L * S, axis=0))
        occ = r.rays(oo, np.ascontiguousarray(D.reshape(-1, 3)), any_hit=True, t_max=np.ascontiguousarray(T.ravel()))["occluded"].reshape(n, L, S)
    total, lit = accumulate(T, E, valid, occ)
    return total, lit, valid, T > 0.0, occ


def case_reference(c, S, to_light=False, **kw):
    key = (S, to_light, tuple(sorted(kw.items())))
    if key not in c["refs"]:
        ref = reference(c["r"], c["P"], c["N"], c["lights"], S, to_light, eye=c["eye"], **kw)
        for a in ref:
            a.setflags(write=False)
        c["refs"][key] = ref
    return c["refs"][key]


def check(tag, got, ref):
    total, lit, valid = ref[:3]
    assert got["sum"].dtype == np.float64 and got["lit"].dtype == np.uint32 and got["valid"].dtype == np.uint8
    assert np.array_equal(got["valid"], valid), f"{tag}: valid"
    bad = np.flatnonzero(got["lit"] != lit)
    assert not len(bad), f"{tag}: lit differs at {len(bad)} points, first {bad[:5]}: {got['lit'][bad[:5]]} != {lit[bad[:5]]}"
    bad = np.flatnonzero((bits(got["sum"]) != bits(total)).any(axis=1))
    assert not len(bad), f"{tag}: sum differs at {len(bad)} points, first {bad[:3]}: {got['sum'][bad[:3]]} != {total[bad[:3]]}"


def guards(tag, ref, L, S):
    """The identity must not pass on emptiness: conditions on the REFERENCE side (they were met on the CPU oracle's visibility before any of this ran)."""
    total, lit, valid, casts, occ = ref
    v = valid == 1
    per_light = (casts & (occ == 0)).sum(axis=2)
    partly = int((v & (lit > 0) & (lit < L * S)).sum())
    some_dark = int((v & (per_light == 0).any(axis=1) & (per_light > 0).any(axis=1)).sum())
    shadowed = int((v & casts.any(axis=(1, 2)) & (lit == 0)).sum())
    print(f"{tag}: {int(v.sum())} valid points of {len(v)}, {partly} with 0 < lit < {L * S}, {some_dark} with a light dark and another lit, {shadowed} in full shadow, "
          f"{int(casts.sum())} rays cast, {int((casts & (occ == 1)).sum())} occluded")
    assert v.sum() > 1000
    if L > 1:
        assert 10 * partly >= v.sum() and 10 * some_dark >= v.sum(), tag
    else:  # one point light: a point is lit or not; a tenth of the valid points each way
        assert 10 * shadowed >= v.sum() and 10 * int((v & (lit > 0)).sum()) >= v.sum(), tag


# ---- 1. the identity: every scene, every traversal, bounded and unbounded
@pytest.mark.parametrize("mname", TRAVERSALS)
@pytest.mark.parametrize("which", list(SAMPLES))
def test_sum_lit_and_valid_equal_the_restated_terms_where_the_ray_queries_see_the_light(host, H, which, mname):
    c = case(host, H, which, mname)
    S, L = SAMPLES[which], len(c["lights"])
    for to_light in (False, True):
        ref = case_reference(c, S, to_light)
        guards(f"{which} {mname} to_light={to_light}", ref, L, S)
        assert np.array_equal(ref[2], c["hit"].astype(np.uint8)), "aov's misses are the invalid points"
        got = c["r"].direct(c["P"], c["N"], samples=S, seed=SEED, eye=c["eye"], to_light=to_light, want=WANT)
        check(f"{which} {mname} to_light={to_light}", got, ref)
        assert np.array_equal(bits(got["mean"]), bits(ref[0] / float(S))) and got["kernel_ms"] > 0.0
    assert L == {"big-scene": 3, "macho-cows": 1, "soft-shadows": 2, "many65": 65}[which]


@pytest.mark.parametrize("mname", TRAVERSALS)
@pytest.mark.parametrize("S", (1, 64))
def test_other_sample_counts_on_the_area_light(host, H, mname, S):
    c = case(host, H, "soft-shadows", mname)
    for to_light in (False, True):
        ref = case_reference(c, S, to_light)
        assert 0 < ref[1].sum() < 2 * S * ref[2].sum()
        check(f"soft-shadows {mname} S={S} to_light={to_light}", c["r"].direct(c["P"], c["N"], samples=S, seed=SEED, eye=c["eye"], to_light=to_light, want=WANT), ref)
    if S == 64:
        a, b = case_reference(c, 64), case_reference(c, 64, pas=1)
        assert not np.array_equal(bits(a[0]), bits(b[0])), "another pass samples the area light elsewhere"
        check(f"soft-shadows {mname} pass 1", c["r"].direct(c["P"], c["N"], samples=64, seed=SEED, pass_index=1, eye=c["eye"], want=WANT), b)


# ---- 2. to_light must matter
def between_floor_and_ceiling():
    grey = Material(diffuse=(0.6, 0.6, 0.6))
    floor = Node.geo(Cube(), grey).scaled((12.0, 0.2, 12.0)).translated((0.0, -0.1, 0.0))
    ceiling = Node.geo(Cube(), grey).scaled((60.0, 0.2, 60.0)).translated((0.0, 4.0, 0.0))
    scene = Scene(root=Node.group([floor, ceiling]), lights=[Light(position=(0.0, 2.0, 0.0), color=(0.9, 0.9, 0.9), falloff=(1.0, 0.0, 0.05))], ambient=(0.0, 0.0, 0.0))
    return host_glue.host_scene(scene), host_glue.cam10(Camera(eye=(0.0, 2.5, 9.0), center=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovy_degrees=45.0))


@pytest.mark.parametrize("mname", TRAVERSALS)
def test_a_light_between_floor_and_ceiling_reaches_the_floor_only_when_the_segment_ends_at_it(host, H, mname):
    c = case(host, H, "room", mname, between_floor_and_ceiling)
    floor = c["hit"] & (c["P"][:, 1] < 1.0)
    assert floor.sum() > 500
    out = {}
    for to_light in (False, True):
        ref = case_reference(c, 1, to_light)
        out[to_light] = c["r"].direct(c["P"], c["N"], samples=1, seed=SEED, eye=c["eye"], to_light=to_light, want=WANT)
        check(f"room {mname} to_light={to_light}", out[to_light], ref)
    assert not out[False]["lit"][floor].any(), "unbounded, the ceiling behind the light shadows every floor point"
    assert out[True]["lit"][floor].all() and (out[True]["sum"][floor] > 0.0).all(), "bounded, the floor is lit"
    assert 2 * int((out[False]["lit"][floor] != out[True]["lit"][floor]).sum()) > int(floor.sum())


# ---- 3. the light term against the render's
def spheres_over_a_plane():
    white = Material(diffuse=(1.0, 1.0, 1.0))
    nodes = [Node.geo(Plane(), white).scaled((12.0, 1.0, 12.0)).translated((0.0, -0.5, 0.0)),
             Node.geo(Sphere(), white).scaled(0.8).translated((-1.2, 0.6, 0.0)),
             Node.geo(Sphere(), white).scaled((1.0, 0.6, 0.7)).translated((1.3, 0.4, 0.4)),
             Node.geo(Sphere(), white).scaled(0.5).translated((0.2, 0.2, 1.8))]
    lights = [Light(position=(6.0, 14.0, 5.0), color=(0.9, 0.7, 0.5), falloff=(1.0, 0.05, 0.01)), Light(position=(-7.0, 12.0, -2.0), color=(0.3, 0.5, 0.8), falloff=(0.5, 0.0, 0.02))]
    scene = Scene(root=Node.group(nodes), lights=lights, ambient=(0.0, 0.0, 0.0))
    return host_glue.host_scene(scene), host_glue.cam10(Camera(eye=(0.5, 3.0, 7.0), center=(0.0, 0.3, 0.0), up=(0.0, 1.0, 0.0), fovy_degrees=40.0))


def test_the_restated_term_is_the_renders_light_term(host, H):
    """Renderer.radiance along the primary rays of the pixel centres - white diffuse material, no specular, no ambient, no reflection: the colour IS the sum of
    the light terms - equals the restatement with step 3 left out (aov's normals are unit already and the render does not normalise again) on aov's position and
    normal, visibility from Renderer.rays on that restatement's rays. This pins the restatement's term to a kernel pinned to the exact reference."""
    import oracle_lib as O
    c = case(host, H, "white", "flat", spheres_over_a_plane)
    cam = Camera(eye=tuple(c["cam"][0:3]), center=tuple(c["cam"][3:6]), up=tuple(c["cam"][6:9]), fovy_degrees=float(np.degrees(c["cam"][9])))
    ys, xs = np.mgrid[0:HT, 0:W]
    o, d = O.camera_rays(cam, W, HT, np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float64))
    rgb = c["r"].radiance(o, d, background=(0.0, 0.0, 0.0), seed=0)["rgb"]
    ref = reference(c["r"], c["P"], c["N"], c["lights"], 1, normalise=False)
    guards("white", ref, 2, 1)
    with_step3 = reference(c["r"], c["P"], c["N"], c["lights"], 1)
    diff = np.abs(rgb - ref[0])
    print("radiance against the restatement without step 3: max |difference| per channel", diff.max(axis=0), "; at", int((bits(rgb) != bits(ref[0])).any(axis=1).sum()),
          "points of", int(c["hit"].sum()), "; the restatement with against without step 3: max", np.abs(with_step3[0] - ref[0]).max(axis=0))
    assert np.array_equal(bits(rgb), bits(ref[0])), "0 x kd + (1 x colour) c / att is the restatement's arithmetic"


# ---- 4. shapes and edges
def test_batch_sizes_cuts_first_indices_and_repeats(host, H):
    c = case(host, H, "soft-shadows", "flat")
    r, P, N, eye = c["r"], c["P"], c["N"], c["eye"]
    run = lambda P, N, **kw: r.direct(np.ascontiguousarray(P), np.ascontiguousarray(N), samples=16, seed=SEED, eye=eye, want=WANT, **kw)
    whole = reference(r, P, N, c["lights"], 16, first=5000, eye=eye)
    got = run(P, N, first_index=5000)
    check("2,479 points", got, whole)
    again = run(P, N, first_index=5000)
    assert all(got[k].tobytes() == again[k].tobytes() for k in WANT), "the same call twice"
    for n in (1, 63, 64, 65):
        check(f"n={n}", run(P[700:700 + n], N[700:700 + n], first_index=5700), tuple(a[700:700 + n] for a in whole))
    a, b = run(P[:1000], N[:1000], first_index=5000), run(P[1000:], N[1000:], first_index=6000)
    check("cut at 1,000", {k: np.concatenate([a[k], b[k]]) for k in WANT}, whole)
    shifted = run(P[1000:], N[1000:], first_index=5000)
    assert not np.array_equal(bits(shifted["sum"]), bits(whole[0][1000:])), "first_index is part of the stream"
    big = 1 << 60
    check("first_index = 2^60", run(P[:200], N[:200], first_index=big), reference(r, P[:200], N[:200], c["lights"], 16, first=big, eye=eye))
    empty = run(np.zeros((0, 3)), np.zeros((0, 3)))
    assert empty["sum"].shape == (0, 3) and empty["lit"].shape == (0,) and empty["mean"].shape == (0, 3) and empty["kernel_ms"] == 0.0
    only = r.direct(P, N, samples=16, seed=SEED, first_index=5000, eye=eye, want=("lit",))  # one buffer alone
    assert sorted(only) == ["kernel_ms", "lit"] and np.array_equal(only["lit"], whole[1])
    far = run(P, N, bias=1e19)  # every origin beyond the ray queries' range: nothing traced
    assert not far["sum"].any() and not far["lit"].any() and np.array_equal(far["valid"], c["hit"].astype(np.uint8))
    check("bias 1/64", run(P, N, bias=0.015625), reference(r, P, N, c["lights"], 16, bias=0.015625, eye=eye))


@pytest.mark.parametrize("which,mname", [("soft-shadows", "flat"), ("big-scene", "kd"), ("many65", "hier")])
def test_invalid_points_report_zeros_and_change_no_neighbour(host, H, which, mname):
    c = case(host, H, which, mname)
    S = SAMPLES[which]
    ref = case_reference(c, S)
    P, N = c["P"].copy(), c["N"].copy()
    rng = np.random.default_rng(5)
    hit = np.flatnonzero(c["hit"])
    spoil = rng.choice(hit, size=len(hit) // 5, replace=False)  # scattered: nearly every wavefront holds some
    kind = np.arange(len(spoil)) % 5
    P[spoil[kind == 0], 1] = np.nan
    N[spoil[kind == 1]] = 0.0
    N[spoil[kind == 2], 2] = -np.inf
    P[spoil[kind == 3], 0] = 2e18
    P[spoil[kind == 4]], N[spoil[kind == 4]] = 0.0, 0.0  # what aov writes where nothing is hit
    want = [a.copy() for a in ref[:3]]
    for a in want:
        a[spoil] = 0
    got = c["r"].direct(P, N, samples=S, seed=SEED, eye=c["eye"], want=WANT)
    check(f"{which} {mname} with invalid points", got, tuple(want))
    assert not got["sum"][spoil].any() and not got["lit"][spoil].any() and not got["valid"][spoil].any() and want[1].sum() > 0
    nothing = c["r"].direct(np.full((130, 3), np.nan), np.ones((130, 3)), samples=4, want=WANT)  # wavefronts without a single ray
    assert not nothing["sum"].any() and not nothing["lit"].any() and not nothing["valid"].any()


def no_lights():
    grey = Material(diffuse=(0.6, 0.6, 0.6))
    scene = Scene(root=Node.group([Node.geo(Sphere(), grey), Node.geo(Plane(), grey).scaled((8.0, 1.0, 8.0)).translated((0.0, -1.0, 0.0))]), lights=[], ambient=(0.2, 0.2, 0.2))
    return host_glue.host_scene(scene), host_glue.cam10(Camera(eye=(0.0, 2.0, 6.0), center=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovy_degrees=40.0))


@pytest.mark.parametrize("mname", TRAVERSALS)
def test_a_scene_without_lights_gives_zeros_and_valid(host, H, mname):
    c = case(host, H, "dark", mname, no_lights)
    got = c["r"].direct(c["P"], c["N"], samples=4, eye=c["eye"], want=WANT)
    assert c["hit"].sum() > 1000 and np.array_equal(got["valid"], c["hit"].astype(np.uint8)) and not got["sum"].any() and not got["lit"].any()


# ---- 5. the chained forms
@pytest.mark.parametrize("mname", TRAVERSALS)
@pytest.mark.parametrize("which", ["big-scene", "soft-shadows"])
def test_direct_camera_equals_direct_fed_with_the_aov_arrays(host, H, which, mname):
    c = case(host, H, which, mname)
    S = SAMPLES[which]
    for to_light in (False, True):
        got = c["r"].direct_camera(c["cam"], W, HT, samples=S, seed=SEED, to_light=to_light, want=WANT)
        assert got["sum"].shape == (HT, W, 3) and got["mean"].shape == (HT, W, 3) and got["lit"].shape == (HT, W) and got["valid"].shape == (HT, W) and got["kernel_ms"] > 0.0
        check(f"{which} {mname} direct_camera to_light={to_light}", {k: got[k].reshape((NPTS,) + got[k].shape[2:]) for k in WANT}, case_reference(c, S, to_light))
    turned = int((((c["N"] * (c["P"] - c["eye"])).sum(axis=1) > 0.0) & c["hit"]).sum())
    print(f"{which} {mname}: {turned} first hits face away from the eye")
    if which == "big-scene":
        assert turned > 0, "PT_AO_FACE_EYE must have something to turn"


@pytest.mark.parametrize("size", [(64, 64), (67, 37)])
def test_direct_chart_equals_direct_fed_with_the_charts_arrays(host, H, size):
    from test_gpu_chart import _cube_among_soft_shadows_lights, cube_mesh, mesh_nodes
    hs = host_glue.host_scene(_cube_among_soft_shadows_lights())
    r = host.Renderer(hs, H.TRAVERSE_FLAT)
    try:
        node, uv = mesh_nodes(hs)[0], cube_mesh().tex_coords
        w, h = size
        ch = r.chart(node, w, h, uv)
        P, N = ch["position"].reshape(-1, 3), ch["normal"].reshape(-1, 3)
        for kw in (dict(samples=16, bias=1e-3, seed=5, pass_index=1), dict(samples=4, bias=1e-3, seed=5, to_light=True)):
            want = r.direct(P, N, first_index=0, want=WANT, **kw)
            got = r.direct_chart(node, w, h, uv, want=WANT, **kw)
            for k in WANT:
                assert got[k].reshape(want[k].shape).tobytes() == want[k].tobytes(), "direct_chart %s" % k
            assert np.array_equal(got["valid"] == 0, ch["covered"] == 0), "valid is 0 exactly on the uncovered texels"
            assert got["mean"].shape == (h, w, 3) and 0 < int(got["lit"].sum()) < 2 * kw["samples"] * int(got["valid"].sum())
        check("the chart's points", r.direct(P, N, samples=4, bias=1e-3, seed=5, want=WANT), reference(r, P, N, lights_of(hs), 4, seed=5, bias=1e-3))
    finally:
        r.close()


# ---- 6. a moved light
def lit_balls(shift):
    grey = Material(diffuse=(0.6, 0.6, 0.6))
    nodes = [Node.geo(Plane(), grey).scaled((10.0, 1.0, 10.0)).translated((0.0, -0.5, 0.0))]
    nodes += [Node.geo(Sphere(), grey).scaled(0.5).translated((-3.0 + 1.5 * k, 0.3 + 0.2 * shift * k, 0.5 * (k % 2))) for k in range(5)]
    lights = [Light(position=(4.0 - 6.0 * shift, 6.0, 3.0), color=(0.9, 0.8, 0.7), falloff=(1.0, 0.02, 0.01)),
              Light(position=(-3.0, 5.0 + shift, -2.0), color=(0.4, 0.5, 0.9), area_a=(0.8, 0.0, 0.0), area_b=(0.0, 0.0, 0.6 + shift))]
    return Scene(root=Node.group(nodes), lights=lights, ambient=(0.1, 0.1, 0.1))


@pytest.mark.parametrize("mname", TRAVERSALS)
def test_after_an_update_the_pass_answers_for_the_moved_lights(host, H, mname):
    cam = host_glue.cam10(Camera(eye=(0.0, 4.0, 9.0), center=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovy_degrees=45.0))
    ha, hb = host_glue.host_scene(lit_balls(0.0)), host_glue.host_scene(lit_balls(1.0))
    r, fresh = host.Renderer(ha, traversal(H, mname), kd_depth=8), host.Renderer(hb, traversal(H, mname), kd_depth=8)
    try:
        before = r.direct_camera(cam, W, HT, samples=8, seed=SEED, want=WANT)
        r.update(hb)
        moved, want = r.direct_camera(cam, W, HT, samples=8, seed=SEED, want=WANT), fresh.direct_camera(cam, W, HT, samples=8, seed=SEED, want=WANT)
        for k in WANT:
            assert moved[k].tobytes() == want[k].tobytes(), k
        P, N, eye, _ = points_of(host, fresh, cam)
        ref = reference(fresh, P, N, lights_of(hb), 8, eye=eye)
        check(f"moved lights {mname}", {k: want[k].reshape((NPTS,) + want[k].shape[2:]) for k in WANT}, ref)
        assert 0 < ref[1].sum() and not np.array_equal(bits(before["sum"]), bits(want["sum"]))
    finally:
        r.close()
        fresh.close()


# ---- 7. device buffers, and the pass among the others
def test_device_tensors_on_a_torch_stream_equal_the_host_path(H):
    """pt_direct_device with points and results in torch tensors on a stream of torch's, in a process of its own in which torch initialises its GPU side first;
    while it is open no second ray-query pass of any kind is accepted, pt_direct_finish closes it, and a buffer that is too short is refused before any kernel."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import os, sys, ctypes as C
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import torch
assert torch.cuda.is_available()
dev = torch.device("cuda:0")
x = torch.ones(1024, device=dev); torch.cuda.synchronize()
import numpy as np
from portrayer_amd import _hip as H
from portrayer_amd import host
from scene_dsl import ASSETS
lib = H.lib()
sc = host.Scene.example("soft-shadows", assets=ASSETS)
r = host.Renderer(sc, H.TRAVERSE_FLAT)
aov = r.aov(sc.camera, 67, 37, want=("position", "normal"))
P, N = np.ascontiguousarray(aov["position"].reshape(-1, 3)), np.ascontiguousarray(aov["normal"].reshape(-1, 3))
n = len(P)
eye = list(host.camera(sc.camera, 67, 37).eye)
ref = r.direct(P, N, samples=16, seed=7, pass_index=2, first_index=11, eye=eye, to_light=True, want=("sum", "lit", "valid"))
assert 0 < ref["lit"].sum() < 32 * ref["valid"].sum()
d_P, d_N = torch.from_numpy(P).to(dev), torch.from_numpy(N).to(dev)
t_sum = torch.full((n, 3), 5.0, dtype=torch.float64, device=dev)
t_lit = torch.full((n,), 5, dtype=torch.int32, device=dev)
t_valid = torch.full((n,), 5, dtype=torch.uint8, device=dev)
d_short = C.c_void_p()
assert lib.pt_device_alloc(r.context, 4096, C.byref(d_short)) == H.OK  # an allocation of its own (a tensor's may lie inside a larger block of torch's): 9,916 bytes are needed
torch.cuda.synchronize()
stream = torch.cuda.Stream(device=dev)
assert stream.cuda_stream != 0
ptr = lambda t, kind: C.cast(C.c_void_p(t.data_ptr()), kind)
b = H.PtDirectBuffers(ptr(t_sum, H._dp), ptr(t_lit, H._up), ptr(t_valid, H._u8p))
p = H.PtDirectParams(n, 16, 2, 7, 11, 0.0, H.AO_FACE_EYE | H.DIRECT_TO_LIGHT, (C.c_double * 3)(*eye))
# a buffer that is too short, and host memory, are refused before anything is queued: nothing is in flight afterwards
short = H.PtDirectBuffers(ptr(t_sum, H._dp), C.cast(d_short, H._up), ptr(t_valid, H._u8p))
assert lib.pt_direct_device(r.context, C.byref(p), C.c_void_p(d_P.data_ptr()), C.c_void_p(d_N.data_ptr()), C.byref(short), C.c_void_p(stream.cuda_stream)) == H.ERR_ARGUMENT
assert b"lit" in lib.pt_last_error(r.context)
assert lib.pt_direct_device(r.context, C.byref(p), C.c_void_p(P.ctypes.data), C.c_void_p(d_N.data_ptr()), C.byref(b), C.c_void_p(stream.cuda_stream)) == H.ERR_ARGUMENT
assert lib.pt_direct_finish(r.context, None) == H.ERR_ARGUMENT
torch.cuda.synchronize()
assert (t_sum == 5.0).all().item() and (t_lit == 5).all().item() and (t_valid == 5).all().item()
assert lib.pt_device_free(r.context, d_short) == H.OK
args = (r.context, C.byref(p), C.c_void_p(d_P.data_ptr()), C.c_void_p(d_N.data_ptr()), C.byref(b), C.c_void_p(stream.cuda_stream))
assert lib.pt_direct_device(*args) == H.OK, lib.pt_last_error(r.context)
assert lib.pt_direct_device(*args) == H.ERR_ARGUMENT  # one ray-query pass in flight per context ...
lit = np.full(n, 9, dtype=np.uint32)
hb = H.PtDirectBuffers(lit=lit.ctypes.data_as(H._up))
assert lib.pt_direct(r.context, C.byref(p), P.ctypes.data_as(H._dp), N.ctypes.data_as(H._dp), C.byref(hb), None) == H.ERR_ARGUMENT  # ... the host path included,
rp, flags = H.PtRaysParams(n, 1, 0), np.full(n, 9, dtype=np.uint8)
rb = H.PtRaysBuffers(occluded=flags.ctypes.data_as(H._u8p))
assert lib.pt_rays(r.context, C.byref(rp), P.ctypes.data_as(H._dp), N.ctypes.data_as(H._dp), C.byref(rb), None) == H.ERR_ARGUMENT  # the ray queries',
assert lib.pt_segments_device(r.context, C.byref(rp), C.c_void_p(d_P.data_ptr()), C.c_void_p(d_N.data_ptr()), C.c_void_p(d_P.data_ptr()), C.byref(rb), None) == H.ERR_ARGUMENT
occ = np.full(n, 9, dtype=np.uint32)
ap = H.PtAoParams(n, 16, 0, 7, 0, 3.0, 0.0, 0, (C.c_double * 3)(0.0, 0.0, 0.0))
ab = H.PtAoBuffers(occluded=occ.ctypes.data_as(H._up))
assert lib.pt_ao(r.context, C.byref(ap), P.ctypes.data_as(H._dp), N.ctypes.data_as(H._dp), C.byref(ab), None) == H.ERR_ARGUMENT  # and ambient occlusion
assert np.all(lit == 9) and np.all(flags == 9) and np.all(occ == 9)
ms = C.c_double(-1.0)
assert lib.pt_direct_finish(r.context, C.byref(ms)) == H.OK and ms.value > 0.0
assert lib.pt_direct_finish(r.context, None) == H.ERR_ARGUMENT and lib.pt_rays_finish(r.context, None) == H.ERR_ARGUMENT  # nothing in flight any more
stream.synchronize()
assert t_sum.cpu().numpy().tobytes() == ref["sum"].tobytes()
assert t_lit.cpu().numpy().view(np.uint32).tobytes() == ref["lit"].tobytes() and t_valid.cpu().numpy().tobytes() == ref["valid"].tobytes()
# an ao pass open refuses a direct pass in turn
d_occ = torch.zeros((n,), dtype=torch.int32, device=dev)
dab = H.PtAoBuffers(occluded=ptr(d_occ, H._up))
assert lib.pt_ao_device(r.context, C.byref(ap), C.c_void_p(d_P.data_ptr()), C.c_void_p(d_N.data_ptr()), C.byref(dab), C.c_void_p(stream.cuda_stream)) == H.OK
assert lib.pt_direct_device(*args) == H.ERR_ARGUMENT
assert lib.pt_ao_finish(r.context, None) == H.OK
assert lib.pt_rays(r.context, C.byref(rp), P.ctypes.data_as(H._dp), N.ctypes.data_as(H._dp), C.byref(rb), None) == H.OK  # the pass is free again
r.close()
assert (x * 2).sum().item() == 2048.0
print("direct into torch tensors ok")
""" % (root, root)
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "direct into torch tensors ok" in done.stdout, done.stdout[-2000:] + done.stderr[-4000:]


def test_a_render_on_each_slot_and_an_aov_pass_in_flight_around_a_direct_pass(H, host):
    """pt_render_device on both slots and a pt_aov_device pass in flight, then pt_direct_device on a stream: every result equals what the same calls give one
    after the other on a second context."""
    import device_glue
    from example_scenes import EXAMPLES
    w, h, samples = 160, 96, 2
    bg = default_background(w, h)
    scene, cam0, _ = EXAMPLES["big-scene"]()
    c = case(host, H, "big-scene", "flat")
    P, N, n = c["P"], c["N"], NPTS
    lib = H.lib()
    camera = device_glue.camera_struct(cam0, w, h)
    results = []
    for overlapped in (False, True):
        ds = device_glue.DeviceScene(scene, H.TRAVERSE_FLAT)
        ctx = H.Context()
        ds.upload(ctx)
        cx = ctx.handle

        def dev(arr=None, nbytes=0):
            ptr = C.c_void_p()
            assert lib.pt_device_alloc(cx, arr.nbytes if arr is not None else nbytes, C.byref(ptr)) == 0
            if arr is not None:
                assert lib.pt_copy_to_device(cx, ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes) == 0
            return ptr
        d_bg, d_P, d_N = dev(bg), dev(P), dev(N)
        d_img, d_img2, d_depth, d_lit, d_sum = dev(nbytes=w * h * 3), dev(nbytes=w * h * 3), dev(nbytes=w * h * 8), dev(nbytes=n * 4), dev(nbytes=n * 24)
        st = H.PtStats()
        ap = H.PtAovParams(w, h, H.PtRect(0, 0, w - 1, h - 1), (C.c_double * 2)(0.5, 0.5))
        ab = H.PtAovBuffers(depth=C.cast(d_depth, H._dp))
        op = H.PtDirectParams(n, 1, 0, SEED, 0, 0.0, H.AO_FACE_EYE, (C.c_double * 3)(*c["eye"]))
        ob = H.PtDirectBuffers(sum=C.cast(d_sum, H._dp), lit=C.cast(d_lit, H._up))

        def render(k, img):
            rp = H.PtRenderParams(w, h, H.PtRect(0, 0, w - 1, h - 1), samples, 10 + k, H.SAMPLE_RNG, 1, 0, 1, 0)
            return lib.pt_render_device(cx, C.byref(camera), d_bg, C.byref(rp), 0, img, C.c_void_p(lib.pt_context_stream(cx, k)))
        direct = lambda: lib.pt_direct_device(cx, C.byref(op), d_P, d_N, C.byref(ob), C.c_void_p(lib.pt_context_stream(cx, 0)))
        if overlapped:
            assert render(0, d_img) == 0 and render(1, d_img2) == 0 and lib.pt_aov_device(cx, C.byref(camera), C.byref(ap), C.byref(ab), None) == 0, lib.pt_last_error(cx)
            assert direct() == 0, lib.pt_last_error(cx)
            assert direct() == H.ERR_ARGUMENT
            assert lib.pt_direct_finish(cx, None) == 0, lib.pt_last_error(cx)
            assert lib.pt_render_finish(cx, C.byref(st)) == 0 and lib.pt_render_finish(cx, C.byref(st)) == 0 and lib.pt_aov_finish(cx, None) == 0, lib.pt_last_error(cx)
        else:
            for k, img in ((0, d_img), (1, d_img2)):
                assert render(k, img) == 0 and lib.pt_render_finish(cx, C.byref(st)) == 0, lib.pt_last_error(cx)
            assert lib.pt_aov_device(cx, C.byref(camera), C.byref(ap), C.byref(ab), None) == 0 and lib.pt_aov_finish(cx, None) == 0, lib.pt_last_error(cx)
            assert direct() == 0 and lib.pt_direct_finish(cx, None) == 0, lib.pt_last_error(cx)
        out = {}
        for name, ptr, arr in (("img", d_img, np.zeros((h, w, 3), dtype=np.uint8)), ("img2", d_img2, np.zeros((h, w, 3), dtype=np.uint8)), ("depth", d_depth, np.zeros((h, w))),
                               ("lit", d_lit, np.zeros(n, dtype=np.uint32)), ("sum", d_sum, np.zeros((n, 3)))):
            assert lib.pt_copy_from_device(cx, arr.ctypes.data_as(C.c_void_p), ptr, arr.nbytes) == 0
            out[name] = arr
        for ptr in (d_bg, d_P, d_N, d_img, d_img2, d_depth, d_lit, d_sum):
            lib.pt_device_free(cx, ptr)
        ctx.close()
        results.append(out)
    for k in results[0]:
        assert results[0][k].tobytes() == results[1][k].tobytes(), k
    got = results[1]
    ref = case_reference(c, 1)
    assert got["img"].any() and got["img2"].any() and np.isfinite(got["depth"]).any()
    assert np.array_equal(got["lit"], ref[1]) and np.array_equal(bits(got["sum"]), bits(ref[0]))


# ---- 8. refusals on a context
def test_argument_errors_with_a_context(host, H):
    lib = H.lib()
    c = case(host, H, "soft-shadows", "flat")
    ctx = c["r"].context
    n = 100
    P, N = np.zeros((n, 3)), np.ones((n, 3))
    lit, total = np.full(n, 3, dtype=np.uint32), np.full((n, 3), 3.0)
    dp = lambda a: a.ctypes.data_as(H._dp)
    ob = H.PtDirectBuffers(sum=dp(total), lit=lit.ctypes.data_as(H._up))
    ok = dict(n=n, samples=16, pass_index=0, seed=0, first_index=0, bias=0.0, flags=0)
    good = H.PtDirectParams(**ok)
    bad_eye = H.PtDirectParams(**dict(ok, flags=H.AO_FACE_EYE))
    bad_eye.eye[0] = float("nan")
    for fn in (lib.pt_direct, lib.pt_direct_device):
        assert fn(ctx, None, dp(P), dp(N), C.byref(ob), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), None, dp(N), C.byref(ob), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(P), None, C.byref(ob), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(P), dp(N), None, None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(P), dp(N), C.byref(H.PtDirectBuffers()), None) == H.ERR_ARGUMENT
        for change in (dict(n=H.AO_MAX + 1), dict(samples=0), dict(samples=3), dict(samples=48), dict(samples=128), dict(bias=-1e-300), dict(bias=float("inf")),
                       dict(bias=float("nan")), dict(flags=4), dict(flags=0x80000001)):
            assert fn(ctx, C.byref(H.PtDirectParams(**dict(ok, **change))), dp(P), dp(N), C.byref(ob), None) == H.ERR_ARGUMENT, change
            assert lib.pt_last_error(ctx).startswith(b"pt_direct:"), change
        assert fn(ctx, C.byref(bad_eye), dp(P), dp(N), C.byref(ob), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(H.PtDirectParams(**dict(ok, n=0))), dp(P), dp(N), C.byref(ob), None) == H.OK  # n = 0: no launch, nothing written, nothing in flight
    assert lib.pt_direct_device(ctx, C.byref(good), dp(P), dp(N), C.byref(ob), None) == H.ERR_ARGUMENT, "host memory is no device pointer"
    assert np.all(lit == 3) and np.all(total == 3.0)
    assert lib.pt_direct_finish(ctx, None) == H.ERR_ARGUMENT  # nothing in flight
    nan_eye_unused = H.PtDirectParams(**ok)
    nan_eye_unused.eye[1] = float("nan")  # the eye is read with PT_AO_FACE_EYE only
    assert lib.pt_direct(ctx, C.byref(nan_eye_unused), dp(P), dp(N), C.byref(ob), None) == H.OK
    bare = H.Context()
    assert lib.pt_direct(bare.handle, C.byref(good), dp(P), dp(N), C.byref(ob), None) == H.ERR_NO_SCENE
    assert lib.pt_direct_device(bare.handle, C.byref(good), dp(P), dp(N), C.byref(ob), None) == H.ERR_NO_SCENE
    bare.close()
