"""The occluder table of the mesh-free walks' shadow rays (pt_walk_wave.h: pt_trace_packet): a shadow ray tests the node that
last blocked a ray of its tile toward the same light before it walks the tree. Its answer is an OR over nodes, so the images must not
change: the plain instantiations with the table (the default) and without it (PORTRAYER_SHADOW_CACHE=0) against each other at the
benchmark's size, and against the oracle at small sizes - big-scene, area lights (a light position per lane) and a scene in which
nothing is ever in the way."""
import numpy as np
import pytest

import host_glue
from scene_dsl import Camera, Cube, Light, Material, Node, Plane, Scene, Sphere, default_background
from ulp import assert_ulp

pytestmark = pytest.mark.gpu

SEMANTICS = ["flat", "hier"]


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def traversal(H, oracle, mode):
    return (H.TRAVERSE_HIER, oracle.MODE_HIER) if mode == "hier" else (H.TRAVERSE_FLAT, oracle.MODE_FLAT)


def render_both(monkeypatch, r, cam, w, h, samples, seed, H):
    """The plain instantiation with the table and without it: (rgb, linear, stats) twice."""
    bg = default_background(w, h)
    kw = dict(samples=samples, seed=seed, sample_mode=H.SAMPLE_RNG)
    monkeypatch.delenv("PORTRAYER_SHADOW_CACHE", raising=False)
    on = r.render(cam, w, h, bg, **kw)
    monkeypatch.setenv("PORTRAYER_SHADOW_CACHE", "0")
    off = r.render(cam, w, h, bg, **kw)
    monkeypatch.delenv("PORTRAYER_SHADOW_CACHE")
    return on, off


@pytest.mark.parametrize("mode", SEMANTICS)
def test_headline_size_with_and_without_the_table(host, H, oracle, monkeypatch, mode):
    """bench.py's frame (big-scene, 1920x1080, 64 samples) in the instantiations it times: identical images and f64 means."""
    from scene_dsl import ASSETS
    sc = host.Scene.example("big-scene", assets=ASSETS)
    tr, _ = traversal(H, oracle, mode)
    r = host.Renderer(sc, tr)
    (rgb, lin, st), (rgb0, lin0, st0) = render_both(monkeypatch, r, sc.camera, 1920, 1080, 64, 0, H)
    r.close()
    assert st["kernel_mode"] == (6 if mode == "hier" else 3) and st["kernel_variant"] == st0["kernel_variant"] == 6
    assert np.array_equal(rgb, rgb0), f"{(rgb != rgb0).any(axis=2).sum()} pixels differ"
    assert_ulp(lin, lin0, 0)


@pytest.mark.parametrize("mode", SEMANTICS)
@pytest.mark.parametrize("size,samples", [((800, 600), 1), ((160, 90), 64)])
def test_big_scene_against_the_oracle(host, H, oracle, monkeypatch, mode, size, samples):
    """C2's size with one sample (a wavefront = 64 pixels) and a small frame with 64 (a wavefront = one pixel), both settings."""
    from example_scenes import EXAMPLES
    from scene_dsl import ASSETS
    sc = host.Scene.example("big-scene", assets=ASSETS)
    w, h = size
    tr, om = traversal(H, oracle, mode)
    r = host.Renderer(sc, tr)
    on, off = render_both(monkeypatch, r, sc.camera, w, h, samples, 3, H)
    r.close()
    ref = oracle.render(oracle.pack_arrays(sc.export()), EXAMPLES["big-scene"]()[1], w, h, samples=samples, seed=3, jitter=oracle.JITTER_RNG, mode=om)
    for rgb, lin, _ in (on, off):
        assert np.array_equal(rgb, ref.rgb), f"{(rgb != ref.rgb).any(axis=2).sum()} pixels differ"
        assert_ulp(lin, ref.linear, 0)


def shadowed_scene(area: bool, occluders: bool):
    """A floor under a few spheres and boxes (or under nothing), two point lights and one area light (or three point lights)."""
    floor = Material(diffuse=(0.7, 0.7, 0.6), specular=(0.2, 0.2, 0.2), shininess=10.0)
    red = Material(diffuse=(0.8, 0.2, 0.2), specular=(0.5, 0.5, 0.5), shininess=40.0)
    kids = [Node.geo(Plane(), floor).scaled(30.0)]
    if occluders:
        kids += [Node.geo(Sphere(), red).scaled(0.8).translated((x, 1.0, z)) for x in (-2.0, 0.0, 2.0) for z in (-2.0, 1.0)]
        kids.append(Node.group([Node.geo(Cube(), red).scaled((0.5, 2.0, 0.5)).rotated_y(0.4).translated((1.0, 0.0, 3.0))]).translated((0.0, 0.2, 0.0)))
    lights = [Light(position=(3.0, 8.0, 4.0), color=(0.6, 0.6, 0.6)),
              Light(position=(-5.0, 6.0, -1.0), color=(0.3, 0.3, 0.4), falloff=(1.0, 0.01, 0.001),
                    area_a=(1.5, 0.0, 0.0) if area else (0.0, 0.0, 0.0), area_b=(0.0, 0.0, 1.5) if area else (0.0, 0.0, 0.0)),
              Light(position=(0.0, 12.0, -6.0), color=(0.3, 0.2, 0.2))]
    return Scene(root=Node.group(kids), lights=lights, ambient=(0.1, 0.1, 0.1)), Camera(eye=(0.0, 6.0, 12.0), center=(0.0, 0.0, 0.0), fovy_degrees=45.0)


@pytest.mark.parametrize("mode", SEMANTICS)
@pytest.mark.parametrize("area,occluders", [(True, True), (False, True), (False, False)])
@pytest.mark.parametrize("samples", [64, 2])
def test_shadowed_scenes_against_the_oracle(host, H, oracle, monkeypatch, mode, area, occluders, samples):
    scene, cam = shadowed_scene(area, occluders)
    w, h = (48, 32) if samples == 64 else (160, 96)
    tr, om = traversal(H, oracle, mode)
    r = host.Renderer(host_glue.host_scene(scene), tr)
    on, off = render_both(monkeypatch, r, host_glue.cam10(cam), w, h, samples, 7, H)
    _, _, st = r.render(host_glue.cam10(cam), w, h, default_background(w, h), samples=samples, seed=7, sample_mode=H.SAMPLE_RNG, stats=True)
    r.close()
    assert on[2]["kernel_mode"] == (6 if mode == "hier" else 3)
    ref = oracle.render(scene, cam, w, h, samples=samples, seed=7, jitter=oracle.JITTER_RNG, mode=om)
    assert st["shadow"] == ref.stats["shadow"] > 0
    for rgb, lin, _ in (on, off):
        assert np.array_equal(rgb, ref.rgb), f"{(rgb != ref.rgb).any(axis=2).sum()} pixels differ"
        assert_ulp(lin, ref.linear, 0)


# ---------------------------------------------------------------------------------------------------
# Hints the test chooses (PORTRAYER_OCC_SEED, pt_plan_launch): the table's test must give the same image whatever an entry holds -
# the surface being shaded, a node behind the shading point, a node under a transformed or shared group, a node the walk's f32 box
# test would have culled, none. Only the plain instantiations read the table: seeded renders are compared as plain images and f64 means.
# ---------------------------------------------------------------------------------------------------
def render_seeded(monkeypatch, r, cam, w, h, samples, seed, H, occ_seed, **kw):
    """The plain instantiation with the table seeded by PORTRAYER_OCC_SEED=occ_seed (None: zeroed, as in every product render)."""
    monkeypatch.delenv("PORTRAYER_SHADOW_CACHE", raising=False)
    if occ_seed is None:
        monkeypatch.delenv("PORTRAYER_OCC_SEED", raising=False)
    else:
        monkeypatch.setenv("PORTRAYER_OCC_SEED", str(occ_seed))
    try:
        return r.render(cam, w, h, default_background(w, h), samples=samples, seed=seed, sample_mode=H.SAMPLE_RNG, **kw)
    finally:
        monkeypatch.delenv("PORTRAYER_OCC_SEED", raising=False)


def n_nodes(hs):
    """The nodes the device walks - the scene's primitives (its groups are not among them): what an entry may name (the hook refuses the
    next index, test_the_seed_is_applied_and_checked)."""
    return int((hs.export()["prim_type"] >= 0).sum())


def assert_same(rgb, lin, want_rgb, want_lin, where):
    assert np.array_equal(rgb, want_rgb), f"{where}: {(rgb != want_rgb).any(axis=2).sum()} pixels differ"
    assert_ulp(lin, want_lin, 0, str(where))


def test_the_seed_is_applied_and_checked(host, H, monkeypatch, capfd):
    """PORTRAYER_VERBOSE=1 reports how many entries were seeded (one per 8x8 tile and light); a hint that is not a node is refused."""
    scene, cam = shadowed_scene(True, True)
    hs = host_glue.host_scene(scene)
    r = host.Renderer(hs, H.TRAVERSE_FLAT)
    monkeypatch.setenv("PORTRAYER_VERBOSE", "1")
    capfd.readouterr()
    render_seeded(monkeypatch, r, host_glue.cam10(cam), 48, 32, 1, 7, H, "all:1")
    lines = [l for l in capfd.readouterr().err.splitlines() if "occluder table" in l]
    assert lines == ["[pt_render] occluder table: 72 entries seeded (PORTRAYER_OCC_SEED=all:1)"], lines  # 6 x 4 tiles x 3 lights
    render_seeded(monkeypatch, r, host_glue.cam10(cam), 48, 32, 1, 7, H, None)
    assert "occluder table" not in capfd.readouterr().err
    render_seeded(monkeypatch, r, host_glue.cam10(cam), 48, 32, 1, 7, H, f"all:{n_nodes(hs) - 1}")
    for bad in (f"all:{n_nodes(hs)}", "all:", "all:x", "12x"):
        with pytest.raises(Exception, match="PORTRAYER_OCC_SEED"):
            render_seeded(monkeypatch, r, host_glue.cam10(cam), 48, 32, 1, 7, H, bad)
    r.close()


@pytest.mark.parametrize("mode", SEMANTICS)
@pytest.mark.parametrize("area,occluders", [(True, True), (False, True), (False, False)])
def test_every_node_as_every_hint(host, H, oracle, monkeypatch, mode, area, occluders):
    """Every entry = node K, for every K: 48 x 32 x 1 (each wavefront is one tile and reads the seeded entry for every light) and 16 x 16 x 64."""
    scene, cam = shadowed_scene(area, occluders)
    hs = host_glue.host_scene(scene)
    tr, om = traversal(H, oracle, mode)
    r = host.Renderer(hs, tr)
    for (w, h), samples in (((48, 32), 1), ((16, 16), 64)):
        ref = oracle.render(scene, cam, w, h, samples=samples, seed=7, jitter=oracle.JITTER_RNG, mode=om)
        for k in range(n_nodes(hs)):
            rgb, lin, st = render_seeded(monkeypatch, r, host_glue.cam10(cam), w, h, samples, 7, H, f"all:{k}")
            assert st["kernel_mode"] == (6 if mode == "hier" else 3)
            assert_same(rgb, lin, ref.rgb, ref.linear, (mode, w, h, samples, k))
    r.close()


@pytest.mark.parametrize("mode", SEMANTICS)
@pytest.mark.parametrize("seed", range(4))
def test_hashed_hints_in_analytic_scenes(host, H, oracle, monkeypatch, mode, seed):
    """Nested, transformed and shared groups; touching, thin and tiny primitives; the camera now and then inside the cloud."""
    from test_gpu_render_parity import analytic_scene
    scene, cam = analytic_scene(seed)
    tr, om = traversal(H, oracle, mode)
    r = host.Renderer(host_glue.host_scene(scene), tr)
    w, h = 101, 67
    for samples in (1, 2):
        ref = oracle.render(scene, cam, w, h, samples=samples, seed=seed, jitter=oracle.JITTER_RNG, mode=om)
        for occ in (11, 90210 + seed):
            rgb, lin, _ = render_seeded(monkeypatch, r, host_glue.cam10(cam), w, h, samples, seed, H, occ)
            assert_same(rgb, lin, ref.rgb, ref.linear, (seed, samples, occ))
    r.close()


@pytest.mark.parametrize("mode", SEMANTICS)
@pytest.mark.parametrize("seed", range(6))
def test_hashed_hints_in_extreme_scenes(host, H, oracle, monkeypatch, mode, seed):
    """Coincident, touching, thin and huge primitives - with the mirror material's reflectivity set to 0, so that the plain straight-line
    kernel (the one that reads the table) renders them rather than the chain kernel."""
    from fuzz_gpu_parity import extreme_scene
    scene, cam = extreme_scene(seed)
    for node in scene.root.children:
        if node.geometry is not None:
            node.geometry[1].reflectivity = 0.0
    tr, om = traversal(H, oracle, mode)
    r = host.Renderer(host_glue.host_scene(scene), tr)
    w, h = 128, 96
    ref = oracle.render(scene, cam, w, h, samples=2, seed=seed, jitter=oracle.JITTER_RNG, mode=om)
    rgb, lin, st = render_seeded(monkeypatch, r, host_glue.cam10(cam), w, h, 2, seed, H, 4242 + seed)
    assert st["kernel_mode"] == (6 if mode == "hier" else 3) and not st["kernel_variant"] & (H.KERNEL_CHAIN | H.KERNEL_INTERPRETER)
    assert_same(rgb, lin, ref.rgb, ref.linear, (seed, mode))
    r.close()


@pytest.mark.parametrize("mode", SEMANTICS)
def test_hashed_hints_in_big_scene(host, H, oracle, monkeypatch, mode):
    from example_scenes import EXAMPLES
    from scene_dsl import ASSETS
    sc = host.Scene.example("big-scene", assets=ASSETS)
    tr, om = traversal(H, oracle, mode)
    r = host.Renderer(sc, tr)
    ref = oracle.render(oracle.pack_arrays(sc.export()), EXAMPLES["big-scene"]()[1], 160, 90, samples=1, seed=3, jitter=oracle.JITTER_RNG, mode=om)
    for occ in (1, 77):
        rgb, lin, _ = render_seeded(monkeypatch, r, sc.camera, 160, 90, 1, 3, H, occ)
        assert_same(rgb, lin, ref.rgb, ref.linear, (mode, occ))
    r.close()


@pytest.mark.parametrize("mode", SEMANTICS)
def test_hashed_hints_in_a_partition(host, H, oracle, monkeypatch, mode):
    """tile_ranks = 3 with a slice that does not start at 0 (each rank's table rows: occ_row, the fallback entry `back`): the three ranks'
    plain renders assembled == the single launch == the oracle."""
    from example_scenes import EXAMPLES
    from scene_dsl import ASSETS
    from test_gpu_multirank import render_partition
    sc = host.Scene.example("big-scene", assets=ASSETS)
    tr, om = traversal(H, oracle, mode)
    r = host.Renderer(sc, tr)
    w, h, rect, samples = 157, 93, (11, 5, 149, 90), 2
    bg = default_background(w, h)
    monkeypatch.setenv("PORTRAYER_OCC_SEED", "31337")
    img, _ = render_partition(H, host, r, sc, w, h, rect, 3, samples, bg, stats=False)
    one, _, st = r.render(sc.camera, w, h, bg, samples=samples, seed=3, sample_mode=H.SAMPLE_RNG, rect=rect, into=np.full((h, w, 3), 7, dtype=np.uint8))
    monkeypatch.delenv("PORTRAYER_OCC_SEED")
    r.close()
    assert st["kernel_mode"] == (6 if mode == "hier" else 3)
    assert np.array_equal(img, one), f"{(img != one).any(axis=2).sum()} pixels differ"
    ref = oracle.render(oracle.pack_arrays(sc.export()), EXAMPLES["big-scene"]()[1], w, h, samples=samples, seed=3, jitter=oracle.JITTER_RNG, mode=om, rect=rect)
    x0, y0, x1, y1 = rect
    inside = (slice(y0, y1 + 1), slice(x0, x1 + 1))
    assert np.array_equal(one[inside], ref.rgb[inside]), f"{(one[inside] != ref.rgb[inside]).any(axis=2).sum()} pixels differ"
    outside = np.ones((h, w), dtype=bool); outside[inside] = False
    assert (img[outside] == 7).all()


@pytest.mark.parametrize("mode", SEMANTICS)
def test_hashed_hints_at_65_lights(host, H, oracle, monkeypatch, mode):
    """The 65-light big-scene of test_gpu_lights (entries at tile * 65 + light, the fallback 65 x occ_row words back)."""
    from test_gpu_lights import lit_scene
    scene, cam = lit_scene(65, "big")
    tr, om = traversal(H, oracle, mode)
    r = host.Renderer(host_glue.host_scene(scene), tr)
    w, h = 61, 45
    ref = oracle.render(scene, cam, w, h, samples=1, seed=4, jitter=oracle.JITTER_RNG, mode=om)
    rgb, lin, st = render_seeded(monkeypatch, r, host_glue.cam10(cam), w, h, 1, 4, H, 65065)
    r.close()
    assert st["kernel_mode"] == (6 if mode == "hier" else 3)
    assert_same(rgb, lin, ref.rgb, ref.linear, mode)


@pytest.mark.parametrize("mode", SEMANTICS)
def test_headline_size_seeded_and_unseeded(host, H, monkeypatch, mode):
    """bench.py's frame (big-scene, 1920x1080, 64 samples): hashed hints change neither the image nor the f64 means."""
    from scene_dsl import ASSETS
    sc = host.Scene.example("big-scene", assets=ASSETS)
    r = host.Renderer(sc, H.TRAVERSE_HIER if mode == "hier" else H.TRAVERSE_FLAT)
    rgb0, lin0, _ = render_seeded(monkeypatch, r, sc.camera, 1920, 1080, 64, 0, H, None)
    rgb, lin, _ = render_seeded(monkeypatch, r, sc.camera, 1920, 1080, 64, 0, H, 2024)
    r.close()
    assert_same(rgb, lin, rgb0, lin0, mode)
