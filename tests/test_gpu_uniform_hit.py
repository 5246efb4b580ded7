"""The surface of a hit from records fetched once per wavefront and node (pt_render_simple.h: the loop over the distinct nodes of the
shaded lanes, pt_shade.h: pt_hit_surface_uniform_flat) instead of per lane. The same functions on the same operands in the same order, so
every image must stay what the oracle computes, bit for bit - in both semantics (the hierarchical kernel keeps the per-lane form; it is
rendered here so that a change of its form meets the same cases), with the occluder table and without it:

 * a cloud of primitives smaller than a pixel at 64 samples: the samples of one pixel hit one, two and many distinct nodes;
 * one sample per pixel: a wavefront is 64 pixels, many nodes per wavefront;
 * stand-alone triangles among the analytic primitives: the per-lane fallback mixed with the uniform form in one wavefront;
 * the scene's highest-numbered node covering the frame: the last record of every array;
 * big-scene; and one frame with the counting instantiation, whose counters must stay the oracle's."""
import numpy as np
import pytest

import host_glue
from scene_dsl import Camera, Cone, Cube, Cylinder, Light, Material, Node, Plane, Scene, Sphere, Triangle, default_background
from test_gpu_shadow_cache import shadowed_scene
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


def mats(rng, n=5):
    return [Material(diffuse=tuple(rng.uniform(0.1, 1, 3)), specular=tuple(rng.uniform(0, 0.9, 3)) if i % 3 else (0, 0, 0), shininess=float(rng.choice([1.0, 25.0, 300.0])))
            for i in range(n)]


def lights():
    return [Light(position=(3.0, 8.0, 6.0), color=(0.7, 0.7, 0.7)), Light(position=(-5.0, 6.0, 4.0), color=(0.3, 0.3, 0.4), falloff=(1.0, 0.01, 0.001)),
            Light(position=(0.0, 2.0, 9.0), color=(0.3, 0.2, 0.2))]


def dust_scene(triangles: bool, last_covers: bool = False):
    """A few hundred primitives much smaller than a pixel of a 16 x 16 frame would be useless (nothing hits them): sizes from a tenth of a pixel to a few pixels,
    in nested, scaled and rotated groups in front of a wall, so that the 64 samples of a pixel land on one node (the wall, a larger primitive), on two (an edge)
    and on many (the dust). triangles: every fourth primitive is a stand-alone triangle. last_covers: the wall is the LAST node of the scene."""
    rng = np.random.default_rng(77 if triangles else 76)
    m = mats(rng)
    prims = [Sphere, Cube, Cylinder, Cone]
    pixel = 2.0 * 6.0 * np.tan(np.radians(25.0)) / 16.0  # the frame's pixel at the cloud's distance (camera at z = 6, fovy 50)

    def leaf(k):
        if triangles and k % 4 == 3:
            v = rng.uniform(-1, 1, (3, 3))
            p = Triangle(v[0], v[1], v[2], normals=rng.uniform(-1, 1, (3, 3)) if k % 8 == 3 else None)
        else:
            p = prims[k % 4]()
        n = Node.geo(p, m[int(rng.integers(0, len(m)))])
        n.scaled(tuple(pixel * np.exp(rng.uniform(np.log(0.1), np.log(3.0), 3))))
        n.rotated_xzy(tuple(rng.uniform(-3.1, 3.1, 3)))
        n.translated(tuple(rng.uniform(-2.6, 2.6, 2)) + (float(rng.uniform(-0.5, 0.5)),))
        return n

    groups = []
    for g in range(6):
        kids = [leaf(8 * g + k) for k in range(40)]
        inner = Node.group([leaf(100 + 8 * g + k) for k in range(12)]).scaled((0.8, 1.1, 0.9)).rotated_y(0.3 * g).translated((0.1 * g, -0.1, 0.0))
        grp = Node.group(kids + [inner])
        if g % 2:
            grp.scaled((1.05, 0.95, 1.0)).rotated_z(0.2 * g).translated((0.0, 0.05 * g, 0.0))
        groups.append(grp)
    wall = Node.geo(Cube(), m[0]).scaled((40.0, 40.0, 1.0)).translated((0.0, 0.0, -2.0))
    kids = groups + [wall] if last_covers else [wall] + groups
    return Scene(root=Node.group(kids), lights=lights(), ambient=(0.1, 0.1, 0.1)), Camera(eye=(0.0, 0.0, 6.0), center=(0.0, 0.0, 0.0), fovy_degrees=50.0)


def check(host, H, oracle, monkeypatch, scene, cam, w, h, samples, seed, mode, stats=False):
    tr, om = traversal(H, oracle, mode)
    ref = oracle.render(scene, cam, w, h, samples=samples, seed=seed, jitter=oracle.JITTER_RNG, mode=om)
    r = host.Renderer(host_glue.host_scene(scene), tr)
    bg = default_background(w, h)
    try:
        for cache in (None, "0"):
            if cache is None:
                monkeypatch.delenv("PORTRAYER_SHADOW_CACHE", raising=False)
            else:
                monkeypatch.setenv("PORTRAYER_SHADOW_CACHE", cache)
            rgb, lin, st = r.render(host_glue.cam10(cam), w, h, bg, samples=samples, seed=seed, sample_mode=H.SAMPLE_RNG)
            assert st["kernel_mode"] == (6 if mode == "hier" else 3) and not st["kernel_variant"] & (H.KERNEL_CHAIN | H.KERNEL_INTERPRETER)
            assert np.array_equal(rgb, ref.rgb), f"cache {cache}: {(rgb != ref.rgb).any(axis=2).sum()} pixels differ"
            assert_ulp(lin, ref.linear, 0)
        monkeypatch.delenv("PORTRAYER_SHADOW_CACHE", raising=False)
        if stats:
            rgb, lin, st = r.render(host_glue.cam10(cam), w, h, bg, samples=samples, seed=seed, sample_mode=H.SAMPLE_RNG, stats=True)
            assert np.array_equal(rgb, ref.rgb)
            assert_ulp(lin, ref.linear, 0)
            for k in ("primary", "shadow", "hits", "reflect"):
                assert st[k] == ref.stats[k], (k, st[k], ref.stats[k])
    finally:
        r.close()
    return ref


@pytest.mark.parametrize("mode", SEMANTICS)
def test_dust_smaller_than_a_pixel(host, H, oracle, monkeypatch, mode):
    """16 x 16 x 64: a wavefront is the 64 samples of one pixel; they hit one node, two, many."""
    scene, cam = dust_scene(triangles=False)
    check(host, H, oracle, monkeypatch, scene, cam, 16, 16, 64, 5, mode, stats=(mode == "flat"))


@pytest.mark.parametrize("mode", SEMANTICS)
def test_many_nodes_per_wavefront(host, H, oracle, monkeypatch, mode):
    """48 x 32 x 1: a wavefront is an 8 x 8 tile of pixels."""
    scene, cam = shadowed_scene(True, True)
    check(host, H, oracle, monkeypatch, scene, cam, 48, 32, 1, 7, mode)
    scene, cam = dust_scene(triangles=False)
    check(host, H, oracle, monkeypatch, scene, cam, 48, 32, 1, 8, mode)


@pytest.mark.parametrize("mode", SEMANTICS)
@pytest.mark.parametrize("size,samples", [((16, 16), 64), ((48, 32), 1)])
def test_triangles_among_the_analytic_hits(host, H, oracle, monkeypatch, mode, size, samples):
    """Stand-alone triangles take the per-lane form - in the same wavefront as lanes that take the uniform one."""
    scene, cam = dust_scene(triangles=True)
    check(host, H, oracle, monkeypatch, scene, cam, size[0], size[1], samples, 9, mode)


@pytest.mark.parametrize("mode", SEMANTICS)
def test_the_last_node_covers_the_frame(host, H, oracle, monkeypatch, mode):
    """The wall behind the dust is the scene's highest-numbered node: most pixels read the last record of info, inv, fwd and nrm."""
    scene, cam = dust_scene(triangles=False, last_covers=True)
    hs = host_glue.host_scene(scene)
    ex = hs.export()
    assert int(ex["prim_type"][-1]) == 5  # (pt_prims.h PT_CUBE) the wall closes the node arrays
    ref = check(host, H, oracle, monkeypatch, scene, cam, 16, 16, 64, 11, mode)
    assert ref.stats["hits"] > 0.9 * 16 * 16 * 64


@pytest.mark.parametrize("mode", SEMANTICS)
def test_big_scene(host, H, oracle, monkeypatch, mode):
    from example_scenes import EXAMPLES
    from scene_dsl import ASSETS
    sc = host.Scene.example("big-scene", assets=ASSETS)
    tr, om = traversal(H, oracle, mode)
    w, h = 160, 90
    ref = oracle.render(oracle.pack_arrays(sc.export()), EXAMPLES["big-scene"]()[1], w, h, samples=64, seed=3, jitter=oracle.JITTER_RNG, mode=om)
    r = host.Renderer(sc, tr)
    try:
        for cache in (None, "0"):
            if cache is None:
                monkeypatch.delenv("PORTRAYER_SHADOW_CACHE", raising=False)
            else:
                monkeypatch.setenv("PORTRAYER_SHADOW_CACHE", cache)
            rgb, lin, st = r.render(sc.camera, w, h, default_background(w, h), samples=64, seed=3, sample_mode=H.SAMPLE_RNG)
            assert st["kernel_mode"] == (6 if mode == "hier" else 3)
            assert np.array_equal(rgb, ref.rgb), f"cache {cache}: {(rgb != ref.rgb).any(axis=2).sum()} pixels differ"
            assert_ulp(lin, ref.linear, 0)
    finally:
        monkeypatch.delenv("PORTRAYER_SHADOW_CACHE", raising=False)
        r.close()
