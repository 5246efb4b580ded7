"""The occluder table of the mesh-free walks' shadow rays (pt_trace.h: pt_trace_packet): a shadow ray tests the node that
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
