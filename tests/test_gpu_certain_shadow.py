"""Shadow rays settled in f32 before the light's f64 set-up (pt_certain.h, pt_render_simple.h: CERTAIN): where the inscribed ball of the tile's cached
occluder says every shaded lane's ray certainly ends in that node, the light is skipped without direction, probe or walk. The answer is the one the exact test
gives, so every image and every f64 mean must equal the oracle's, and equal the render without the occluder table (PORTRAYER_SHADOW_CACHE=0, which takes no
part in any of this). Each scene is rendered with the table zeroed, as in every product render, and with hints the test chooses (PORTRAYER_OCC_SEED): every
node K of a small scene as every entry, four hashed seeds on big-scene - so every node's ball is tried against rays it does not block.

Flat_scene semantics: the hierarchical one has no certain-shadow table (no composed forward record is resident for it)."""
import numpy as np
import pytest

import host_glue
from scene_dsl import Camera, Cone, Cube, Cylinder, Light, Material, Node, Plane, Scene, Sphere, default_background
from ulp import assert_ulp

pytestmark = pytest.mark.gpu

PRIMS = {"sphere": Sphere, "cube": Cube, "cylinder": Cylinder, "cone": Cone}
FLOOR = Material(diffuse=(0.7, 0.7, 0.6), specular=(0.2, 0.2, 0.2), shininess=10.0)
RED = Material(diffuse=(0.8, 0.2, 0.2), specular=(0.5, 0.5, 0.5), shininess=40.0)
BLUE = Material(diffuse=(0.2, 0.3, 0.8), specular=(0.4, 0.4, 0.4), shininess=25.0)


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def render(monkeypatch, r, cam, w, h, samples, seed, H, occ_seed=None, cache=True):
    monkeypatch.delenv("PORTRAYER_SHADOW_CACHE", raising=False)
    monkeypatch.delenv("PORTRAYER_OCC_SEED", raising=False)
    if not cache:
        monkeypatch.setenv("PORTRAYER_SHADOW_CACHE", "0")
    if occ_seed is not None:
        monkeypatch.setenv("PORTRAYER_OCC_SEED", str(occ_seed))
    try:
        return r.render(cam, w, h, default_background(w, h), samples=samples, seed=seed, sample_mode=H.SAMPLE_RNG)
    finally:
        monkeypatch.delenv("PORTRAYER_SHADOW_CACHE", raising=False)
        monkeypatch.delenv("PORTRAYER_OCC_SEED", raising=False)


def check(monkeypatch, H, r, cam, ref, w, h, samples, seed, occ_seeds):
    """Table zeroed, table off, and every hint of occ_seeds: all equal to the oracle's image and f64 means."""
    rgb0, lin0, st = render(monkeypatch, r, cam, w, h, samples, seed, H, cache=False)
    assert st["kernel_mode"] == 3 and not st["kernel_variant"] & (H.KERNEL_CHAIN | H.KERNEL_INTERPRETER)
    assert np.array_equal(rgb0, ref.rgb), f"table off: {(rgb0 != ref.rgb).any(axis=2).sum()} pixels differ from the oracle"
    assert_ulp(lin0, ref.linear, 0, "table off")
    for occ in [None, *occ_seeds]:
        rgb, lin, _ = render(monkeypatch, r, cam, w, h, samples, seed, H, occ_seed=occ)
        assert np.array_equal(rgb, ref.rgb), f"hint {occ}: {(rgb != ref.rgb).any(axis=2).sum()} pixels differ from the oracle"
        assert_ulp(lin, ref.linear, 0, f"hint {occ}")
        assert np.array_equal(rgb, rgb0)
        assert_ulp(lin, lin0, 0, f"hint {occ} against the render without the table")


def nodes_with_a_ball(hs, H):
    """Per flattened node whether the host build of the table routine gives it a ball: a ray from model-space (3, 0, 0) through the node's centre to (-3, 0, 0)
    is certain exactly then (pt_test_certain_shadow). The kernel has no counter outside the counting build, so this is what shows that a scene exercises the
    skip at all - or, for the scenes built for that, that it cannot."""
    import ctypes as C
    f = hs.flatten()
    n = len(f["prim_type"])
    out = np.zeros(n, dtype=bool)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    for k in range(n):
        fwd = np.ascontiguousarray(f["trans"][k, :3, :].reshape(12))
        inv = np.ascontiguousarray(f["invtrans"][k, :3, :].reshape(12))
        a, c = f["trans"][k, :3, :3], f["trans"][k, :3, 3]
        P = np.ascontiguousarray(c + a @ np.array([3.0, 0.0, 0.0]))
        L = np.ascontiguousarray(c - a @ np.array([3.0, 0.0, 0.0]))
        certain, exact = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        if int(f["prim_type"][k]) < 0:
            continue
        assert H.lib().pt_test_certain_shadow(1, int(f["prim_type"][k]), fwd.ctypes.data_as(dp), inv.ctypes.data_as(dp), P.ctypes.data_as(dp), L.ctypes.data_as(dp),
                                              certain.ctypes.data_as(ip), exact.ctypes.data_as(ip)) == 0
        out[k] = bool(certain[0])
    return out


def n_nodes(hs):
    return int((hs.export()["prim_type"] >= 0).sum())


def check_small(monkeypatch, host, H, oracle, scene, cam, balls, w=48, h=32, samples=64, seed=7):
    """balls: whether some node of the scene must have a ball (the skip can fire) or none may."""
    hs = host_glue.host_scene(scene)
    assert nodes_with_a_ball(hs, H).any() == balls
    r = host.Renderer(hs, H.TRAVERSE_FLAT)
    ref = oracle.render(scene, cam, w, h, samples=samples, seed=seed, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
    assert ref.stats["shadow"] > 0
    check(monkeypatch, H, r, host_glue.cam10(cam), ref, w, h, samples, seed, [f"all:{k}" for k in range(n_nodes(hs))])
    r.close()


@pytest.mark.parametrize("size,samples", [((160, 90), 64), ((96, 64), 2)])
def test_big_scene(host, H, oracle, monkeypatch, size, samples):
    """The benchmark's scene: a wavefront is one pixel (64 samples) or 32 pixels (2)."""
    from example_scenes import EXAMPLES
    from scene_dsl import ASSETS
    sc = host.Scene.example("big-scene", assets=ASSETS)
    w, h = size
    assert nodes_with_a_ball(sc, H).sum() > 300  # (the spheres and the cubes, half of 1000 nodes)
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    ref = oracle.render(oracle.pack_arrays(sc.export()), EXAMPLES["big-scene"]()[1], w, h, samples=samples, seed=3, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
    check(monkeypatch, H, r, sc.camera, ref, w, h, samples, 3, [5, 1009, 90210, 20261019])
    r.close()


def shadowed_scene(area: bool, occluders: bool):
    """A floor under a few spheres and boxes (or under nothing), two point lights and one area light (or three point lights)."""
    kids = [Node.geo(Plane(), FLOOR).scaled(30.0)]
    if occluders:
        kids += [Node.geo(Sphere(), RED).scaled(0.8).translated((x, 1.0, z)) for x in (-2.0, 0.0, 2.0) for z in (-2.0, 1.0)]
        kids.append(Node.group([Node.geo(Cube(), RED).scaled((0.5, 2.0, 0.5)).rotated_y(0.4).translated((1.0, 0.0, 3.0))]).translated((0.0, 0.2, 0.0)))
    lights = [Light(position=(3.0, 8.0, 4.0), color=(0.6, 0.6, 0.6)),
              Light(position=(-5.0, 6.0, -1.0), color=(0.3, 0.3, 0.4), falloff=(1.0, 0.01, 0.001),
                    area_a=(1.5, 0.0, 0.0) if area else (0.0, 0.0, 0.0), area_b=(0.0, 0.0, 1.5) if area else (0.0, 0.0, 0.0)),
              Light(position=(0.0, 12.0, -6.0), color=(0.3, 0.2, 0.2))]
    return Scene(root=Node.group(kids), lights=lights, ambient=(0.1, 0.1, 0.1)), Camera(eye=(0.0, 6.0, 12.0), center=(0.0, 0.0, 0.0), fovy_degrees=45.0)


@pytest.mark.parametrize("area,occluders", [(True, True), (False, True), (False, False)])
def test_shadowed_scenes(host, H, oracle, monkeypatch, area, occluders):
    scene, cam = shadowed_scene(area, occluders)
    check_small(monkeypatch, host, H, oracle, scene, cam, balls=occluders)


@pytest.mark.parametrize("kind", list(PRIMS))
def test_a_light_inside_the_primitive(host, H, oracle, monkeypatch, kind):
    """One light sits inside the solid (every ray toward it ends in the solid, from outside and from the solid's own surface), one outside; a second
    solid of the same type stands between the floor and the outer light. Sphere and cube have a ball; cylinder and cone have none and take the exact path."""
    kids = [Node.geo(Plane(), FLOOR).scaled(30.0),
            Node.geo(PRIMS[kind](), RED).scaled(2.0).rotated_xzy((0.3, 0.5, 0.2)).translated((-1.0, 1.5, 0.0)),
            Node.geo(PRIMS[kind](), BLUE).scaled(1.2).rotated_z(0.4).translated((2.5, 1.0, 1.0))]
    lights = [Light(position=(-1.0, 1.4, 0.05), color=(0.8, 0.8, 0.8)),
              Light(position=(6.0, 7.0, 5.0), color=(0.5, 0.5, 0.4))]
    cam = Camera(eye=(1.0, 5.0, 10.0), center=(0.0, 1.0, 0.0), fovy_degrees=45.0)
    check_small(monkeypatch, host, H, oracle, Scene(root=Node.group(kids), lights=lights, ambient=(0.1, 0.1, 0.1)), cam, balls=kind in ("sphere", "cube"))


def test_primitives_too_small_for_a_ball(host, H, oracle, monkeypatch):
    """World radii of 0.001 .. 0.002: below the 2^-10 the table keeps between the ball and the surface, so no node has a ball and every ray takes the exact path."""
    kids = [Node.geo(Plane(), FLOOR).scaled(0.2)]
    for i, kind in enumerate(PRIMS):
        kids.append(Node.geo(PRIMS[kind](), RED if i % 2 else BLUE).scaled(0.002 if kind == "sphere" else 0.004).translated((0.006 * (i - 1.5), 0.003, 0.002 * (i % 2))))
    lights = [Light(position=(0.02, 0.05, 0.03), color=(0.8, 0.8, 0.8)), Light(position=(-0.03, 0.04, -0.01), color=(0.4, 0.4, 0.5))]
    cam = Camera(eye=(0.0, 0.02, 0.04), center=(0.0, 0.002, 0.0), fovy_degrees=40.0)
    check_small(monkeypatch, host, H, oracle, Scene(root=Node.group(kids), lights=lights, ambient=(0.1, 0.1, 0.1)), cam, balls=False)


def test_non_uniform_scale_and_shear(host, H, oracle, monkeypatch):
    """Every type stretched, rotated and stretched again by its group (a sheared composite): the ball's radius comes from the bound on the smallest singular value."""
    inner = []
    for i, kind in enumerate(PRIMS):
        inner.append(Node.geo(PRIMS[kind](), RED if i % 2 else BLUE).scaled((1.6, 0.7, 1.1)).rotated_xzy((0.4 + 0.3 * i, 0.2 * i, 0.7)).translated((-3.0 + 2.0 * i, 1.2, 0.5 * (i % 2))))
    kids = [Node.geo(Plane(), FLOOR).scaled(30.0), Node.group(inner).scaled((1.3, 0.8, 1.0)).rotated_y(0.3)]
    lights = [Light(position=(3.0, 8.0, 4.0), color=(0.6, 0.6, 0.6)), Light(position=(-6.0, 5.0, 2.0), color=(0.4, 0.4, 0.5)),
              Light(position=(0.0, 9.0, -6.0), color=(0.3, 0.2, 0.2), area_a=(1.0, 0.0, 0.0), area_b=(0.0, 0.0, 1.0))]
    cam = Camera(eye=(0.0, 5.0, 11.0), center=(0.0, 0.5, 0.0), fovy_degrees=45.0)
    check_small(monkeypatch, host, H, oracle, Scene(root=Node.group(kids), lights=lights, ambient=(0.1, 0.1, 0.1)), cam, balls=True)
