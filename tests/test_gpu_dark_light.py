"""A point light enclosed in a sphere or a cube is dark everywhere, and the launch settles that once per light (pt_certain.h 4.-8., pt_dark_light_kernel,
pt_render_simple.h): the straight-line kernels skip such a light wherever the lane guard lets every shaded lane through. The answer is the one the
exact path gives, so every image and every f64 mean must equal the oracle's and equal the render of the same library with PORTRAYER_DARK_LIGHTS=0 (no light is
flagged: the code as it was). Each scene is rendered with the occluder table zeroed and with hints the test chooses (PORTRAYER_OCC_SEED hashed and all:K).

The launch's per-light records are read back (pt_test_dark_lights) and compared with the host replay of the table routines over every flattened node
(pt_test_dark_light): the same lights flagged, through the same - the lowest - node; and each case says which lights its scene was built to have flagged."""
import ctypes as C

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
WHITE = (0.7, 0.7, 0.7)
CAM = Camera(eye=(1.0, 5.0, 10.0), center=(0.0, 1.0, 0.0), fovy_degrees=45.0)


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def render(monkeypatch, r, cam, w, h, samples, seed, H, occ_seed=None, dark=True):
    monkeypatch.delenv("PORTRAYER_DARK_LIGHTS", raising=False)
    monkeypatch.delenv("PORTRAYER_OCC_SEED", raising=False)
    if not dark:
        monkeypatch.setenv("PORTRAYER_DARK_LIGHTS", "0")
    if occ_seed is not None:
        monkeypatch.setenv("PORTRAYER_OCC_SEED", str(occ_seed))
    try:
        return r.render(cam, w, h, default_background(w, h), samples=samples, seed=seed, sample_mode=H.SAMPLE_RNG)
    finally:
        monkeypatch.delenv("PORTRAYER_DARK_LIGHTS", raising=False)
        monkeypatch.delenv("PORTRAYER_OCC_SEED", raising=False)


def records(H, r):
    """The last launch's dark-light records, (lights, 8) uint32; None where that launch had none."""
    info = (C.c_uint64 * 2)()
    assert H.lib().pt_test_dark_lights(r.context, None, 0, info) == 0
    if info[0] == 0:
        return None
    out = np.zeros((int(info[0]), int(info[1])), dtype=np.uint32)
    assert H.lib().pt_test_dark_lights(r.context, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, info) == 0
    return out


def replay(H, hs, lights):
    """Per light the lowest flattened node whose ball the host build of the table routines finds it enclosed in, + 1 (0: none)."""
    f = hs.flatten()
    keep = np.flatnonzero(f["prim_type"] >= 0)
    n = len(keep)
    fwd = np.ascontiguousarray(f["trans"][keep, :3, :].reshape(n, 12))
    inv = np.ascontiguousarray(f["invtrans"][keep, :3, :].reshape(n, 12))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    out = []
    for l in lights:
        L = np.ascontiguousarray(np.tile(np.array(l.position, dtype=np.float64), (n, 1)))
        area = np.ascontiguousarray(np.tile(np.array([*l.area_a, *l.area_b], dtype=np.float64), (n, 1)))
        P = np.ascontiguousarray(L + 1.0)
        flagged = np.zeros(n, dtype=np.int32)
        for typ in np.unique(f["prim_type"][keep]):
            m = np.flatnonzero(f["prim_type"][keep] == typ)
            fl, g, e = (np.zeros(len(m), dtype=np.int32) for _ in range(3))
            a = (np.ascontiguousarray(x[m]) for x in (fwd, inv, P, L, area))
            assert H.lib().pt_test_dark_light(len(m), int(typ), *(x.ctypes.data_as(dp) for x in a), fl.ctypes.data_as(ip), g.ctypes.data_as(ip), e.ctypes.data_as(ip)) == 0
            flagged[m] = fl
        hit = np.flatnonzero(flagged)
        out.append(int(keep[hit[0]]) + 1 if hit.size else 0)
    return out


def n_nodes(hs):
    return int((hs.export()["prim_type"] >= 0).sum())


def check_records(H, r, hs, lights, dark):
    rec = records(H, r)
    assert rec is not None and rec.shape == (len(lights), 8)
    nodes = [int(x) for x in rec[:, 4]]
    assert [x != 0 for x in nodes] == [bool(d) for d in dark], f"flagged through nodes {nodes}, the scene was built for {dark}"
    assert nodes == replay(H, hs, lights)
    for k, l in enumerate(lights):
        if nodes[k]:
            assert np.array_equal(rec[k, :3].view(np.float32), np.array(l.position, dtype=np.float32)) and rec[k, 3:4].view(np.float32)[0] > 0.0
            assert rec[k, 5:6].view(np.float32)[0] == np.float32(1e-30)
        else:
            assert not rec[k].any()


def check(monkeypatch, host, H, oracle, scene, cam, dark, w=48, h=32, samples=64, seed=7, all_hints=True):
    """dark: per light whether the scene was built to have it flagged. Flags off, table zeroed, a hashed table and every all:K: all equal to the oracle."""
    hs = host_glue.host_scene(scene)
    r = host.Renderer(hs, H.TRAVERSE_FLAT)
    ref = oracle.render(scene, cam, w, h, samples=samples, seed=seed, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
    assert ref.stats["shadow"] > 0
    c10 = host_glue.cam10(cam)
    rgb0, lin0, st = render(monkeypatch, r, c10, w, h, samples, seed, H, dark=False)
    assert st["kernel_mode"] == 3 and not st["kernel_variant"] & (H.KERNEL_CHAIN | H.KERNEL_INTERPRETER)
    rec = records(H, r)
    assert rec is not None and not rec.any(), "PORTRAYER_DARK_LIGHTS=0 flags nothing"
    assert np.array_equal(rgb0, ref.rgb), f"flags off: {(rgb0 != ref.rgb).any(axis=2).sum()} pixels differ from the oracle"
    assert_ulp(lin0, ref.linear, 0, "flags off")
    hints = [None, 20261021] + ([f"all:{k}" for k in range(n_nodes(hs))] if all_hints else ["all:0", f"all:{n_nodes(hs) - 1}"])
    for occ in hints:
        rgb, lin, _ = render(monkeypatch, r, c10, w, h, samples, seed, H, occ_seed=occ)
        if occ is None:
            check_records(H, r, hs, scene.lights, dark)
        assert np.array_equal(rgb, ref.rgb), f"hint {occ}: {(rgb != ref.rgb).any(axis=2).sum()} pixels differ from the oracle"
        assert_ulp(lin, ref.linear, 0, f"hint {occ}")
        assert np.array_equal(rgb, rgb0)
        assert_ulp(lin, lin0, 0, f"hint {occ} against the render with no light flagged")
    r.close()


def enclosure(kind):
    """The solid the light sits in: the sphere scaled, the others rotated and scaled as well."""
    n = Node.geo(PRIMS[kind](), RED).scaled(2.0 if kind == "sphere" else (2.0, 2.6, 2.2))
    return (n if kind == "sphere" else n.rotated_xzy((0.3, 0.5, 0.2))).translated((-1.0, 1.5, 0.0))


def around():
    return [Node.geo(Plane(), FLOOR).scaled(30.0),
            Node.geo(Sphere(), BLUE).scaled(0.8).translated((2.5, 0.8, 1.0)),
            Node.geo(Cube(), BLUE).scaled(1.2).rotated_y(0.4).translated((-3.5, 0.6, 2.0))]


OUTER = Light(position=(6.0, 7.0, 5.0), color=(0.5, 0.5, 0.4))


@pytest.mark.parametrize("kind,samples", [("sphere", 64), ("sphere", 2), ("sphere", 16), ("cube", 64), ("cube", 2), ("cube", 16), ("cylinder", 64), ("cone", 64)])
def test_a_light_inside_a_solid(host, H, oracle, monkeypatch, kind, samples):
    """Matte objects around a solid with a light in it and a light outside. Sphere and cube: flagged. Cylinder and cone have no ball: not flagged, the exact path.
    64 samples: a wavefront is one pixel; 2 and 16: it is not."""
    scene = Scene(root=Node.group(around() + [enclosure(kind)]), lights=[Light(position=(-1.0, 1.4, 0.05), color=WHITE), OUTER], ambient=(0.1, 0.1, 0.1))
    check(monkeypatch, host, H, oracle, scene, CAM, [kind in ("sphere", "cube"), False], samples=samples, all_hints=samples == 64)


@pytest.mark.parametrize("side", ["inside", "outside"])
def test_a_hair_inside_and_outside_the_margin(host, H, oracle, monkeypatch, side):
    """A sphere of radius 2 at c: the table's rho = 2 (1 - 2^-5) - 2^-10 - 2^-20 |c| up to 2^-19, and a light is flagged up to (1 - 2^-6) rho from c. The light 1e-4
    of that inside: flagged; 1e-4 outside (still deep inside the sphere): not flagged, and the image is the same."""
    c = np.array([-1.0, 1.5, 0.0])
    rho = 2.0 * (1.0 - 2.0 ** -5) - 2.0 ** -10 - 2.0 ** -20 * np.linalg.norm(c)
    d = (1.0 - 2.0 ** -6) * rho * (1.0 - 1e-4 if side == "inside" else 1.0 + 1e-4)
    u = np.array([0.6, 0.0, 0.8])
    scene = Scene(root=Node.group(around() + [enclosure("sphere")]), lights=[Light(position=tuple(c + d * u), color=WHITE), OUTER], ambient=(0.1, 0.1, 0.1))
    check(monkeypatch, host, H, oracle, scene, CAM, [side == "inside", False], all_hints=False)


def test_a_second_solid_cuts_the_enclosing_one(host, H, oracle, monkeypatch):
    """A cube pushed into the enclosing sphere: part of its surface - shaded points - lies inside the sphere, some of it between the light and the sphere's surface."""
    kids = around() + [enclosure("sphere"), Node.geo(Cube(), BLUE).scaled(1.6).rotated_y(0.3).translated((0.6, 1.2, 1.2))]
    scene = Scene(root=Node.group(kids), lights=[Light(position=(-1.0, 1.4, 0.05), color=WHITE), OUTER], ambient=(0.1, 0.1, 0.1))
    check(monkeypatch, host, H, oracle, scene, CAM, [True, False])


def test_the_camera_inside_the_enclosing_sphere(host, H, oracle, monkeypatch):
    """Every shaded point is the sphere's inner surface or an object inside it; the light is inside too, and the ray toward it still leaves the sphere behind it."""
    kids = [Node.geo(Sphere(), RED).scaled(6.0).translated((0.0, 1.0, 0.0)), Node.geo(Cube(), BLUE).scaled(1.0).rotated_y(0.5).translated((1.0, 0.5, -2.0)),
            Node.geo(Sphere(), BLUE).scaled(0.6).translated((-1.5, 0.0, -1.0))]
    scene = Scene(root=Node.group(kids), lights=[Light(position=(0.5, 3.0, 1.0), color=WHITE), Light(position=(0.0, 20.0, 30.0), color=(0.5, 0.5, 0.4))], ambient=(0.1, 0.1, 0.1))
    cam = Camera(eye=(0.0, 1.0, 3.5), center=(0.0, 0.5, -2.0), fovy_degrees=60.0)
    check(monkeypatch, host, H, oracle, scene, cam, [True, False])


def test_the_middle_one_of_three_lights(host, H, oracle, monkeypatch):
    lights = [Light(position=(3.0, 8.0, 4.0), color=(0.6, 0.6, 0.6)), Light(position=(-1.0, 1.4, 0.05), color=WHITE), Light(position=(-5.0, 6.0, -1.0), color=(0.3, 0.3, 0.4), falloff=(1.0, 0.01, 0.001))]
    scene = Scene(root=Node.group(around() + [enclosure("cube")]), lights=lights, ambient=(0.1, 0.1, 0.1))
    check(monkeypatch, host, H, oracle, scene, CAM, [False, True, False])


def test_an_area_light_inside_a_solid_is_not_flagged(host, H, oracle, monkeypatch):
    lights = [Light(position=(-1.0, 1.4, 0.05), color=WHITE, area_a=(0.2, 0.0, 0.0), area_b=(0.0, 0.0, 0.2)), OUTER]
    scene = Scene(root=Node.group(around() + [enclosure("sphere")]), lights=lights, ambient=(0.1, 0.1, 0.1))
    check(monkeypatch, host, H, oracle, scene, CAM, [False, False], all_hints=False)


def test_dark_lights_at_the_ends_of_66(host, H, oracle, monkeypatch):
    """Lights 0, 63, 64 and 65 of 66 inside the cube, the others on a ring above the scene."""
    inside = [(-1.0, 1.4, 0.05), (-0.9, 1.3, 0.1), (-1.1, 1.6, -0.1), (-1.0, 1.25, 0.15)]
    lights = []
    for k in range(66):
        if k in (0, 63, 64, 65):
            lights.append(Light(position=inside[len([x for x in (0, 63, 64, 65) if x < k])], color=WHITE))
        else:
            a = 2.0 * np.pi * k / 66.0
            lights.append(Light(position=(8.0 * np.cos(a), 6.0 + 0.05 * k, 8.0 * np.sin(a)), color=(0.03, 0.03, 0.03)))
    scene = Scene(root=Node.group(around() + [enclosure("cube")]), lights=lights, ambient=(0.1, 0.1, 0.1))
    check(monkeypatch, host, H, oracle, scene, CAM, [k in (0, 63, 64, 65) for k in range(66)], w=32, h=24, all_hints=False)


def test_the_flag_follows_a_scene_update(host, H, oracle, monkeypatch):
    """One context: the light inside the sphere, moved out of it by pt_scene_update, and moved back. The records are the launch's own."""
    def scene_with(pos):
        return Scene(root=Node.group(around() + [enclosure("sphere")]), lights=[Light(position=pos, color=WHITE), OUTER], ambient=(0.1, 0.1, 0.1))
    inside, outside = (-1.0, 1.4, 0.05), (-1.0, 6.0, 0.05)
    w, h, samples, seed = 48, 32, 64, 11
    c10 = host_glue.cam10(CAM)
    refs = {p: oracle.render(scene_with(p), CAM, w, h, samples=samples, seed=seed, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT) for p in (inside, outside)}
    assert not np.array_equal(refs[inside].rgb, refs[outside].rgb)
    hs = host_glue.host_scene(scene_with(inside))
    r = host.Renderer(hs, H.TRAVERSE_FLAT)
    for step, pos in enumerate((inside, outside, inside, outside, inside)):
        if step:
            hs = host_glue.host_scene(scene_with(pos))
            r.update(hs)
        rgb, lin, _ = render(monkeypatch, r, c10, w, h, samples, seed, H)
        check_records(H, r, hs, scene_with(pos).lights, [pos == inside, False])
        assert np.array_equal(rgb, refs[pos].rgb), f"step {step}"
        assert_ulp(lin, refs[pos].linear, 0, f"step {step}")
    r.close()


def test_big_scene(host, H, oracle, monkeypatch):
    """The benchmark's scene: its third light lies inside flattened node 956, a cube, and is flagged through it; the other two lie inside nothing."""
    from example_scenes import EXAMPLES
    from scene_dsl import ASSETS
    sc = host.Scene.example("big-scene", assets=ASSETS)
    w, h, samples, seed = 160, 90, 64, 3
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    ref = oracle.render(oracle.pack_arrays(sc.export()), EXAMPLES["big-scene"]()[1], w, h, samples=samples, seed=seed, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
    rgb0, lin0, _ = render(monkeypatch, r, sc.camera, w, h, samples, seed, H, dark=False)
    assert np.array_equal(rgb0, ref.rgb)
    assert_ulp(lin0, ref.linear, 0, "flags off")
    for occ in (None, 5, 20261021):
        rgb, lin, _ = render(monkeypatch, r, sc.camera, w, h, samples, seed, H, occ_seed=occ)
        if occ is None:
            rec = records(H, r)
            assert [int(x) for x in rec[:, 4]] == [0, 0, 957]
        assert np.array_equal(rgb, ref.rgb), f"hint {occ}: {(rgb != ref.rgb).any(axis=2).sum()} pixels differ from the oracle"
        assert_ulp(lin, ref.linear, 0, f"hint {occ}")
        assert_ulp(lin, lin0, 0, f"hint {occ} against the render with no light flagged")
    r.close()
