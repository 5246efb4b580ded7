"""What a render launch has, as the planner says it (pt_plan_launch, csrc/pt_api.hip; pt_test_launch_plan) and as the launch shows it: small frames of five scenes - mesh-free
with 2 lights and with 33, one opaque mirror, one dielectric, one small mesh - in the crate's three traversal semantics, counting and plain, under the switches the
planner reads. Every image and every f64 mean equals the oracle's bit for bit (one oracle render per scene, mode and sample count); the kernel pt_stats reports, the
records pt_test_pixel_list_summary finds, the queue pt_test_pixel_list_queue finds and the lights pt_test_dark_lights has records for are what the plan of the same
inputs holds; and a malformed switch value fails with its pinned words in front of anything that is reserved or queued."""
import ctypes as C

import numpy as np
import pytest

import host_glue
from scene_dsl import Camera, Cone, Cube, Cylinder, Light, Material, Mesh, Node, Scene, Sphere, default_background
from test_kernel_choice import _grid_mesh
from test_launch_plan import plan_of, work_shape
from ulp import assert_ulp

pytestmark = pytest.mark.gpu

W = HGT = 16
ONE_PIXEL, SEVERAL_PIXELS = 64, 16  # samples: K C = 64, a wavefront is one pixel (tests/test_gpu_pixel_lists.py); K C = 16, four pixels
KD_DEPTH = 6
KEYS = ("PORTRAYER_SHADOW_CACHE", "PORTRAYER_DARK_LIGHTS", "PORTRAYER_PIXEL_LISTS", "PORTRAYER_BACKGROUND_SKIP", "PORTRAYER_PIXEL_LIST_CAP", "PORTRAYER_PIXEL_LIST_PENDING",
        "PORTRAYER_FINE_QUEUES", "PORTRAYER_BATCH_MAX", "PORTRAYER_OCC_SEED", "PORTRAYER_ITEM_STRIDE", "PORTRAYER_NO_TEX", "PORTRAYER_WAVES", "PORTRAYER_KD_WAVES",
        "PORTRAYER_CHAIN", "PORTRAYER_CHAIN_WAVES", "PORTRAYER_PARK", "PORTRAYER_FORK", "PORTRAYER_LDS_BUDGET_KB")
SWITCHES = ["", "PORTRAYER_SHADOW_CACHE=0", "PORTRAYER_DARK_LIGHTS=0", "PORTRAYER_PIXEL_LISTS=0", "PORTRAYER_BACKGROUND_SKIP=0", "PORTRAYER_PIXEL_LIST_CAP=0",
            "PORTRAYER_PIXEL_LIST_PENDING=1", "PORTRAYER_FINE_QUEUES=0", "PORTRAYER_BATCH_MAX=1", "PORTRAYER_OCC_SEED=7", "PORTRAYER_OCC_SEED=all:0"]
SCENES = ("two lights", "33 lights", "mirror", "dielectric", "mesh")
CAMERA = Camera(eye=(0.7, 1.9, 7.5), center=(0.0, 0.2, 0.0))


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def set_switches(monkeypatch, switch):
    for k in KEYS:
        monkeypatch.delenv(k, raising=False)
    for kv in switch.split():
        k, v = kv.split("=")
        monkeypatch.setenv(k, v)


def build_scene(name):
    """-> (DSL scene, the traits pt_scene_upload derives from it, without the traversal)"""
    n_lights = 33 if name == "33 lights" else 2
    mats = [Material(diffuse=(0.8, 0.3, 0.2), specular=(0.5, 0.5, 0.5), shininess=25.0), Material(diffuse=(0.2, 0.7, 0.3), specular=(0.0, 0.0, 0.0)),
            Material(diffuse=(0.3, 0.4, 0.8), specular=(0.6, 0.6, 0.3), shininess=300.0)]
    if name == "mirror":
        mats[1].reflectivity = 0.8
    if name == "dielectric":
        mats[1].reflectivity = 0.9; mats[1].refraction_index = 1.5
    kids = [Node.geo(p(), mats[k % 3]).scaled((0.9 + 0.2 * k, 1.2 - 0.1 * k, 0.8 + 0.15 * k)).rotated_xzy((0.4 + 0.5 * k, -0.7 + 0.3 * k, 1.1 - 0.6 * k))
            .translated((-2.4 + 1.2 * k, 0.4 * (k % 2) - 0.3, -0.5 * k)) for k, p in enumerate((Sphere, Cube, Cylinder, Cone, Sphere))]
    if name == "mesh":
        kids.append(Node.geo(Mesh(_grid_mesh(12)), mats[0]).scaled(2.0).rotated_xzy((0.3, 0.2, 0.1)).translated((0.3, 1.4, 0.5)))
    lights = [Light(position=(6.0 * np.cos(2.4 * k), 5.0 + (k % 3), 6.0 * np.sin(2.4 * k) + 3.0), color=(1.2 / n_lights,) * 3) for k in range(n_lights)]
    mesh = name == "mesh"
    traits = dict(n_nodes=len(kids), n_lights=n_lights, has_meshes=int(mesh), has_kdmesh=0, instanced_tris=12 if mesh else 0, reflective=int(name in ("mirror", "dielectric")),
                  reflective_opaque=int(name != "dielectric"), glossy=0, area_light=0)
    return Scene(root=Node.group(kids), lights=lights, ambient=(0.1, 0.1, 0.1)), traits


@pytest.fixture(scope="module")
def cases(host, H, oracle):
    """(scene, mode) -> (renderer, traits, {samples: the oracle's render}); every renderer lives for the module."""
    out = {}
    for name in SCENES:
        scene, traits = build_scene(name)
        hs = host_glue.host_scene(scene)
        assert int((hs.export()["prim_type"] >= 0).sum()) == traits["n_nodes"]
        for mode, tr, om in (("flat", H.TRAVERSE_FLAT, oracle.MODE_FLAT), ("kd", H.TRAVERSE_KD, oracle.MODE_KD), ("hier", H.TRAVERSE_HIER, oracle.MODE_HIER)):
            refs = {s: oracle.render(scene, CAMERA, W, HGT, samples=s, seed=11, jitter=oracle.JITTER_RNG, mode=om, kd_depth=KD_DEPTH) for s in (ONE_PIXEL, SEVERAL_PIXELS)}
            out[(name, mode)] = (host.Renderer(hs, tr, kd_depth=KD_DEPTH), dict(traits, traverse=tr), refs)
    yield out
    for r, _, _ in out.values():
        r.close()


def observed(H, r):
    """What the hooks find of the renderer's last launch: the records, whether it had a queue, the lights it had dark-light records for."""
    lib, c = H.lib(), r.context
    summary, queue, dark = (C.c_uint64 * 32)(), (C.c_uint64 * 3)(), (C.c_uint64 * 2)()
    assert lib.pt_test_pixel_list_summary(c, summary) == 0, lib.pt_last_error(c)
    assert lib.pt_test_pixel_list_queue(c, None, 0, queue) == 0, lib.pt_last_error(c)
    assert lib.pt_test_dark_lights(c, None, 0, dark) == 0, lib.pt_last_error(c)
    return int(summary[0]), int(queue[0]), int(dark[0])


def check_launches(H, cases, samples, where):
    shape = work_shape(W, HGT, samples)
    bg = default_background(W, HGT)
    seen = set()
    for (name, mode), (r, traits, refs) in cases.items():
        ref = refs[samples]
        for counting in (True, False):
            rgb, linear, st = r.render(host_glue.cam10(CAMERA), W, HGT, bg, samples=samples, seed=11, sample_mode=H.SAMPLE_RNG, stats=counting)
            tag = f"{where}: {name} / {mode} / {'counting' if counting else 'plain'} (kernel mode {st['kernel_mode']}, variant {st['kernel_variant']})"
            assert np.array_equal(rgb, ref.rgb), tag
            assert_ulp(linear, ref.linear, 0, tag)
            if counting:
                for k in ("primary", "shadow", "reflect", "refract", "hits"):
                    assert st[k] == ref.stats[k], (tag, k)
            plan = plan_of(H, traits, stats=counting, **shape)
            has = plan[H.PLAN_HAS]
            assert (st["kernel_mode"], st["kernel_variant"]) == (plan[H.PLAN_KERNEL_MODE], plan[H.PLAN_KERNEL_VARIANT]) and bool(st["kernel_variant"] & H.KERNEL_COUNTING) == counting, tag
            records, queue, dark = observed(H, r)
            assert records == (shape["n_slots"] if has & H.PLAN_HAS_PIXEL_LISTS else 0), tag
            assert queue == (1 if has & H.PLAN_HAS_QUEUE else 0), tag
            assert dark == (traits["n_lights"] if has & H.PLAN_HAS_DARK_RECORDS else 0), tag
            seen.add((mode, bool(has & H.PLAN_HAS_PIXEL_LISTS), bool(has & H.PLAN_HAS_QUEUE), bool(has & H.PLAN_HAS_DARK_RECORDS)))
    return seen


@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: s or "default")
def test_a_launch_has_what_its_plan_says(H, cases, monkeypatch, switch):
    set_switches(monkeypatch, switch)
    seen = check_launches(H, cases, ONE_PIXEL, switch or "default")
    if switch == "":  # the default launches between them have everything, and lack it
        assert ("flat", True, True, True) in seen and ("flat", False, False, True) in seen and ("kd", False, False, False) in seen, seen


def test_several_pixels_per_wavefront(H, cases, monkeypatch):
    set_switches(monkeypatch, "")
    seen = check_launches(H, cases, SEVERAL_PIXELS, "several pixels per wavefront")
    assert not any(lists or queue for (_, lists, queue, _) in seen), seen


@pytest.mark.parametrize("switch,words", [("PORTRAYER_OCC_SEED=12x", "PORTRAYER_OCC_SEED=12x: expected all:<node> or a decimal seed"),
                                          ("PORTRAYER_OCC_SEED=all:5", "PORTRAYER_OCC_SEED=all:5: K must be a node index below 5"),
                                          ("PORTRAYER_PIXEL_LIST_CAP=7", "PORTRAYER_PIXEL_LIST_CAP=7: expected 0 .. 6"),
                                          ("PORTRAYER_PIXEL_LIST_PENDING=0", "PORTRAYER_PIXEL_LIST_PENDING=0: expected 1 .. 1024")])
def test_a_malformed_switch_fails_in_front_of_the_launch(H, cases, monkeypatch, switch, words):
    r, traits, refs = cases[("two lights", "flat")]
    lib, c = H.lib(), r.context
    bg = default_background(W, HGT)
    kw = dict(samples=ONE_PIXEL, seed=11, sample_mode=H.SAMPLE_RNG)
    set_switches(monkeypatch, switch)
    with pytest.raises(Exception) as e:
        r.render(host_glue.cam10(CAMERA), W, HGT, bg, **kw)
    assert words in str(e.value), str(e.value)
    assert lib.pt_last_error(c).decode() == words
    assert lib.pt_render_finish(c, None) == H.ERR_ARGUMENT and lib.pt_last_error(c).decode() == "no render in flight"  # nothing was queued
    assert plan_of(H, traits, stats=False, expect=H.ERR_ARGUMENT, **work_shape(W, HGT, ONE_PIXEL)) == words
    set_switches(monkeypatch, "")
    rgb, linear, _ = r.render(host_glue.cam10(CAMERA), W, HGT, bg, **kw)
    assert np.array_equal(rgb, refs[ONE_PIXEL].rgb)
    assert_ulp(linear, refs[ONE_PIXEL].linear, 0)
