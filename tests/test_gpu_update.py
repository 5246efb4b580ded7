"""pt_scene_update / Renderer.update on the GPU: a renderer created on scene A and then moved to scene B answers exactly as a fresh Renderer on B and as the
oracle's render of B - u8 image, f64 linear means and the six ray counters - in all three traversals, with the scene-level tree rebuilt on the host and on
the device (PORTRAYER_BUILD, read at call time). Every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_glue  # noqa: E402
from example_scenes import big_scene, fish, macho_cows, normal_mapping, transmission_refraction, water_glass  # noqa: E402
from scene_dsl import Camera, Cube, Light, Material, Node, Scene, Sphere, default_background  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ["flat", "kd", "hier"]
BUILDERS = ["host", "device"]
COUNTERS = ("primary", "shadow", "reflect", "refract", "hits", "depth11_skipped")
W, HT = 96, 54
KW = dict(samples=2, seed=5)


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def traverse(H, oracle, mode):
    return {"flat": (H.TRAVERSE_FLAT, oracle.MODE_FLAT), "kd": (H.TRAVERSE_KD, oracle.MODE_KD), "hier": (H.TRAVERSE_HIER, oracle.MODE_HIER)}[mode]


def geometry_nodes(node, out=None):
    out = [] if out is None else out
    if node.geometry is not None:
        out.append(node)
    for c in node.children:
        geometry_nodes(c, out)
    return out


def moved(builder, oracle):
    """Scene B of a builder's scene A: its first child rotated, one object scaled non-uniformly, its last child carried 1e3 units away - out of A's
    root box - and the camera aimed at where that went."""
    scene, cam, _ = builder()
    before = oracle.flatten(oracle.pack(scene))["trans"][:, :3, 3].copy()
    kids = scene.root.children
    kids[0].rotated_y(0.6)
    geos = geometry_nodes(scene.root)
    geos[len(geos) // 2].scaled((1.3, 0.7, 1.1))
    kids[-1].translated((1e3, 0.0, 0.0))
    after = oracle.flatten(oracle.pack(scene))["trans"][:, :3, 3]
    far = int(np.argmax(np.linalg.norm(after - before, axis=1)))
    assert np.linalg.norm(after[far] - before[far]) > 900.0
    view = np.array(cam.eye, dtype=np.float64) - np.array(cam.center, dtype=np.float64)
    view *= min(1.0, 30.0 / np.linalg.norm(view))
    return scene, Camera(eye=tuple(after[far] + view), center=tuple(after[far]), up=cam.up, fovy_degrees=cam.fovy_degrees)


def spheres_and_cubes(n, place):
    red = Material(diffuse=(0.8, 0.2, 0.2), specular=(0.5, 0.5, 0.5), shininess=40.0)
    blue = Material(diffuse=(0.2, 0.3, 0.8), specular=(0.3, 0.3, 0.3), shininess=25.0)
    kids = [place(Node.geo(Sphere() if i % 2 == 0 else Cube(), red if i % 3 else blue), i) for i in range(n)]
    return Scene(root=Node.group(kids), lights=[Light(position=(4.0, 9.0, 12.0), color=(0.9, 0.9, 0.9)), Light(position=(-6.0, 5.0, 3.0), color=(0.3, 0.3, 0.4))],
                 ambient=(0.1, 0.1, 0.1))


def grid(n, phase):
    """n spheres and cubes on a jittered grid; `phase` moves every one of them."""
    rng = np.random.default_rng(77)
    side = int(np.ceil(n ** (1 / 3)))
    jit = rng.uniform(-0.2, 0.2, size=(n, 3))

    def place(node, i):
        x, y, z = i % side, (i // side) % side, i // (side * side)
        node = node.scaled((0.5 + 0.1 * (i % 4), 0.6, 0.5)).rotated_y(0.3 * i + phase)
        return node.translated((1.6 * x + jit[i, 0] + phase, 1.6 * y + jit[i, 1], 1.6 * z + jit[i, 2] - 0.5 * phase * (i % 2)))
    c = 0.8 * (side - 1)
    return (lambda: (spheres_and_cubes(n, place), Camera(eye=(c + 1.0 + phase, c + 2.0, c + 2.2 * side + 2.5), center=(c + phase, c, c), fovy_degrees=45.0), None))


def degenerate(kind, phase):
    def place(node, i):
        if kind == "coincident":
            return node.translated((phase, 0.5, 0.0))
        if kind == "line":
            return node.scaled(0.4).translated((0.9 * i - 28.0 + phase, 0.0, 0.0))
        return (node.scaled(1e6).translated((0.0, -5e5 - 1.0, 0.0)) if i == 0 else node.scaled(0.5).translated((0.7 * (i % 8) - 2.5 + phase, 0.3, 0.7 * (i // 8) - 2.5)))
    eye = {"coincident": (1.5 + phase, 2.0, 3.0), "line": (phase, 6.0, 40.0), "giant": (0.5 + phase, 4.0, 9.0)}[kind]
    center = {"coincident": (phase, 0.5, 0.0), "line": (phase, 0.0, 0.0), "giant": (phase, 0.0, 0.0)}[kind]
    return lambda: (spheres_and_cubes(64, place), Camera(eye=eye, center=center, fovy_degrees=45.0), None)


_CACHE = {}


def case(oracle, key, make):
    """(scene, camera, packed oracle scene, host scene) under `key`, built once"""
    if key not in _CACHE:
        scene, cam = make()
        _CACHE[key] = (scene, cam, oracle.pack(scene), host_glue.host_scene(scene))
    return _CACHE[key]


def reference(oracle, key, mode, w, h):
    k = ("ref", key, mode, w, h)
    if k not in _CACHE:
        _, cam, ps, _ = _CACHE[key]
        _CACHE[k] = oracle.render(ps, cam, w, h, samples=KW["samples"], seed=KW["seed"], jitter=oracle.JITTER_RNG, mode={"flat": oracle.MODE_FLAT, "kd": oracle.MODE_KD, "hier": oracle.MODE_HIER}[mode], kd_depth=8)
    return _CACHE[k]


def shoot(H, r, cam, w, h):
    rgb, lin, st = r.render(host_glue.cam10(cam), w, h, default_background(w, h), stats=True, sample_mode=H.SAMPLE_RNG, **KW)
    plain, plain_lin, st0 = r.render(host_glue.cam10(cam), w, h, default_background(w, h), sample_mode=H.SAMPLE_RNG, **KW)
    assert np.array_equal(rgb, plain) and np.array_equal(lin.view(np.uint64), plain_lin.view(np.uint64))
    return rgb, lin, st, st0


def same_render(got, want, where, variants=True):
    assert np.array_equal(got[0], want[0]), f"{where}: {(got[0] != want[0]).any(axis=2).sum()} pixels differ"
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), f"{where}: linear means differ"
    for k in COUNTERS:
        assert got[2][k] == want[2][k], (where, k, got[2][k], want[2][k])
    if variants:
        for k in ("kernel_mode", "kernel_variant"):
            assert got[2][k] == want[2][k] and got[3][k] == want[3][k], (where, k)


def equals_oracle(got, ref, where):
    assert np.array_equal(got[0], ref.rgb), f"{where}: {(got[0] != ref.rgb).any(axis=2).sum()} pixels differ from the oracle's"
    assert np.array_equal(got[1].view(np.uint64), ref.linear.view(np.uint64)), f"{where}: linear means differ from the oracle's"
    for k in ("primary", "shadow", "reflect", "refract", "hits"):
        assert got[2][k] == ref.stats[k], (where, k)


def scene_info(H, r):
    """pt_test_scene_info: stack_cap, who built the scene-level tree last (0 upload, 1 update on the host, 2 on the device), rounds, tree bytes"""
    out = (C.c_uint64 * 4)()
    assert H.lib().pt_test_scene_info(r.context, C.byref(out)) == 0
    return dict(stack_cap=int(out[0]), builder=int(out[1]), rounds=int(out[2]), tree_bytes=int(out[3]))


def update_and_compare(H, host, oracle, monkeypatch, name, make_a, make_b, mode, builder, w=W, h=HT, differ=0.0):
    monkeypatch.setenv("PORTRAYER_BUILD", builder)
    _, cam_a, _, host_a = case(oracle, (name, "A"), make_a)
    _, cam_b, _, host_b = case(oracle, (name, "B"), make_b)
    ref_b = reference(oracle, (name, "B"), mode, w, h)
    where = f"{name}, {mode}, {builder} build"
    if differ:
        ref_a = reference(oracle, (name, "A"), mode, w, h)
        assert (ref_a.rgb != ref_b.rgb).any(axis=2).mean() >= differ, f"{where}: A and B must look different, or doing nothing would pass"
    r = host.Renderer(host_a, traverse(H, oracle, mode)[0], kd_depth=8)
    fresh = host.Renderer(host_b, traverse(H, oracle, mode)[0], kd_depth=8)
    try:
        shoot(H, r, cam_a, w, h)   # the scene has been in use (occluder tables, work buffers) before it moves
        r.update(host_b)
        got, want = shoot(H, r, cam_b, w, h), shoot(H, fresh, cam_b, w, h)
        info, info_fresh = scene_info(H, r), scene_info(H, fresh)
    finally:
        r.close(); fresh.close()
    n_nodes = len(host_b.flatten()["prim_type"])
    on_device = builder == "device" and n_nodes >= 16
    assert info["builder"] == (2 if on_device else 1) and info_fresh["builder"] == 0, (where, info)
    assert (info["rounds"] > 0) == on_device, (where, info)
    if not on_device:  # the upload's tree: the upload's stack (the clustering tree has a depth of its own)
        assert info["stack_cap"] == info_fresh["stack_cap"], (where, info, info_fresh)
    assert info["tree_bytes"] == info_fresh["tree_bytes"], (where, info, info_fresh)
    same_render(got, want, where)
    equals_oracle(got, ref_b, where)


EXAMPLE_BUILDERS = {"big-scene": lambda: big_scene(10), "macho-cows": macho_cows, "fish": fish, "normal-mapping": normal_mapping, "water-glass": water_glass}


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(EXAMPLE_BUILDERS))
def test_moved_scene_equals_uploaded_scene(H, host, oracle, monkeypatch, name, mode, builder):
    make = EXAMPLE_BUILDERS[name]
    update_and_compare(H, host, oracle, monkeypatch, name, lambda: make()[:2], lambda: moved(make, oracle), mode, builder, differ=0.10)


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 2, 3, 15, 16, 17, 33, 70])
def test_builder_boundaries(H, host, oracle, monkeypatch, n, mode, builder):
    """the device build starts at 16 nodes; it searches 16 places to either side, so 33 and 70 need clusters beyond one window and several rounds"""
    update_and_compare(H, host, oracle, monkeypatch, f"grid-{n}", lambda: grid(n, 0.0)()[:2], lambda: grid(n, 0.9)()[:2], mode, builder, w=64, h=36)


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["coincident", "line", "giant"])
def test_degenerate_placements(H, host, oracle, monkeypatch, kind, mode, builder):
    """64 nodes: all at one place (equal Morton codes, coincident faces: ties are resolved by node index / dfs_rank, not by the tree), all on a line, one 1e6 times the others"""
    update_and_compare(H, host, oracle, monkeypatch, f"degenerate-{kind}", lambda: degenerate(kind, 0.0)()[:2], lambda: degenerate(kind, 1.25)()[:2], mode, builder, w=64, h=36)


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("mode", MODES)
def test_no_state_leaks(H, host, oracle, monkeypatch, mode, builder):
    monkeypatch.setenv("PORTRAYER_BUILD", builder)
    phases = [0.0, 0.9, 0.0, 1.7, 0.4, 0.9]
    scenes = {p: case(oracle, ("grid-70", p), lambda p=p: grid(70, p)()[:2]) for p in set(phases)}
    tr = traverse(H, oracle, mode)[0]
    r = host.Renderer(scenes[0.0][3], tr, kd_depth=8)
    fresh = {}
    try:
        sizes, trees = [], []
        for step, p in enumerate(phases):
            if step:
                r.update(scenes[p][3])
                sizes.append(H.lib().pt_test_scene_bytes(r.context))
                trees.append(scene_info(H, r)["tree_bytes"])
            if p not in fresh:
                f = host.Renderer(scenes[p][3], tr, kd_depth=8)
                fresh[p] = shoot(H, f, scenes[p][1], 64, 36)
                f.close()
            same_render(shoot(H, r, scenes[p][1], 64, 36), fresh[p], f"step {step} (phase {p}), {mode}, {builder} build")
        assert len(set(trees)) == 1, f"the tree buffers grew: {trees}"
        if mode != "kd":
            assert len(set(sizes[1:])) == 1, f"the context's scene buffers grew: {sizes}"
        # the k-d arrays follow the scene and buffers never shrink: once every phase has been seen (step 4) a phase seen before adds nothing
        assert sizes[-1] == sizes[-2], f"the context's scene buffers grew: {sizes}"
    finally:
        r.close()


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["big-scene", "macho-cows"])
def test_the_other_passes_after_an_update(H, host, oracle, monkeypatch, name, mode, builder):
    from test_gpu_rays import incoherent_batch
    monkeypatch.setenv("PORTRAYER_BUILD", builder)
    make = EXAMPLE_BUILDERS[name]
    _, _, _, host_a = case(oracle, (name, "A"), lambda: make()[:2])
    _, cam_b, ps_b, host_b = case(oracle, (name, "B"), lambda: moved(make, oracle))
    if ("batch", name) not in _CACHE:
        _CACHE[("batch", name)] = incoherent_batch(oracle, ps_b, oracle.flatten(ps_b), 4242, n=4096)
    o, d = _CACHE[("batch", name)]
    assert len(o) <= 4096
    tr = traverse(H, oracle, mode)[0]
    r, fresh = host.Renderer(host_a, tr, kd_depth=8), host.Renderer(host_b, tr, kd_depth=8)

    def everything(x):
        out = {"aov." + k: v for k, v in x.aov(host_glue.cam10(cam_b), W, HT).items()}
        for reorder in (False, True):
            out.update({f"rays{int(reorder)}." + k: v for k, v in x.rays(o, d, reorder=reorder).items()})
            out[f"any{int(reorder)}"] = x.rays(o, d, any_hit=True, reorder=reorder)["occluded"]
            out[f"radiance{int(reorder)}"] = x.radiance(o, d, background=(0.1, 0.2, 0.3), seed=9, reorder=reorder)["rgb"]
        return {k: v for k, v in out.items() if not k.endswith("kernel_ms")}
    try:
        everything(r)
        r.update(host_b)
        got, want = everything(r), everything(fresh)
    finally:
        r.close(); fresh.close()
    assert len(got) == 6 + 2 * 7 + 2 + 2
    for k in want:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{name}, {mode}, {builder} build: {k} differs"
    assert (got["aov.node"] >= 0).any() and np.isfinite(got["rays0.t"]).any()


def relit(make, change):
    def build():
        scene, cam = make()[:2]
        change(scene)
        return scene, cam
    return build


def _other_lights(scene):
    scene.lights = [Light(position=(l.position[0] + 3.0, l.position[1] * 0.5 + 1.0, l.position[2] - 2.0), color=(l.color[2], l.color[0] * 0.5, l.color[1]), falloff=l.falloff,
                          area_a=l.area_a, area_b=l.area_b) for l in scene.lights]


def _area_light(scene):
    l = scene.lights[0]
    scene.lights[0] = Light(position=l.position, color=l.color, falloff=l.falloff, area_a=(0.8, 0.0, 0.0), area_b=(0.0, 0.0, 0.8))


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("mode", MODES)
def test_lights_move_and_change_colour(H, host, oracle, monkeypatch, mode, builder):
    update_and_compare(H, host, oracle, monkeypatch, "relit-water-glass", lambda: water_glass()[:2], relit(water_glass, _other_lights), mode, builder, differ=0.10)


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("mode", MODES)
def test_a_point_light_becomes_an_area_light(H, host, oracle, monkeypatch, mode, builder):
    """forkable changes: the dielectric scene's kernel variant after the update is the fresh upload's (same_render compares it)"""
    update_and_compare(H, host, oracle, monkeypatch, "area-refraction", lambda: transmission_refraction()[:2], relit(transmission_refraction, _area_light), mode, builder, w=64, h=36)


@pytest.mark.parametrize("mode", ["flat", "hier"])
@pytest.mark.parametrize("switch", [("PORTRAYER_OCC_SEED", "all:7"), ("PORTRAYER_OCC_SEED", "all:999"), ("PORTRAYER_SHADOW_CACHE", "0")])
def test_shadow_occluder_table(H, host, oracle, monkeypatch, mode, switch):
    monkeypatch.setenv(*switch)
    make = EXAMPLE_BUILDERS["big-scene"]
    for builder in BUILDERS:
        update_and_compare(H, host, oracle, monkeypatch, "big-scene", lambda: make()[:2], lambda: moved(make, oracle), mode, builder)


def kd_of(H, hs, keep):
    t = hs.kdtree(8)
    kdt = H.PtKdTree()
    kdt.n_nodes = len(t["axis"]); kdt.n_items = len(t["items"])
    cols = {k: np.ascontiguousarray(t[k]) for k in ("axis", "plane", "front", "back", "first", "count", "items")}
    keep.append(cols)
    kdt.axis, kdt.front, kdt.back, kdt.first, kdt.count, kdt.leaf_items = (H._p(cols[k], H._ip) for k in ("axis", "front", "back", "first", "count", "items"))
    kdt.plane = H._p(cols["plane"], H._dp)
    kdt.root_min = (C.c_double * 3)(*t["root_bounds"][:3]); kdt.root_max = (C.c_double * 3)(*t["root_bounds"][3:])
    kdt.max_depth = t["max_depth"]
    return kdt


def motion_of(H, hs, mode, keep):
    f = hs.flatten()
    arrays = [np.ascontiguousarray(f[k].reshape(-1, 16)) for k in ("trans", "invtrans", "normal_trans")]
    mo = H.PtSceneMotion()
    mo.n_nodes = len(arrays[0])
    mo.trans, mo.invtrans, mo.normal_trans = (H._p(a, H._dp) for a in arrays)
    if mode == "hier":
        g = hs.graph()
        ga = [np.ascontiguousarray(g[k].reshape(-1, 16)) for k in ("trans", "invtrans", "normal_trans")]
        mo.n_graph_nodes = len(ga[0])
        mo.graph_trans, mo.graph_invtrans, mo.graph_normal_trans = (H._p(a, H._dp) for a in ga)
        arrays += ga
    keep.append(arrays)
    return mo


@pytest.mark.parametrize("mode", MODES)
def test_errors_leave_the_scene_usable(H, host, oracle, monkeypatch, mode):
    monkeypatch.setenv("PORTRAYER_BUILD", "device")
    L = H.lib()
    _, cam_a, _, host_a = case(oracle, ("grid-33", "A"), lambda: grid(33, 0.0)()[:2])
    _, cam_b, _, host_b = case(oracle, ("grid-33", "B"), lambda: grid(33, 0.9)()[:2])
    tr = traverse(H, oracle, mode)[0]
    keep = []
    fresh_ctx = H.Context()
    assert L.pt_scene_update(fresh_ctx.handle, C.byref(motion_of(H, host_b, mode, keep)), None) == -3  # PT_ERR_NO_SCENE
    fresh_ctx.close()
    r = host.Renderer(host_a, tr, kd_depth=8)
    try:
        before = shoot(H, r, cam_a, 64, 36)
        ctx = r.context
        kdt = None
        if mode == "kd":
            kdt = kd_of(H, host_b, keep)
        kdp = C.byref(kdt) if kdt is not None else None

        def refused(mo, kd=kdp):
            return L.pt_scene_update(ctx, C.byref(mo), kd) == -1  # PT_ERR_ARGUMENT
        mo = motion_of(H, host_b, mode, keep); mo.n_nodes += 1
        assert refused(mo)
        mo = motion_of(H, host_b, mode, keep); mo.n_graph_nodes += 1
        assert refused(mo)
        light = np.zeros(30)
        mo = motion_of(H, host_b, mode, keep); mo.lights = H._p(light, H._dp); mo.n_lights = 5
        assert refused(mo)
        if mode == "hier":
            mo = motion_of(H, host_b, mode, keep); mo.graph_invtrans = None
            assert refused(mo)
        if mode == "kd":
            assert refused(motion_of(H, host_b, mode, keep), None)
        if mode == "flat":
            dummy = H.PtKdTree()
            assert refused(motion_of(H, host_b, mode, keep), C.byref(dummy))
        assert L.pt_scene_update(ctx, None, kdp) == -1
        mo = motion_of(H, host_b, mode, keep); mo.trans = None
        assert refused(mo)
        # a render in flight: refused until its _finish
        w, h = 64, 36
        bg = np.ascontiguousarray(default_background(w, h))
        camera = host.camera(host_glue.cam10(cam_a), w, h)
        rp_ = H.PtRenderParams(w, h, H.PtRect(0, 0, w - 1, h - 1), 2, 5, H.SAMPLE_RNG, 1, 0, 1, 0)
        d_bg, d_rgb = C.c_void_p(), C.c_void_p()
        assert L.pt_device_alloc(ctx, bg.nbytes, C.byref(d_bg)) == 0 and L.pt_device_alloc(ctx, w * h * 3, C.byref(d_rgb)) == 0
        assert L.pt_copy_to_device(ctx, d_bg, bg.ctypes.data_as(C.c_void_p), bg.nbytes) == 0
        assert L.pt_render_device(ctx, C.byref(camera), d_bg, C.byref(rp_), 0, d_rgb, None) == 0, L.pt_last_error(ctx)
        assert refused(motion_of(H, host_b, mode, keep))
        assert b"in flight" in L.pt_last_error(ctx)
        st_ = H.PtStats()
        assert L.pt_render_finish(ctx, C.byref(st_)) == 0
        assert L.pt_device_free(ctx, d_bg) == 0 and L.pt_device_free(ctx, d_rgb) == 0
        # a ray pass in flight: refused until its _finish
        o = np.ascontiguousarray(np.tile([0.0, 0.0, 50.0], (64, 1))); d = np.ascontiguousarray(np.tile([0.0, 0.0, -1.0], (64, 1)))
        d_o, d_d, d_t = C.c_void_p(), C.c_void_p(), C.c_void_p()
        for ptr, nbytes in ((d_o, o.nbytes), (d_d, d.nbytes), (d_t, 64 * 8)):
            assert L.pt_device_alloc(ctx, nbytes, C.byref(ptr)) == 0
        assert L.pt_copy_to_device(ctx, d_o, o.ctypes.data_as(C.c_void_p), o.nbytes) == 0 and L.pt_copy_to_device(ctx, d_d, d.ctypes.data_as(C.c_void_p), d.nbytes) == 0
        rp = H.PtRaysParams(64, 0, 0)
        rb = H.PtRaysBuffers(); rb.t = C.cast(d_t, H._dp)
        assert L.pt_rays_device(ctx, C.byref(rp), d_o, d_d, C.byref(rb), None) == 0
        assert refused(motion_of(H, host_b, mode, keep))
        assert b"in flight" in L.pt_last_error(ctx)
        assert L.pt_rays_finish(ctx, None) == 0
        for ptr in (d_o, d_d, d_t):
            assert L.pt_device_free(ctx, ptr) == 0
        # every refusal came before the first write
        same_render(shoot(H, r, cam_a, 64, 36), before, f"after the refused updates, {mode}")
        assert L.pt_scene_update(ctx, C.byref(motion_of(H, host_b, mode, keep)), kdp) == 0, L.pt_last_error(ctx)
        got = shoot(H, r, cam_b, 64, 36)
    finally:
        r.close()
    equals_oracle(got, reference(oracle, ("grid-33", "B"), mode, 64, 36), f"the same update once nothing is in flight, {mode}")


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("mode", MODES)
def test_a_node_of_two_ranks(H, host, oracle, monkeypatch, mode, builder):
    """pt_node_scene_update on two ranks of one device, then pt_node_render: the single context's image; refused while a frame is open"""
    monkeypatch.setenv("PORTRAYER_BUILD", builder)
    _, cam_a, _, host_a = case(oracle, ("grid-33", "A"), lambda: grid(33, 0.0)()[:2])
    _, cam_b, _, host_b = case(oracle, ("grid-33", "B"), lambda: grid(33, 0.9)()[:2])
    ref = reference(oracle, ("grid-33", "B"), mode, 64, 36)
    monkeypatch.setenv("PORTRAYER_DEVICES", "0,0")
    r = host.Renderer(host_a, traverse(H, oracle, mode)[0], kd_depth=8)
    try:
        assert r.ranks == 2 and r.node
        L, w, h, keep = H.lib(), 64, 36, []
        bg = np.ascontiguousarray(default_background(w, h))
        p = H.PtRenderParams(w, h, H.PtRect(0, 0, w - 1, h - 1), 2, 5, H.SAMPLE_RNG, 1, 0, 1, 0)
        camera = host.camera(host_glue.cam10(cam_a), w, h)
        assert L.pt_node_upload_background(r.node, bg.ctypes.data_as(H._dp), C.byref(p), None) == 0, L.pt_node_last_error(r.node)
        assert L.pt_node_frame_begin(r.node, C.byref(camera), C.byref(p)) == 0, L.pt_node_last_error(r.node)
        mo = motion_of(H, host_a, mode, keep)
        assert L.pt_node_scene_update(r.node, C.byref(mo), None) == -1 and b"frames are in flight" in L.pt_node_last_error(r.node)
        assert L.pt_node_frame_end(r.node, C.byref(H.PtStats())) == 0, L.pt_node_last_error(r.node)
        r.update(host_b)
        rgb, _, st = r.render(host_glue.cam10(cam_b), w, h, bg, sample_mode=H.SAMPLE_RNG, want_linear=False, **KW)
    finally:
        r.close()
    assert np.array_equal(rgb, ref.rgb), f"{mode}, {builder} build: {(rgb != ref.rgb).any(axis=2).sum()} pixels differ"


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("mode", MODES)
def test_lights_null_keeps_the_resident_lights(H, host, oracle, monkeypatch, mode, builder):
    """through the C ABI: a renderer on water-glass under OTHER lights, its objects moved with lights = NULL and ambient = NULL: the other lights stay"""
    monkeypatch.setenv("PORTRAYER_BUILD", builder)
    relit_glass = relit(water_glass, _other_lights)
    _, _, _, host_a = case(oracle, ("relit-water-glass", "B"), relit_glass)
    _, cam_b, _, host_b = case(oracle, ("relit-moved-water-glass", "B"), lambda: moved(lambda: (*relit_glass(), None), oracle))
    ref = reference(oracle, ("relit-moved-water-glass", "B"), mode, W, HT)
    keep = []
    r = host.Renderer(host_a, traverse(H, oracle, mode)[0], kd_depth=8)
    try:
        mo = motion_of(H, host_b, mode, keep)
        assert not mo.lights and not mo.ambient
        kdt = kd_of(H, host_b, keep) if mode == "kd" else None
        assert H.lib().pt_scene_update(r.context, C.byref(mo), C.byref(kdt) if kdt is not None else None) == 0, H.lib().pt_last_error(r.context)
        got = shoot(H, r, cam_b, W, HT)
    finally:
        r.close()
    equals_oracle(got, ref, f"lights = NULL, {mode}, {builder} build")


@pytest.mark.parametrize("builder", BUILDERS)
def test_kd_stack_follows_the_new_kd_tree(H, host, oracle, monkeypatch, builder):
    """64 nodes at one place (the k-d build splits them down to its depth limit) moved apart (a shallower tree) and back, so the k-d depth
    falls and rises: stack_cap is the fresh upload's each time, whatever the scene was before"""
    monkeypatch.setenv("PORTRAYER_BUILD", "host")  # the fresh uploads' tree, so that stack_cap can be compared ...
    _, cam_a, _, host_a = case(oracle, ("degenerate-coincident", "A"), lambda: degenerate("coincident", 0.0)()[:2])
    _, cam_b, _, host_b = case(oracle, ("spread-64", "B"), lambda: (spheres_and_cubes(64, lambda node, i: node.scaled(0.4).translated((3.0 * (i % 4), 3.0 * ((i // 4) % 4), 3.0 * (i // 16)))),
                                                                      Camera(eye=(6.0, 7.0, 30.0), center=(4.5, 4.5, 4.5), fovy_degrees=45.0)))
    depth_a, depth_b = host_a.kdtree(8)["max_depth"], host_b.kdtree(8)["max_depth"]
    assert abs(depth_b - depth_a) > 2, (depth_a, depth_b)
    fresh = {}
    for name, hs in (("A", host_a), ("B", host_b)):
        f = host.Renderer(hs, H.TRAVERSE_KD, kd_depth=8)
        fresh[name] = scene_info(H, f)["stack_cap"]
        f.close()
    assert fresh["B"] == fresh["A"] + 3 * (depth_b - depth_a)  # (pt_set_stack_cap: three entries per k-d level)
    monkeypatch.setenv("PORTRAYER_BUILD", builder)  # ... the k-d walk's stack does not depend on the scene-level tree
    r = host.Renderer(host_a, H.TRAVERSE_KD, kd_depth=8)
    try:
        for name, hs in (("B", host_b), ("B", host_b), ("A", host_a), ("B", host_b)):
            r.update(hs)
            assert scene_info(H, r)["stack_cap"] == fresh[name], (name, builder)
        got = shoot(H, r, cam_b, 64, 36)
    finally:
        r.close()
    equals_oracle(got, reference(oracle, ("spread-64", "B"), "kd", 64, 36), f"spread-64 after coincident, {builder} build")
