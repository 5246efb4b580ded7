"""Per-pixel candidate lists for primary rays (pt_pixel_list.h; pt_api.hip: pt_pixel_list_kernel; pt_render_simple.h: PIXEL_LISTS): where a wavefront is
one pixel, the mesh-free flat_scene kernel's primary stage runs the walk's own leaf test on the list of leaves the pixel's beam reaches instead of walking the tree, and a
pixel with an empty list is background without a ray. The tree only ever culled, so every image and every f64 mean must stay the oracle's, bit for bit - by the default
path, with PORTRAYER_PIXEL_LISTS=0 (the walk, from the same library) and with PORTRAYER_PIXEL_LIST_CAP = 0, 1, 2, which cuts every list short so that small scenes
reach the tail-bound stop and the fall-back to the walk. (A cap of 0 with a reached leaf is a list of length 0 that is NOT background; a cap of k against k + 1 reached
leaves is the list of length K + 1.)"""
import ctypes as C

import numpy as np
import pytest

import host_glue
from scene_dsl import Camera, Cone, Cube, Cylinder, Light, Material, Node, Plane, Scene, Sphere, Triangle, default_background
from ulp import assert_ulp

pytestmark = pytest.mark.gpu

VARIANTS = [("default", {}), ("walk", {"PORTRAYER_PIXEL_LISTS": "0"}), ("cap 0", {"PORTRAYER_PIXEL_LIST_CAP": "0"}), ("cap 1", {"PORTRAYER_PIXEL_LIST_CAP": "1"}),
            ("cap 2", {"PORTRAYER_PIXEL_LIST_CAP": "2"})]
KEYS = ("PORTRAYER_PIXEL_LISTS", "PORTRAYER_PIXEL_LIST_CAP")


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


@pytest.fixture(scope="module")
def big(host, oracle):
    """big-scene, its packed arrays for the oracle, its camera - and the oracle's renders, each computed once."""
    from example_scenes import EXAMPLES
    from scene_dsl import ASSETS
    sc = host.Scene.example("big-scene", assets=ASSETS)
    packed = oracle.pack_arrays(sc.export())
    cam = EXAMPLES["big-scene"]()[1]
    refs = {}

    def ref(w, h, samples, seed):
        key = (w, h, samples, seed)
        if key not in refs:
            refs[key] = oracle.render(packed, cam, w, h, samples=samples, seed=seed, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
        return refs[key]
    return sc, ref


def variants(monkeypatch):
    """Yields each variant's name with its environment set."""
    for name, env in VARIANTS:
        for k in KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        yield name
    for k in KEYS:
        monkeypatch.delenv(k, raising=False)


def flat_kernel(H, st):
    return st["kernel_mode"] == 3 and not st["kernel_variant"] & (H.KERNEL_CHAIN | H.KERNEL_INTERPRETER | H.KERNEL_COUNTING)


def summary(H, r):
    """pt_test_pixel_list_summary of the renderer's last launch: records, background, cut at the cap, marked, and the records by length."""
    out = (C.c_uint64 * 32)()  # (the hook writes 5 + K words, K = 6 as shipped; room for any K a build may have)
    assert H.lib().pt_test_pixel_list_summary(r.context, out) == 0, H.lib().pt_last_error(r.context)
    s = [int(v) for v in out]
    return {"records": s[0], "background": s[1], "cut": s[2], "marked": s[3], "by_length": s[4:]}


def check_lists(name, s, base, lists=True):
    """What the launch's records must look like under variant `name` (base: the default variant's summary): that the path ran at all, and that the cap cut what it had to."""
    if not lists or name == "walk":
        assert s["records"] == 0, (name, s)
        return
    assert s["records"] > 0 and s["records"] % 64 == 0 and s["marked"] == 0 and sum(s["by_length"]) == s["records"], (name, s)
    if name == "default":
        return
    cap = int(name.split()[1])
    assert not any(s["by_length"][cap + 1:]), (name, s)
    longer = sum(base["by_length"][cap + 1:])  # the records the cap cuts: each must report a finite tail
    assert s["cut"] >= longer, (name, s, base)
    assert (s["cut"] > 0) == (longer + base["cut"] > 0), (name, s, base)
    assert s["background"] == base["background"], (name, s, base)  # an empty list with nothing left out stays what it is under any cap


def check(monkeypatch, H, r, cam10, ref, w, h, samples, seed, rect=None, lists=True):
    """The five renders against the oracle's image and f64 means (inside rect, where one is given: pixels outside keep the caller's bytes). Returns the default variant's summary."""
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, w - 1, h - 1)
    base = None
    for name in variants(monkeypatch):
        rgb, lin, st = r.render(cam10, w, h, default_background(w, h), samples=samples, seed=seed, sample_mode=H.SAMPLE_RNG, rect=rect)
        assert flat_kernel(H, st), (name, st)
        a, b = rgb[y0:y1 + 1, x0:x1 + 1], ref.rgb[y0:y1 + 1, x0:x1 + 1]
        assert np.array_equal(a, b), f"{name}: {(a != b).any(axis=2).sum()} pixels differ from the oracle"
        assert_ulp(lin[y0:y1 + 1, x0:x1 + 1], ref.linear[y0:y1 + 1, x0:x1 + 1], 0, name)
        if rect is not None:
            outside = np.ones((h, w), bool)
            outside[y0:y1 + 1, x0:x1 + 1] = False
            assert not rgb[outside].any()
        s = summary(H, r)
        if name == "default":
            base = s
        check_lists(name, s, base, lists)
    return base


def check_scene(monkeypatch, host, H, oracle, scene, cam, w=16, h=16, samples=64, seed=5):
    ref = oracle.render(scene, cam, w, h, samples=samples, seed=seed, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
    r = host.Renderer(host_glue.host_scene(scene), H.TRAVERSE_FLAT)
    try:
        base = check(monkeypatch, H, r, host_glue.cam10(cam), ref, w, h, samples, seed)
    finally:
        r.close()
    ref.lists = base
    return ref


# ---- big-scene

@pytest.mark.parametrize("w,h,samples", [(96, 64, 64), (93, 61, 64), (32, 24, 128), (96, 64, 16)],
                         ids=["whole tiles", "partial tiles", "two chunk groups per pixel", "several pixels per wavefront: the path is off"])
def test_big_scene(host, H, big, monkeypatch, w, h, samples):
    sc, ref = big
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    try:
        rf = ref(w, h, samples, 3)
        assert 0 < rf.stats["hits"] < rf.stats["primary"]  # hits and background both
        base = check(monkeypatch, H, r, sc.camera, rf, w, h, samples, 3, lists=samples != 16)
        if samples != 16:  # background pixels, lists of one entry, of several, and lists cut at the shipped K = 6 (the K + 1 case against the real K)
            tiles_x, tiles_y = (w + 7) // 8, (h + 7) // 8
            assert base["records"] == tiles_x * tiles_y * 64
            assert base["background"] > 0 and base["by_length"][1] > 0 and sum(base["by_length"][3:]) > 0 and base["cut"] > 0, base
    finally:
        r.close()


def test_big_scene_slice_off_the_tile_grid(host, H, big, monkeypatch):
    """x0, y0 no multiples of 8: the launch's tiles start at the slice's corner, and the last ones are partial."""
    sc, ref = big
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    try:
        check(monkeypatch, H, r, sc.camera, ref(96, 64, 64, 3), 96, 64, 64, 3, rect=(13, 5, 70, 49))
    finally:
        r.close()


def test_big_scene_two_rank_tile_partition(host, H, big, monkeypatch):
    """Rank 0 of 2, then rank 1 of 2, into the same buffers (pt_render: pixels of the other rank's tiles keep the caller's bytes): a launch's records are its OWN tiles'."""
    sc, ref = big
    w, h, samples, seed = 93, 61, 64, 3
    rf = ref(w, h, samples, seed)
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    lib, c = H.lib(), r.context
    bg = np.ascontiguousarray(default_background(w, h))
    cam = host.camera(sc.camera, w, h)
    dp = C.POINTER(C.c_double)
    try:
        for name in variants(monkeypatch):
            rgb = np.zeros((h, w, 3), np.uint8)
            lin = np.zeros((h, w, 3), np.float64)
            for rank in (0, 1):
                p = H.PtRenderParams(w, h, H.PtRect(0, 0, w - 1, h - 1), samples, seed, H.SAMPLE_RNG, 1 if bg.shape == (h, 3) else 0, rank, 2, 0)
                st = H.PtStats()
                assert lib.pt_render(c, C.byref(cam), bg.ctypes.data_as(dp), C.byref(p), rgb.ctypes.data_as(C.POINTER(C.c_uint8)), lin.ctypes.data_as(dp), C.byref(st)) == 0, lib.pt_last_error(c)
                assert flat_kernel(H, st.as_dict())
                if rank == 0:
                    assert (rgb != rf.rgb).any()  # half of the tiles are still the caller's zeros
                tiles = ((w + 7) // 8) * ((h + 7) // 8)
                sm = summary(H, r)
                assert sm["records"] in ((0,) if name == "walk" else ((tiles // 2) * 64, ((tiles + 1) // 2) * 64)), (name, rank, sm)  # a rank's share of the tiles, not all of them
            assert np.array_equal(rgb, rf.rgb), f"{name}: {(rgb != rf.rgb).any(axis=2).sum()} pixels differ from the oracle"
            assert_ulp(lin, rf.linear, 0, name)
    finally:
        r.close()


# ---- small scenes

def lights():
    return [Light(position=(3.0, 8.0, 6.0), color=(0.7, 0.7, 0.7)), Light(position=(-5.0, 6.0, 4.0), color=(0.3, 0.3, 0.4), falloff=(1.0, 0.01, 0.001)),
            Light(position=(0.0, 2.0, 9.0), color=(0.3, 0.2, 0.2))]


def materials():
    return [Material(diffuse=(0.8, 0.3, 0.2), specular=(0.5, 0.5, 0.5), shininess=25.0), Material(diffuse=(0.2, 0.7, 0.3), specular=(0.0, 0.0, 0.0)),
            Material(diffuse=(0.3, 0.4, 0.8), specular=(0.6, 0.6, 0.3), shininess=300.0)]


def a_triangle():
    return Triangle((-0.9, -0.7, 0.0), (1.0, -0.5, 0.2), (0.1, 0.9, -0.1))


def posed(node, k):
    return (node.scaled((0.9 + 0.35 * k, 1.4 - 0.2 * k, 0.7 + 0.25 * k)).rotated_xzy((0.4 + 0.5 * k, -0.7 + 0.3 * k, 1.1 - 0.6 * k))
            .translated((-2.2 + 1.5 * k, 0.4 * (k % 2) - 0.3, -0.5 * k)))


def several(extra=()):
    m = materials()
    kids = [posed(Node.geo(p(), m[k % 3]), k) for k, p in enumerate((Sphere, Cube, Cylinder, Cone))]
    return Scene(root=Node.group(kids + list(extra)), lights=lights(), ambient=(0.1, 0.1, 0.1))


def test_two_frames_open_on_the_two_slots(host, H, oracle, monkeypatch):
    """pt_render_device on the context's two streams, both open at once, with different cameras: a slot's records are its own frame's."""
    scene = several()
    cams = [Camera(eye=(0.7, 1.9, 7.5), center=(0.0, 0.2, 0.0)), Camera(eye=(-6.0, 3.0, 2.5), center=(0.2, 0.0, -0.5)), Camera(eye=(2.0, -1.0, 9.0), center=(0.0, 0.2, 0.0))]
    w, h, samples = 24, 16, 64
    refs = [oracle.render(scene, cam, w, h, samples=samples, seed=20 + k, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT) for k, cam in enumerate(cams)]
    assert not np.array_equal(refs[0].rgb, refs[1].rgb)
    r = host.Renderer(host_glue.host_scene(scene), H.TRAVERSE_FLAT)
    lib, c = H.lib(), r.context
    bg = np.ascontiguousarray(default_background(w, h))
    d_bg, d_img = C.c_void_p(), [C.c_void_p(), C.c_void_p()]
    try:
        assert lib.pt_device_alloc(c, bg.nbytes, C.byref(d_bg)) == 0 and lib.pt_copy_to_device(c, d_bg, bg.ctypes.data_as(C.c_void_p), bg.nbytes) == 0
        for d in d_img:
            assert lib.pt_device_alloc(c, w * h * 3, C.byref(d)) == 0
        for name in variants(monkeypatch):
            st, got, slots = H.PtStats(), [], []

            def close(k):
                assert lib.pt_render_finish(c, C.byref(st)) == 0, lib.pt_last_error(c)
                img = np.zeros((h, w, 3), dtype=np.uint8)
                assert lib.pt_copy_from_device(c, img.ctypes.data_as(C.c_void_p), d_img[slots[k]], img.nbytes) == 0
                got.append((img, st.as_dict()))

            for k, cam in enumerate(cams):
                slot = int(lib.pt_context_next_slot(c))
                slots.append(slot)
                p = H.PtRenderParams(w, h, H.PtRect(0, 0, w - 1, h - 1), samples, 20 + k, H.SAMPLE_RNG, 1 if bg.shape == (h, 3) else 0, 0, 1, 0)
                camera = host.camera(host_glue.cam10(cam), w, h)
                assert lib.pt_render_device(c, C.byref(camera), d_bg, C.byref(p), 0, d_img[slot], C.c_void_p(lib.pt_context_stream(c, slot))) == 0, lib.pt_last_error(c)
                if k > 0:
                    close(k - 1)
            close(len(cams) - 1)
            assert slots[0] != slots[1]
            sm = summary(H, r)  # (the last frame's; the device path has no f64 means to compare: pt_render_device writes the 8-bit image only)
            assert sm["records"] == (0 if name == "walk" else ((w + 7) // 8) * ((h + 7) // 8) * 64), (name, sm)
            for k, ((img, stk), ref) in enumerate(zip(got, refs)):
                assert flat_kernel(H, stk), stk
                assert np.array_equal(img, ref.rgb), f"{name}, frame {k}: {(img != ref.rgb).any(axis=2).sum()} pixels differ from its own camera's image"
    finally:
        for d in d_img + [d_bg]:
            if d:
                lib.pt_device_free(c, d)
        r.close()


def test_a_camera_inside_a_primitives_box(host, H, oracle, monkeypatch):
    """The eye inside a room (a cube and a sphere around it): the boxes contain the eye, every bound is 0, every primary ray hits."""
    m = materials()
    room = [Node.geo(Cube(), m[1]).scaled((30.0, 28.0, 32.0)).rotated_y(0.2), Node.geo(Sphere(), m[2]).scaled((12.0, 11.0, 13.0)).translated((0.5, 0.0, 0.5))]
    ref = check_scene(monkeypatch, host, H, oracle, several(room), Camera(eye=(0.25, 0.5, 6.5), center=(0.0, 0.2, 0.0)))
    assert ref.stats["hits"] == ref.stats["primary"]


@pytest.mark.parametrize("size", [(16, 16), (9, 7)], ids=["even", "odd"])
def test_a_camera_looking_exactly_along_an_axis(host, H, oracle, monkeypatch, size):
    """Directions with exact zeros on the centre row and column of an odd-sized image, ranges that touch or straddle zero beside the centre lines of an even one."""
    m = materials()
    kids = [Node.geo(Cube(), m[0]).translated((0.0, 0.0, 0.0)), Node.geo(Sphere(), m[1]).scaled(0.6).translated((1.5, 0.0, 1.0)),
            Node.geo(Cylinder(), m[2]).scaled(0.5).translated((0.0, 1.5, -1.0)), Node.geo(Cone(), m[0]).scaled(0.7).translated((-1.5, -1.0, 0.5))]
    scene = Scene(root=Node.group(kids), lights=lights(), ambient=(0.1, 0.1, 0.1))
    ref = check_scene(monkeypatch, host, H, oracle, scene, Camera(eye=(0.0, 0.0, 8.0), center=(0.0, 0.0, 0.0), fovy_degrees=40.0), w=size[0], h=size[1])
    assert 0 < ref.stats["hits"] < ref.stats["primary"]


def test_two_coincident_primitives(host, H, oracle, monkeypatch):
    """The same sphere twice, in two colours: every hit is an exact tie, and the lower index wins whichever is tested first - with a cap of 1 one of the two is the tail."""
    m = materials()
    twin = lambda mat: Node.geo(Sphere(), mat).scaled((1.5, 1.2, 1.0)).rotated_z(0.3).translated((0.3, 0.2, 0.0))
    scene = Scene(root=Node.group([twin(m[0]), twin(m[2]), Node.geo(Cube(), m[1]).translated((-2.5, 0.0, -1.0))]), lights=lights(), ambient=(0.1, 0.1, 0.1))
    ref = check_scene(monkeypatch, host, H, oracle, scene, Camera(eye=(0.7, 1.9, 7.5), center=(0.0, 0.2, 0.0)))
    assert ref.stats["hits"] > 0


def test_a_plane_and_a_stand_alone_triangle(host, H, oracle, monkeypatch):
    m = materials()
    extra = [Node.geo(Plane(), m[0]).scaled(30.0).translated((0.0, -2.0, 0.0)), posed(Node.geo(a_triangle(), m[1]), 4)]
    ref = check_scene(monkeypatch, host, H, oracle, several(extra), Camera(eye=(0.7, 1.9, 7.5), center=(0.0, 0.2, 0.0)))
    assert ref.stats["hits"] > 0


def test_sheared_and_very_small_nodes(host, H, oracle, monkeypatch):
    """A group's non-uniform scale over rotated children (sheared composites) and primitives of 1e-3 of the frame: boxes thinner than a pixel's beam."""
    m = materials()
    inner = [Node.geo(p(), m[k % 3]).scaled((1.6, 0.7, 1.1)).rotated_xzy((0.4 + 0.3 * k, 0.2 * k, 0.7)).translated((-3.0 + 2.0 * k, 1.2, 0.5 * (k % 2)))
             for k, p in enumerate((Sphere, Cube, Cylinder, Cone))]
    small = [Node.geo(p(), m[k % 3]).scaled(0.004).translated((-0.6 + 0.4 * k, -0.5 + 0.1 * k, 2.0)) for k, p in enumerate((Sphere, Cube, Cylinder, Cone))]
    scene = Scene(root=Node.group([Node.group(inner).scaled((1.3, 0.8, 1.0)).rotated_y(0.3)] + small), lights=lights(), ambient=(0.1, 0.1, 0.1))
    ref = check_scene(monkeypatch, host, H, oracle, scene, Camera(eye=(0.0, 2.0, 11.0), center=(0.0, 0.5, 0.0)), w=24, h=16)
    assert ref.stats["hits"] > 0


def test_every_pixel_is_background(host, H, oracle, monkeypatch):
    """The scene lies behind the camera: every list is empty with an infinite tail - one 8x8 tile, no ray drawn."""
    ref = check_scene(monkeypatch, host, H, oracle, several(), Camera(eye=(0.7, 1.9, 7.5), center=(0.7, 1.9, 20.0)), w=8, h=8)
    assert ref.stats["hits"] == 0
    assert ref.lists["records"] == 64 and ref.lists["background"] == 64  # one tile, every list empty with nothing left out


def test_one_primitive_fills_the_frame(host, H, oracle, monkeypatch):
    """A scene of ONE node - the tree's root is a leaf, every list has length 1 - that covers every pixel of one 8x8 tile."""
    scene = Scene(root=Node.group([Node.geo(Cube(), materials()[0]).scaled((40.0, 40.0, 1.0)).rotated_z(0.1).translated((0.0, 0.0, -3.0))]), lights=lights(), ambient=(0.1, 0.1, 0.1))
    ref = check_scene(monkeypatch, host, H, oracle, scene, Camera(eye=(0.3, 0.4, 7.0), center=(0.0, 0.0, 0.0)), w=8, h=8)
    assert ref.stats["hits"] == ref.stats["primary"]
    assert ref.lists["by_length"][1] == 64 and ref.lists["cut"] == 0  # every list has length 1; under a cap of 0 (check_lists) each is cut: length 0, not background
