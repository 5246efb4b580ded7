"""The eye table of the mesh-free flat_scene straight-line kernels (pt_api.hip: pt_eye_table_kernel; pt_walk_wave.h: pt_test_node_uniform<EYE>; pt_shade.h:
pt_hit_model<EYE>): the camera's eye in every node's space is worked out once per launch and read through the scalar cache by the primary walk's leaf tests
and by the surface of a primary hit, instead of being transformed in every lane. The same function on the same operands, so every image and every f64 mean
must stay what the oracle computes, bit for bit:

 * every primitive type under a non-uniform scale, a rotation about all three axes and a translation, a wavefront being one, four and 64 pixels;
 * eyes with a zero and a -0.0 component, inside a cube, inside a sphere, and at a primitive's model origin;
 * the scene's highest-numbered node covering the frame: the table's last record;
 * two frames open at once with different cameras (a table per slot), a node moved between two renders (a table per launch);
 * the hierarchical kernel and the counting instantiation, which keep the per-lane transform; big-scene with the occluder table and without it."""
import ctypes as C

import numpy as np
import pytest

import host_glue
from scene_dsl import Camera, Cone, Cube, Cylinder, Light, Material, Node, Plane, Scene, Sphere, Triangle, default_background
from ulp import assert_ulp

pytestmark = pytest.mark.gpu

SIZES = [((16, 16), 64), ((32, 16), 16), ((48, 32), 1)]  # a wavefront = one pixel, four pixels, 64 pixels


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def lights():
    return [Light(position=(3.0, 8.0, 6.0), color=(0.7, 0.7, 0.7)), Light(position=(-5.0, 6.0, 4.0), color=(0.3, 0.3, 0.4), falloff=(1.0, 0.01, 0.001)),
            Light(position=(0.0, 2.0, 9.0), color=(0.3, 0.2, 0.2))]


def materials():
    return [Material(diffuse=(0.8, 0.3, 0.2), specular=(0.5, 0.5, 0.5), shininess=25.0), Material(diffuse=(0.2, 0.7, 0.3), specular=(0.0, 0.0, 0.0)),
            Material(diffuse=(0.3, 0.4, 0.8), specular=(0.6, 0.6, 0.3), shininess=300.0)]


def a_triangle(k=0):
    return Triangle((-0.9, -0.7, 0.1 * k), (1.0, -0.5, 0.2), (0.1, 0.9, -0.1), normals=((0.1, 0.0, 1.0), (0.0, 0.2, 1.0), (-0.1, 0.1, 1.0)) if k % 2 else None)


PRIMS = {"sphere": Sphere, "cube": Cube, "cylinder": Cylinder, "cone": Cone, "plane": Plane, "triangle": a_triangle}


def posed(node, k):
    """Scaled non-uniformly, rotated about all three axes, translated - differently for every k."""
    return (node.scaled((0.9 + 0.35 * k, 1.4 - 0.2 * k, 0.7 + 0.25 * k)).rotated_xzy((0.4 + 0.5 * k, -0.7 + 0.3 * k, 1.1 - 0.6 * k))
            .translated((-2.2 + 1.5 * k, 0.4 * (k % 2) - 0.3, -0.5 * k)))


def prim_scene(kind):
    """Four nodes of one primitive type and a stand-alone triangle among them, one of the four inside a transformed group."""
    m = materials()
    kids = [posed(Node.geo(PRIMS[kind](), m[k % 3]), k) for k in range(3)]
    kids.insert(2, posed(Node.geo(a_triangle(1), m[1]), 4))
    kids.append(Node.group([posed(Node.geo(PRIMS[kind](), m[2]), 3)]).scaled((1.1, 0.9, 1.0)).rotated_z(0.3).translated((0.2, 1.0, -1.0)))
    return Scene(root=Node.group(kids), lights=lights(), ambient=(0.1, 0.1, 0.1))


def flat_kernel(H, st):
    return st["kernel_mode"] == 3 and not st["kernel_variant"] & (H.KERNEL_CHAIN | H.KERNEL_INTERPRETER)


def check(host, H, oracle, scene, cam, w, h, samples, seed, r=None):
    """One plain render in the flat_scene semantics against the oracle; returns the oracle's result."""
    ref = oracle.render(scene, cam, w, h, samples=samples, seed=seed, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
    own = r is None
    if own:
        r = host.Renderer(host_glue.host_scene(scene), H.TRAVERSE_FLAT)
    try:
        rgb, lin, st = r.render(host_glue.cam10(cam), w, h, default_background(w, h), samples=samples, seed=seed, sample_mode=H.SAMPLE_RNG)
    finally:
        if own:
            r.close()
    assert flat_kernel(H, st), st
    assert np.array_equal(rgb, ref.rgb), f"{(rgb != ref.rgb).any(axis=2).sum()} pixels differ"
    assert_ulp(lin, ref.linear, 0)
    return ref


@pytest.mark.parametrize("size,samples", SIZES)
@pytest.mark.parametrize("kind", list(PRIMS))
def test_every_primitive_type(host, H, oracle, kind, size, samples):
    cam = Camera(eye=(0.7, 1.9, 7.5), center=(0.0, 0.2, 0.0), fovy_degrees=50.0)
    ref = check(host, H, oracle, prim_scene(kind), cam, size[0], size[1], samples, 5)
    assert ref.stats["hits"] > 0


def room_scene():
    """A few primitives inside a cube of side 30 and a sphere of radius 12 (scaled, rotated): an eye near the origin is inside both."""
    m = materials()
    kids = [posed(Node.geo(p(), m[k % 3]), k) for k, p in enumerate((Sphere, Cube, Cylinder, Cone))]
    kids.append(Node.geo(Cube(), m[1]).scaled((30.0, 28.0, 32.0)).rotated_y(0.2))
    kids.append(Node.geo(Sphere(), m[2]).scaled((12.0, 11.0, 13.0)).rotated_xzy((0.1, 0.2, 0.3)).translated((0.5, 0.0, 0.5)))
    return Scene(root=Node.group(kids), lights=[Light(position=(1.0, 4.0, 5.0), color=(0.7, 0.7, 0.7)), Light(position=(-3.0, 2.0, 4.0), color=(0.3, 0.3, 0.4)),
                                                Light(position=(0.0, -2.0, 6.0), color=(0.3, 0.2, 0.2))], ambient=(0.1, 0.1, 0.1))


def origin_scene(eye):
    """A sphere and a cube whose model origins are the eye (unrotated: the inverse's translation cancels the scaled eye exactly; and rotated), in front of other nodes."""
    m = materials()
    kids = [posed(Node.geo(p(), m[k % 3]), k) for k, p in enumerate((Sphere, Cube, Cylinder, Cone))]
    kids.append(Node.geo(Sphere(), m[0]).scaled((2.0, 4.0, 8.0)).translated(eye))
    kids.append(Node.geo(Cube(), m[1]).scaled((40.0, 36.0, 44.0)).rotated_xzy((0.3, -0.2, 0.5)).translated(eye))
    return Scene(root=Node.group(kids), lights=lights(), ambient=(0.1, 0.1, 0.1))


EYES = {
    "zero-component": lambda: (prim_scene("cube"), Camera(eye=(0.0, 2.0, 7.0), center=(0.3, 0.2, 0.0))),
    "minus-zero-component": lambda: (prim_scene("cylinder"), Camera(eye=(-0.0, 2.0, 7.0), center=(0.3, 0.2, 0.0))),
    "two-minus-zeros": lambda: (prim_scene("sphere"), Camera(eye=(-0.0, -0.0, 8.0), center=(0.3, 0.2, 0.0))),
    "inside-cube-and-sphere": lambda: (room_scene(), Camera(eye=(0.25, 0.5, 6.5), center=(0.0, 0.2, 0.0))),
    "model-origin": lambda: (origin_scene((0.5, 1.25, 6.0)), Camera(eye=(0.5, 1.25, 6.0), center=(0.0, 0.2, 0.0))),
}


@pytest.mark.parametrize("size,samples", [((16, 16), 64), ((48, 32), 1)])
@pytest.mark.parametrize("name", list(EYES))
def test_eyes(host, H, oracle, name, size, samples):
    scene, cam = EYES[name]()
    ref = check(host, H, oracle, scene, cam, size[0], size[1], samples, 6)
    assert ref.stats["hits"] > 0
    if name in ("inside-cube-and-sphere", "model-origin"):  # closed rooms around the eye: every primary ray hits
        assert ref.stats["hits"] == ref.stats["primary"]


def test_the_last_node_covers_the_frame(host, H, oracle):
    """The wall is the scene's highest-numbered node: most pixels' walks and surfaces read the table's last record."""
    m = materials()
    kids = [posed(Node.geo(p(), m[k % 3]).scaled(0.3), k) for k, p in enumerate((Sphere, Cube, Cylinder, Cone))]
    kids.append(Node.geo(Cube(), m[0]).scaled((40.0, 40.0, 1.0)).rotated_z(0.1).translated((0.0, 0.0, -3.0)))
    scene = Scene(root=Node.group(kids), lights=lights(), ambient=(0.1, 0.1, 0.1))
    ex = host_glue.host_scene(scene).export()
    assert int(ex["prim_type"][-1]) == 5  # (pt_prims.h PT_CUBE) the wall closes the node arrays
    for (w, h), samples in SIZES:
        ref = check(host, H, oracle, scene, Camera(eye=(0.3, 0.4, 7.0), center=(0.0, 0.0, 0.0)), w, h, samples, 11)
        assert ref.stats["hits"] > 0.9 * w * h * samples


def test_two_frames_in_flight_with_different_cameras(host, H, oracle):
    """pt_render_device on the context's two streams, both open at once (bench.py --overlap's calls): each image is its own camera's. A table shared between the
    slots would give the first frame the second camera's eye (or half of each)."""
    scene = prim_scene("cube")
    cams = [Camera(eye=(0.7, 1.9, 7.5), center=(0.0, 0.2, 0.0)), Camera(eye=(-6.0, 3.0, 2.5), center=(0.2, 0.0, -0.5)), Camera(eye=(2.0, -1.0, 9.0), center=(0.0, 0.2, 0.0)),
            Camera(eye=(0.0, 6.0, 4.0), center=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0))]
    w, h, samples = 64, 48, 64
    refs = [oracle.render(scene, cam, w, h, samples=samples, seed=20 + k, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT) for k, cam in enumerate(cams)]
    r = host.Renderer(host_glue.host_scene(scene), H.TRAVERSE_FLAT)
    lib, c = H.lib(), r.context
    bg = np.ascontiguousarray(default_background(w, h))
    d_bg, d_img = C.c_void_p(), [C.c_void_p(), C.c_void_p()]
    try:
        assert lib.pt_device_alloc(c, bg.nbytes, C.byref(d_bg)) == 0 and lib.pt_copy_to_device(c, d_bg, bg.ctypes.data_as(C.c_void_p), bg.nbytes) == 0
        for d in d_img:
            assert lib.pt_device_alloc(c, w * h * 3, C.byref(d)) == 0
        assert lib.pt_context_stream(c, 0) != lib.pt_context_stream(c, 1)
        st, got, slots = H.PtStats(), [], []

        def close(k):  # the oldest open frame is frame k
            assert lib.pt_render_finish(c, C.byref(st)) == 0, lib.pt_last_error(c)
            img = np.zeros((h, w, 3), dtype=np.uint8)
            assert lib.pt_copy_from_device(c, img.ctypes.data_as(C.c_void_p), d_img[slots[k]], img.nbytes) == 0
            got.append((img, st.as_dict()))

        for k, cam in enumerate(cams):
            slot = int(lib.pt_context_next_slot(c))
            slots.append(slot)
            p = H.PtRenderParams(w, h, H.PtRect(0, 0, w - 1, h - 1), samples, 20 + k, H.SAMPLE_RNG, 1, 0, 1, 0)
            camera = host.camera(host_glue.cam10(cam), w, h)
            assert lib.pt_render_device(c, C.byref(camera), d_bg, C.byref(p), 0, d_img[slot], C.c_void_p(lib.pt_context_stream(c, slot))) == 0, lib.pt_last_error(c)
            if k > 0:
                close(k - 1)
        close(len(cams) - 1)
        assert slots == [0, 1, 0, 1]
        for k, ((img, stk), ref) in enumerate(zip(got, refs)):
            assert flat_kernel(H, stk), stk
            assert np.array_equal(img, ref.rgb), f"frame {k}: {(img != ref.rgb).any(axis=2).sum()} pixels differ from its own camera's image"
    finally:
        for d in d_img + [d_bg]:
            if d:
                lib.pt_device_free(c, d)
        r.close()


def test_a_node_moves_between_two_renders(host, H, oracle):
    """pt_scene_update moves and rotates one node; the same renderer then renders the moved scene. A table that outlived the first launch would still hold the
    eye in the node's old space."""
    def scene_at(phase):
        m = materials()
        kids = [posed(Node.geo(p(), m[k % 3]), k) for k, p in enumerate((Sphere, Cube, Cylinder, Cone))]
        kids.append(Node.geo(Cube(), m[1]).scaled((1.5, 0.8, 1.1)).rotated_xzy((0.2 + phase, 0.5 * phase, -0.3)).translated((0.5 - 2.0 * phase, 1.0 + phase, 1.0)))
        kids.append(Node.geo(Plane(), m[0]).scaled(30.0).translated((0.0, -2.0, 0.0)))
        return Scene(root=Node.group(kids), lights=lights(), ambient=(0.1, 0.1, 0.1))
    cam = Camera(eye=(0.7, 1.9, 7.5), center=(0.0, 0.2, 0.0))
    a, b = scene_at(0.0), scene_at(0.8)
    r = host.Renderer(host_glue.host_scene(a), H.TRAVERSE_FLAT)
    try:
        for (w, h), samples in (((16, 16), 64), ((48, 32), 1)):
            ref_a = check(host, H, oracle, a, cam, w, h, samples, 9, r=r)
            r.update(host_glue.host_scene(b))
            ref_b = check(host, H, oracle, b, cam, w, h, samples, 9, r=r)
            assert not np.array_equal(ref_a.rgb, ref_b.rgb)
            r.update(host_glue.host_scene(a))
    finally:
        r.close()


def test_the_paths_that_keep_the_per_lane_transform(host, H, oracle):
    """The hierarchical kernel and the counting instantiation do not read the table: images as the oracle's, the counting run's ray counts too."""
    scene = prim_scene("cone")
    cam = Camera(eye=(0.7, 1.9, 7.5), center=(0.0, 0.2, 0.0))
    for (w, h), samples in (((16, 16), 64), ((48, 32), 1)):
        bg = default_background(w, h)
        ref = oracle.render(scene, cam, w, h, samples=samples, seed=4, jitter=oracle.JITTER_RNG, mode=oracle.MODE_HIER)
        r = host.Renderer(host_glue.host_scene(scene), H.TRAVERSE_HIER)
        try:
            rgb, lin, st = r.render(host_glue.cam10(cam), w, h, bg, samples=samples, seed=4, sample_mode=H.SAMPLE_RNG)
        finally:
            r.close()
        assert st["kernel_mode"] == 6 and not st["kernel_variant"] & (H.KERNEL_CHAIN | H.KERNEL_INTERPRETER)
        assert np.array_equal(rgb, ref.rgb), f"hier: {(rgb != ref.rgb).any(axis=2).sum()} pixels differ"
        assert_ulp(lin, ref.linear, 0)
        ref = oracle.render(scene, cam, w, h, samples=samples, seed=4, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
        r = host.Renderer(host_glue.host_scene(scene), H.TRAVERSE_FLAT)
        try:
            rgb, lin, st = r.render(host_glue.cam10(cam), w, h, bg, samples=samples, seed=4, sample_mode=H.SAMPLE_RNG, stats=True)
        finally:
            r.close()
        assert flat_kernel(H, st) and st["kernel_variant"] & H.KERNEL_COUNTING
        assert np.array_equal(rgb, ref.rgb), f"counting: {(rgb != ref.rgb).any(axis=2).sum()} pixels differ"
        assert_ulp(lin, ref.linear, 0)
        for k in ("primary", "shadow", "hits"):
            assert st[k] == ref.stats[k], (k, st[k], ref.stats[k])


def test_big_scene(host, H, oracle, monkeypatch):
    """160 x 90 x 64, seed 3, with the occluder table and with PORTRAYER_SHADOW_CACHE=0."""
    from example_scenes import EXAMPLES
    from scene_dsl import ASSETS
    sc = host.Scene.example("big-scene", assets=ASSETS)
    w, h = 160, 90
    ref = oracle.render(oracle.pack_arrays(sc.export()), EXAMPLES["big-scene"]()[1], w, h, samples=64, seed=3, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    try:
        for cache in (None, "0"):
            if cache is None:
                monkeypatch.delenv("PORTRAYER_SHADOW_CACHE", raising=False)
            else:
                monkeypatch.setenv("PORTRAYER_SHADOW_CACHE", cache)
            rgb, lin, st = r.render(sc.camera, w, h, default_background(w, h), samples=64, seed=3, sample_mode=H.SAMPLE_RNG)
            assert flat_kernel(H, st), st
            assert np.array_equal(rgb, ref.rgb), f"cache {cache}: {(rgb != ref.rgb).any(axis=2).sum()} pixels differ"
            assert_ulp(lin, ref.linear, 0)
    finally:
        monkeypatch.delenv("PORTRAYER_SHADOW_CACHE", raising=False)
        r.close()
