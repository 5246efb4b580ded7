"""The primary-visibility pass (pt_aov / pt_aov_device / Renderer.aov) against the oracle, bit for bit.

For every pixel (x, y) the oracle traces Camera::ray_at(x + off_x, y + off_y) (po_camera_rays -> po_cast_rays) in the traversal the scene
was uploaded with; depth, position, node and (normalised in the order DESIGN section 2 pins) normal must carry the same bits. There is no
tolerance in this file: every quantity comes from expressions the render path already evaluates bit-identically to the oracle."""
import ctypes as C
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_glue  # noqa: E402
from scene_dsl import ASSETS, Camera, Light, Material, Mesh, MeshData, Node, Scene, Triangle, default_background  # noqa: E402

pytestmark = pytest.mark.gpu

W, HT = 203, 117  # a multiple of 8 in neither direction
MESH_TYPES = (2, 3)  # PT_PRIM_MESH, PT_PRIM_KDMESH
ALL = ("depth", "position", "normal", "node", "sub", "material")


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def modes(H, O):
    return (("flat", H.TRAVERSE_FLAT, O.MODE_FLAT), ("kd", H.TRAVERSE_KD, O.MODE_KD), ("hier", H.TRAVERSE_HIER, O.MODE_HIER))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def oracle_aov(O, ps, cam, w, h, mode, kd_depth, offset=(0.5, 0.5), rect=None, workers=16):
    """The oracle's answer for every pixel of rect (default: the image), as (h, w[, 3]) arrays: t, id, point, the world normal normalised
    as material.rs:123-125 does it (s = (x*x + y*y) + z*z, each component / sqrt(s)). Rows of rays side by side on the host's cores."""
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, w - 1, h - 1)
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    xy = np.stack([xs.ravel() + offset[0], ys.ravel() + offset[1]], axis=1).astype(np.float64)
    o, d = O.camera_rays(cam, w, h, xy)
    parts = [p for p in np.array_split(np.arange(len(o)), workers) if len(p)]
    with ThreadPoolExecutor(max_workers=workers) as ex:
        res = list(ex.map(lambda p: O.cast_rays(ps, o[p], d[p], mode=mode, kd_depth=kd_depth), parts))
    t, ids, pt, nr = (np.concatenate([r[k] for r in res]) for k in range(4))
    hit = ids >= 0
    with np.errstate(all="ignore"):
        s = (nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1]) + nr[:, 2] * nr[:, 2]
        n = nr / np.sqrt(s)[:, None]
    n[~hit] = 0.0
    shape = (y1 - y0 + 1, x1 - x0 + 1)
    return dict(t=t.reshape(shape), id=ids.reshape(shape), point=pt.reshape(shape + (3,)), normal=n.reshape(shape + (3,)))


def compare(tag, got, ref, flat, hier, flat_node=None):
    """got: Renderer.aov's arrays; ref: oracle_aov's; flat: the oracle's flattened scene (prim_type / prim_data / material per node)."""
    hit = ref["id"] >= 0
    for name, figure in (("depth", int((bits(got["depth"]) != bits(ref["t"])).sum())),
                         ("position", int((bits(got["position"])[hit] != bits(ref["point"])[hit]).any(axis=-1).sum())),
                         ("normal", int((bits(got["normal"])[hit] != bits(ref["normal"])[hit]).any(axis=-1).sum()))):
        print(f"{tag}: {name}: {figure} of {hit.size} pixels differ ({int(hit.sum())} hits)")
    assert np.array_equal(np.isfinite(got["depth"]), hit), f"{tag}: (depth < inf) != (id >= 0)"
    assert np.array_equal(bits(got["depth"]), bits(ref["t"])), f"{tag}: depth differs from the oracle's t"
    assert np.all(np.isposinf(got["depth"][~hit]))
    assert np.array_equal(got["node"] >= 0, hit), f"{tag}: node >= 0 where the oracle hits nothing, or the reverse"
    assert np.all(got["node"][~hit] == -1) and np.all(got["sub"][~hit] == -1) and np.all(got["material"][~hit] == -1)
    if not hier:
        assert np.array_equal(got["node"], ref["id"]), f"{tag}: node differs from the oracle's id"
    if flat_node is not None:
        assert np.array_equal(got["node"], flat_node), f"{tag}: node differs from the flat_scene run's"
    assert np.array_equal(bits(got["position"])[hit], bits(ref["point"])[hit]), f"{tag}: position differs"
    assert np.array_equal(bits(got["normal"])[hit], bits(ref["normal"])[hit]), f"{tag}: normal differs"
    assert not bits(got["position"])[~hit].any() and not bits(got["normal"])[~hit].any(), f"{tag}: misses must hold +0"
    node = got["node"][hit]
    assert np.array_equal(got["material"][hit], flat["material_expected"][node]), f"{tag}: material"
    sub, meshy = got["sub"][hit], np.isin(flat["prim_type"][node], MESH_TYPES)
    assert np.all(sub[~meshy] == 0), f"{tag}: sub must be 0 on hits of anything but a mesh"
    if meshy.any():
        tri_off = flat["_mesh_tri_off"]
        m = flat["prim_data"][node][meshy]
        assert np.all(sub[meshy] >= 0) and np.all(sub[meshy].astype(np.int64) < (tri_off[m + 1] - tri_off[m]).astype(np.int64)), f"{tag}: sub outside its mesh"


def first_use_order(material):
    """The host layer's numbering of the oracle's material indices. `material` is an index into the table the caller uploaded (pt_scene.materials). The
    oracle's table (Scene.export) lists a scene's materials in the order of the scene graph; the host layer's Renderer - like Scene.flatten() - lists them
    in the order the FLATTENED nodes first use them. Same materials, same nodes: the oracle's index of node i, renumbered by first use over i = 0, 1, ..,
    is the index the Renderer uploaded for it. (Where the oracle's own arrays are uploaded through the C ABI the indices are the oracle's as they are:
    test_material_is_the_uploaded_index_through_the_c_abi.)"""
    seen = {}
    return np.array([seen.setdefault(int(m), len(seen)) for m in material], dtype=np.int32)


def packed_tri_off(a):
    return np.asarray(a["mesh_tri_off"], dtype=np.int64)


def run_scene(O, H, host, tag, hs, ps, tri_off, cam, kd_depth, same_in_hier=False, offset=(0.5, 0.5), which=("flat", "kd", "hier")):
    flat = O.flatten(ps)
    flat["_mesh_tri_off"] = tri_off
    flat["material_expected"] = first_use_order(flat["material"])
    assert np.array_equal(flat["material_expected"], hs.flatten()["material"]), "Scene.flatten() numbers materials by first use"
    flat_node = None
    for name, tr, om in modes(H, O):
        if name not in which:
            continue
        r = host.Renderer(hs, tr, kd_depth=kd_depth)
        got = r.aov(cam, W, HT, offset=offset)
        r.close()
        ref = oracle_aov(O, ps, cam, W, HT, om, kd_depth, offset)
        compare(f"{tag} {name}", got, ref, flat, hier=name == "hier", flat_node=flat_node if (name == "hier" and same_in_hier) else None)
        if name == "flat":
            flat_node = got["node"]


EXAMPLE_SCENES = ["primitives", "hier", "instance", "simple-cows", "smooth-shading", "robot-alarm-clock", "big-scene", "soft-shadows", "glossy-reflection"]


@pytest.mark.parametrize("name", EXAMPLE_SCENES)
def test_example_scene_matches_the_oracle_in_every_traversal(oracle, host, H, name):
    sc = host.Scene.example(name, assets=ASSETS)
    a = sc.export()
    ps = oracle.pack_arrays(a)
    # soft-shadows and glossy-reflection have no transformed groups: hierarchical and flat_scene agree bit for bit there
    run_scene(oracle, H, host, name, sc, ps, packed_tri_off(a), sc.camera, 10, same_in_hier=name in ("soft-shadows", "glossy-reflection"))


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("kind", ["random", "extreme"])
def test_generated_scene_matches_the_oracle_in_every_traversal(oracle, host, H, kind, seed):
    from fuzz_gpu_parity import extreme_scene
    from test_gpu_render_parity import random_scene
    scene, cam = (random_scene if kind == "random" else extreme_scene)(seed)
    ps = oracle.pack(scene)
    run_scene(oracle, H, host, f"{kind} {seed}", host_glue.host_scene(scene), ps, packed_tri_off(ps.arrays), host_glue.cam10(cam), 8)


@pytest.mark.parametrize("name", ["primitives", "simple-cows"])
def test_offset_other_than_the_pixel_centre(oracle, host, H, name):
    sc = host.Scene.example(name, assets=ASSETS)
    a = sc.export()
    run_scene(oracle, H, host, name + " offset", sc, oracle.pack_arrays(a), packed_tri_off(a), sc.camera, 10, offset=(0.25, 0.8125))



def test_slices_leave_everything_outside_untouched(oracle, host, H):
    sc = host.Scene.example("primitives", assets=ASSETS)
    for tr in (H.TRAVERSE_FLAT, H.TRAVERSE_KD, H.TRAVERSE_HIER):
        r = host.Renderer(sc, tr)
        full = r.aov(sc.camera, W, HT)
        rect = (13, 9, 150, 101)  # no corner on a tile boundary
        into = {k: np.full((HT, W) + ((3,) if n == 3 else ()), -7 if dt is np.int32 else -7.25, dtype=dt) for k, (dt, n) in H.AOV_BUFFERS.items()}
        sentinel = {k: v.copy() for k, v in into.items()}
        part = r.aov(sc.camera, W, HT, rect=rect, into=into)
        inside = np.zeros((HT, W), dtype=bool)
        inside[rect[1]:rect[3] + 1, rect[0]:rect[2] + 1] = True
        for k in ALL:
            assert part[k][inside].tobytes() == full[k][inside].tobytes(), f"{k}: inside the slice != the full frame"
            assert part[k][~inside].tobytes() == sentinel[k][~inside].tobytes(), f"{k}: a pixel outside the slice was written"
        one = r.aov(sc.camera, W, HT, rect=(101, 58, 101, 58))  # picking one pixel
        for k in ALL:
            assert one[k][58, 101].tobytes() == full[k][58, 101].tobytes(), k
            rest = np.ones((HT, W), dtype=bool); rest[58, 101] = False
            assert not np.frombuffer(one[k][rest].tobytes(), dtype=np.uint8).any(), f"{k}: the 1 x 1 slice wrote elsewhere"
        r.close()


def test_argument_errors(host, H):
    lib = H.lib()
    sc = host.Scene.example("primitives", assets=ASSETS)
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    ctx = r.context
    cam = host.camera(sc.camera, W, HT)
    depth = np.zeros((HT, W))
    b = H.PtAovBuffers(depth=depth.ctypes.data_as(H._dp))
    good = H.PtAovParams(W, HT, H.PtRect(0, 0, W - 1, HT - 1), (C.c_double * 2)(0.5, 0.5))
    assert lib.pt_aov(ctx, C.byref(cam), C.byref(good), C.byref(b), None) == H.OK
    for rect in ((0, 0, W, HT - 1), (0, 0, W - 1, HT), (W, 0, W - 1, HT - 1), (0, HT, W - 1, HT - 1)):
        p = H.PtAovParams(W, HT, H.PtRect(*rect), (C.c_double * 2)(0.5, 0.5))
        assert lib.pt_aov(ctx, C.byref(cam), C.byref(p), C.byref(b), None) == H.ERR_SLICE, rect
        assert lib.pt_aov_device(ctx, C.byref(cam), C.byref(p), C.byref(b), None) == H.ERR_SLICE, rect
    with pytest.raises(host.PortrayerPanic):
        r.aov(sc.camera, W, HT, rect=(0, 0, W, HT - 1))
    assert lib.pt_aov(ctx, C.byref(cam), None, C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_aov(ctx, None, C.byref(good), C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_aov(ctx, C.byref(cam), C.byref(good), C.byref(H.PtAovBuffers()), None) == H.ERR_ARGUMENT
    assert lib.pt_aov(ctx, C.byref(cam), C.byref(good), None, None) == H.ERR_ARGUMENT
    for off in ((float("nan"), 0.5), (0.5, float("inf"))):
        p = H.PtAovParams(W, HT, H.PtRect(0, 0, W - 1, HT - 1), (C.c_double * 2)(*off))
        assert lib.pt_aov(ctx, C.byref(cam), C.byref(p), C.byref(b), None) == H.ERR_ARGUMENT, off
    assert lib.pt_aov_finish(ctx, None) == H.ERR_ARGUMENT  # nothing in flight
    bare = H.Context()
    assert lib.pt_aov(bare.handle, C.byref(cam), C.byref(good), C.byref(b), None) == H.ERR_NO_SCENE
    assert lib.pt_aov_device(bare.handle, C.byref(cam), C.byref(good), C.byref(b), None) == H.ERR_NO_SCENE
    bare.close()
    empty = H.PtAovParams(W, HT, H.PtRect(5, 5, 4, 4), (C.c_double * 2)(0.5, 0.5))  # an inverted slice traces nothing (render.rs:60-65)
    depth[:] = 3.0
    assert lib.pt_aov(ctx, C.byref(cam), C.byref(empty), C.byref(b), None) == H.OK and np.all(depth == 3.0)
    r.close()


@pytest.mark.parametrize("name,traverse", [("primitives", "hier"), ("simple-cows", "flat"), ("robot-alarm-clock", "kd")])
def test_every_single_buffer_request_equals_the_all_buffers_request(host, H, name, traverse):
    sc = host.Scene.example(name, assets=ASSETS)
    r = host.Renderer(sc, {"flat": H.TRAVERSE_FLAT, "kd": H.TRAVERSE_KD, "hier": H.TRAVERSE_HIER}[traverse])
    full = r.aov(sc.camera, W, HT)
    for k in ALL:
        one = r.aov(sc.camera, W, HT, want=(k,))
        assert set(one) == {k, "kernel_ms"}
        assert one[k].tobytes() == full[k].tobytes(), k
    two = r.aov(sc.camera, W, HT, want=("depth", "node"))
    assert two["depth"].tobytes() == full["depth"].tobytes() and two["node"].tobytes() == full["node"].tobytes()
    r.close()


def mesh_and_triangle_scenes(obj):
    """Scene A: one Mesh of `obj` under a transform; scene B: the same triangles as stand-alone Triangle primitives, in mesh order, under the same transform."""
    md = MeshData.load_obj(os.path.join(ASSETS, obj))
    mat = Material(diffuse=(0.7, 0.4, 0.2), specular=(0.3, 0.3, 0.3), shininess=10.0)
    lights = [Light(position=(4.0, 6.0, 8.0), color=(0.9, 0.9, 0.9))]

    def place(n):
        return n.scaled((1.3, 0.8, 1.1)).rotated_xzy((0.4, -0.7, 1.1)).translated((0.3, -0.2, 0.1))
    a = Scene(root=Node.group([place(Node.geo(Mesh(md), mat))]), lights=lights, ambient=(0.2, 0.2, 0.2))
    tris = [Node.geo(Triangle(*(md.positions[i] for i in t)), mat) for t in md.triangles]
    b = Scene(root=Node.group([place(Node.group(tris))]), lights=lights, ambient=(0.2, 0.2, 0.2))
    return a, b, len(md.triangles)


SUB_CAMERAS = {"buckyball.obj": Camera(eye=(0.5, 1.0, 9.0), center=(0.2, 0.0, 0.0), fovy_degrees=40.0),
               "plane.obj": Camera(eye=(0.5, 3.0, 6.0), center=(0.3, -0.2, 0.1), fovy_degrees=12.0)}


@pytest.mark.parametrize("obj", ["buckyball.obj", "plane.obj"])
def test_sub_is_the_triangle_inside_the_mesh(oracle, host, H, obj):
    a, b, n_tris = mesh_and_triangle_scenes(obj)
    cam = SUB_CAMERAS[obj]
    pa, pb = oracle.pack(a), oracle.pack(b)
    ra = oracle_aov(oracle, pa, cam, W, HT, oracle.MODE_FLAT, -1)
    rb = oracle_aov(oracle, pb, cam, W, HT, oracle.MODE_FLAT, -1)
    # the precondition, no pixel excluded: the mesh behind its bounding-box test (mesh.rs:152) and the bare triangles agree on every t
    assert np.array_equal(bits(ra["t"]), bits(rb["t"])), "the input does not meet the precondition: choose another mesh / transform / camera"
    hit = rb["id"] >= 0
    assert hit.sum() > 500 and len(np.unique(rb["id"][hit])) >= min(n_tris, 20), "the camera must see the mesh"
    fb = oracle.flatten(pb)
    first = int(np.flatnonzero(fb["prim_type"] == 1)[0])  # PT_PRIM_TRIANGLE: the triangles follow their groups in breadth-first order, in mesh order
    assert np.array_equal(np.flatnonzero(fb["prim_type"] == 1), np.arange(first, first + n_tris))
    for tr in (H.TRAVERSE_FLAT, H.TRAVERSE_KD, H.TRAVERSE_HIER):
        r = host.Renderer(host_glue.host_scene(a), tr)
        got = r.aov(host_glue.cam10(cam), W, HT, want=("depth", "sub", "node"))
        r.close()
        if tr == H.TRAVERSE_FLAT:
            assert np.array_equal(bits(got["depth"]), bits(ra["t"]))
        if tr != H.TRAVERSE_KD:  # (the kdtree semantics may lose hits at cell borders, DESIGN: compare where they see the mesh)
            assert np.array_equal(got["node"] >= 0, hit)
        seen = got["node"] >= 0
        assert np.array_equal(got["sub"][seen], (rb["id"] - first)[seen]), "sub != the triangle the linear scan over bare triangles finds"
        assert np.all(got["sub"][~seen] == -1)


@pytest.mark.parametrize("which", ["example:primitives-simple", "example:entering-the-mirror-dimension", "example:macho-cows", "random:2", "random:7", "extreme:3"])
@pytest.mark.parametrize("traverse", ["flat", "kd", "hier"])
def test_material_is_the_uploaded_index_through_the_c_abi(oracle, H, which, traverse):
    """pt_scene built from the oracle's own flattened arrays (device_glue.DeviceScene): material == O.flatten(scene)["material"][node], as it stands."""
    import device_glue
    from example_scenes import EXAMPLES
    from fuzz_gpu_parity import extreme_scene
    from test_gpu_render_parity import random_scene
    kind, arg = which.split(":")
    scene, cam = EXAMPLES[arg]()[:2] if kind == "example" else (random_scene if kind == "random" else extreme_scene)(int(arg))
    ds = device_glue.DeviceScene(scene, {"flat": H.TRAVERSE_FLAT, "kd": H.TRAVERSE_KD, "hier": H.TRAVERSE_HIER}[traverse], kd_depth=8)
    if traverse == "hier":  # the scene graph beside the oracle's flattened arrays (same nodes, same breadth-first order): the host library's, as a binding would pass it
        g = host_glue.host_scene(scene).graph()
        keep = ds.keep
        keep["g_tr"], keep["g_inv"], keep["g_nrm"] = (np.ascontiguousarray(g[k].reshape(-1, 16)) for k in ("trans", "invtrans", "normal_trans"))
        keep["g_off"], keep["g_rank"] = np.ascontiguousarray(g["chain_off"]), np.ascontiguousarray(g["dfs_rank"])
        keep["g_chain"] = np.ascontiguousarray(np.concatenate([g["chain"], np.zeros(1, dtype=np.uint32)]))
        assert len(keep["g_off"]) == ds.struct.n_nodes + 1
        st = ds.struct
        st.n_graph_nodes = len(keep["g_tr"])
        st.graph_trans, st.graph_invtrans, st.graph_normal_trans = (keep[k].ctypes.data_as(H._dp) for k in ("g_tr", "g_inv", "g_nrm"))
        st.node_chain_off, st.node_chain, st.node_dfs_rank = (keep[k].ctypes.data_as(H._up) for k in ("g_off", "g_chain", "g_rank"))
    ctx = H.Context()
    ds.upload(ctx)
    camera = device_glue.camera_struct(cam, W, HT)
    out = {k: np.zeros((HT, W) + ((3,) if n == 3 else ()), dtype=dt) for k, (dt, n) in H.AOV_BUFFERS.items()}
    b = H.PtAovBuffers(**{k: out[k].ctypes.data_as(H._dp if dt is np.float64 else H._ip) for k, (dt, _) in H.AOV_BUFFERS.items()})
    p = H.PtAovParams(W, HT, H.PtRect(0, 0, W - 1, HT - 1), (C.c_double * 2)(0.5, 0.5))
    ctx.check(H.lib().pt_aov(ctx.handle, C.byref(camera), C.byref(p), C.byref(b), None), "pt_aov")
    ctx.close()
    flat = dict(ds.flat)
    flat["_mesh_tri_off"] = packed_tri_off(ds.ps.arrays)
    flat["material_expected"] = flat["material"]
    ref = oracle_aov(oracle, ds.ps, cam, W, HT, {"flat": oracle.MODE_FLAT, "kd": oracle.MODE_KD, "hier": oracle.MODE_HIER}[traverse], 8)
    compare(f"{which} {traverse} (C ABI)", out, ref, flat, hier=traverse == "hier")


def test_device_buffers_on_a_stream_equal_the_host_path(H):
    """pt_aov_device into torch tensors on a stream of torch's, in a process of its own in which torch initialises its GPU side first (as in
    test_gpu_multirank.test_node_rccl_leg_inside_a_process_that_carries_torch)."""
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
W, HT = 203, 117
lib = H.lib()
sc = host.Scene.example("simple-cows", assets=ASSETS)
r = host.Renderer(sc, H.TRAVERSE_FLAT)
ref = r.aov(sc.camera, W, HT)
assert (ref["node"] >= 0).sum() > 1000
cam = host.camera(sc.camera, W, HT)
p = H.PtAovParams(W, HT, H.PtRect(0, 0, W - 1, HT - 1), (C.c_double * 2)(0.5, 0.5))
t = {k: torch.full((HT, W) + ((3,) if n == 3 else ()), -5, dtype=torch.float64 if dt is np.float64 else torch.int32, device=dev) for k, (dt, n) in H.AOV_BUFFERS.items()}
torch.cuda.synchronize()
stream = torch.cuda.Stream(device=dev)
assert stream.cuda_stream != 0
b = H.PtAovBuffers()
for k, (dt, _) in H.AOV_BUFFERS.items():
    setattr(b, k, C.cast(C.c_void_p(t[k].data_ptr()), H._dp if dt is np.float64 else H._ip))
assert lib.pt_aov_device(r.context, C.byref(cam), C.byref(p), C.byref(b), C.c_void_p(stream.cuda_stream)) == H.OK, lib.pt_last_error(r.context)
assert lib.pt_aov_device(r.context, C.byref(cam), C.byref(p), C.byref(b), C.c_void_p(stream.cuda_stream)) == H.ERR_ARGUMENT  # one pass in flight per context
ms = C.c_double(-1.0)
assert lib.pt_aov_finish(r.context, C.byref(ms)) == H.OK and ms.value > 0.0
stream.synchronize()
for k in H.AOV_BUFFERS:
    assert t[k].cpu().numpy().tobytes() == ref[k].tobytes(), k
r.close()
assert (x * 2).sum().item() == 2048.0
print("aov into torch tensors ok")
""" % (root, root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "aov into torch tensors ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_renders_around_and_in_flight_across_a_pass_are_unchanged(oracle, host, H):
    import device_glue
    from example_scenes import EXAMPLES
    w, h, samples = 160, 96, 4
    bg = default_background(w, h)
    sc = host.Scene.example("macho-cows", assets=ASSETS)
    r1, r2 = host.Renderer(sc, H.TRAVERSE_FLAT), host.Renderer(sc, H.TRAVERSE_FLAT)
    a1 = r1.render(sc.camera, w, h, bg, samples=samples, seed=3, sample_mode=H.SAMPLE_RNG)
    r1.aov(sc.camera, W, HT)
    b1 = r1.render(sc.camera, w, h, bg, samples=samples, seed=4, sample_mode=H.SAMPLE_RNG)
    a2 = r2.render(sc.camera, w, h, bg, samples=samples, seed=3, sample_mode=H.SAMPLE_RNG)
    b2 = r2.render(sc.camera, w, h, bg, samples=samples, seed=4, sample_mode=H.SAMPLE_RNG)  # this renderer never ran a pass
    for (x, y) in ((a1, a2), (b1, b2)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(bits(x[1]), bits(y[1]))
    r1.close(); r2.close()

    # pt_render_device x 2 in flight, a pass, pt_render_finish x 2: the oracle's images
    scene, cam0, _ = EXAMPLES["macho-cows"]()
    ds = device_glue.DeviceScene(scene, H.TRAVERSE_FLAT)
    lib = H.lib()
    ctx = H.Context()
    ds.upload(ctx)
    c = ctx.handle
    d_bg = C.c_void_p()
    assert lib.pt_device_alloc(c, bg.nbytes, C.byref(d_bg)) == 0 and lib.pt_copy_to_device(c, d_bg, bg.ctypes.data_as(C.c_void_p), bg.nbytes) == 0
    d_img = [C.c_void_p(), C.c_void_p()]
    camera = device_glue.camera_struct(cam0, w, h)
    for k in range(2):
        assert lib.pt_device_alloc(c, w * h * 3, C.byref(d_img[k])) == 0
        p = H.PtRenderParams(w, h, H.PtRect(0, 0, w - 1, h - 1), samples, 10 + k, H.SAMPLE_RNG, 1, 0, 1, 0)
        assert lib.pt_render_device(c, C.byref(camera), d_bg, C.byref(p), 0, d_img[k], C.c_void_p(lib.pt_context_stream(c, k))) == 0, lib.pt_last_error(c)
    depth, node = np.zeros((h, w)), np.zeros((h, w), dtype=np.int32)
    b = H.PtAovBuffers(depth=depth.ctypes.data_as(H._dp), node=node.ctypes.data_as(H._ip))
    ap = H.PtAovParams(w, h, H.PtRect(0, 0, w - 1, h - 1), (C.c_double * 2)(0.5, 0.5))
    assert lib.pt_aov(c, C.byref(camera), C.byref(ap), C.byref(b), None) == H.OK, lib.pt_last_error(c)
    ps = oracle.pack(scene)
    ref = oracle_aov(oracle, ps, cam0, w, h, oracle.MODE_FLAT, -1)
    assert np.array_equal(bits(depth), bits(ref["t"])) and np.array_equal(node, ref["id"])
    st = H.PtStats()
    for k in range(2):
        assert lib.pt_render_finish(c, C.byref(st)) == 0, lib.pt_last_error(c)
        img = np.zeros((h, w, 3), dtype=np.uint8)
        assert lib.pt_copy_from_device(c, img.ctypes.data_as(C.c_void_p), d_img[k], img.nbytes) == 0
        want = oracle.render(ps, cam0, w, h, samples=samples, seed=10 + k, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
        assert np.array_equal(img, want.rgb), f"frame {k} in flight across the pass differs from the oracle"
    for d in d_img + [d_bg]:
        lib.pt_device_free(c, d)
    ctx.close()


def cast_one_ray(H, oracle, ctx, cam, w, h):
    """pt_test_cast_rays' return code for the ray of the image's centre."""
    o, d = oracle.camera_rays(cam, w, h, [[w / 2 + 0.5, h / 2 + 0.5]])
    t1, n1, s1 = np.zeros(1), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    return H.lib().pt_test_cast_rays(ctx, 1, o.ctypes.data_as(H._dp), d.ctypes.data_as(H._dp), 0, t1.ctypes.data_as(H._dp), n1.ctypes.data_as(H._ip), s1.ctypes.data_as(H._ip))


def test_the_device_built_tree_of_a_million_triangles(oracle, host, H):
    """The synthetic big-soup (1.25 M triangles in one mesh, its tree built on the device) at a small image size: depth and node agree with the oracle on
    EVERY pixel of the frame (one ray per pixel: the oracle's scan over the mesh's triangles, mesh.rs:157-166, takes a few seconds for the 960 rays).
    Measured: pt_test_cast_rays does NOT refuse this scene - the stack its trees can need fits the 160 KB of LDS -, so the refusal the pass must not
    inherit is provoked in test_a_stack_deeper_than_lds_is_walked_not_refused below."""
    w, h = 40, 24
    sc = host.Scene.example("synthetic:big-soup", n=6, assets=ASSETS)
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    got = r.aov(sc.camera, w, h, want=("depth", "node"))
    r.close()
    ref = oracle_aov(oracle, oracle.pack_arrays(sc.export()), sc.camera, w, h, oracle.MODE_FLAT, -1)
    hit = ref["id"] >= 0
    print(f"big-soup: depth: {int((bits(got['depth']) != bits(ref['t'])).sum())} of {hit.size} pixels differ, node: {int((got['node'] != ref['id']).sum())} ({int(hit.sum())} hits)")
    assert hit.sum() > 100, "the camera must see the soup"
    assert np.array_equal(bits(got["depth"]), bits(ref["t"])), "depth differs from the oracle's t"
    assert np.array_equal(got["node"], ref["id"]), "node differs from the oracle's id"


@pytest.mark.parametrize("mode", ["flat", "kd", "hier"])
def test_a_stack_deeper_than_lds_is_walked_not_refused(oracle, host, H, monkeypatch, mode):
    """PORTRAYER_STACK_CAP=450 declares trees with up to 450 pending entries for a small scene with Mesh and KDMesh instances (as
    test_gpu_render_parity.test_deep_trees_take_lds_rows_from_the_lanes_not_the_render does): 450 KB of stack per block, which pt_test_cast_rays - the whole
    stack in LDS - refuses with PT_ERR_SCENE ("tree too deep for it"). The pass gives the wavefronts the rows they need and continues the lanes' stacks in HBM:
    it completes, changes no bit against the run without the declaration, and agrees with the oracle."""
    from test_gpu_render_parity import random_scene
    scene, cam = random_scene(3)
    tr, om = {"flat": (H.TRAVERSE_FLAT, oracle.MODE_FLAT), "kd": (H.TRAVERSE_KD, oracle.MODE_KD), "hier": (H.TRAVERSE_HIER, oracle.MODE_HIER)}[mode]
    out = []
    for cap in (None, "450"):
        if cap:
            monkeypatch.setenv("PORTRAYER_STACK_CAP", cap)
        r = host.Renderer(host_glue.host_scene(scene), tr, kd_depth=8)
        rc = cast_one_ray(H, oracle, r.context, host_glue.cam10(cam), W, HT)
        if cap:
            assert rc == H.ERR_SCENE and b"too deep" in H.lib().pt_last_error(r.context), (rc, H.lib().pt_last_error(r.context))
        else:
            assert rc == H.OK
        out.append(r.aov(host_glue.cam10(cam), W, HT))
        r.close()
    for k in ALL:
        assert out[0][k].tobytes() == out[1][k].tobytes(), k
    ref = oracle_aov(oracle, oracle.pack(scene), cam, W, HT, om, 8)
    assert (ref["id"] >= 0).sum() > 1000
    assert np.array_equal(bits(out[1]["depth"]), bits(ref["t"])) and np.array_equal(out[1]["node"] >= 0, ref["id"] >= 0)
    if mode != "hier":
        assert np.array_equal(out[1]["node"], ref["id"])


@pytest.mark.parametrize("name,mode", [("macho-cows", "flat"), ("macho-cows", "kd"), ("robot-alarm-clock", "hier"), ("big-scene", "kd"), ("big-scene", "flat")])
def test_traversal_stack_beyond_lds_gives_the_same_buffers(host, H, monkeypatch, name, mode):
    """PORTRAYER_LDS_STACK=1 keeps one entry of a lane's stack in LDS, the rest in its HBM column (PtStackSpill), as for a render: nothing may change."""
    sc = host.Scene.example(name, assets=ASSETS)
    tr = {"flat": H.TRAVERSE_FLAT, "kd": H.TRAVERSE_KD, "hier": H.TRAVERSE_HIER}[mode]
    out = []
    for lds in (None, "1"):
        if lds:
            monkeypatch.setenv("PORTRAYER_LDS_STACK", lds)
        r = host.Renderer(sc, tr)
        out.append(r.aov(sc.camera, W, HT))
        r.close()
    assert (out[0]["node"] >= 0).sum() > 1000
    for k in ALL:
        assert out[0][k].tobytes() == out[1][k].tobytes(), k


_OVERFLOW = r"""
import sys
sys.path.insert(0, %r)
from portrayer_amd import _hip as H
from portrayer_amd import host
sc = host.Scene.example("big-scene")
r = host.Renderer(sc, H.TRAVERSE_FLAT)
try:
    r.aov(sc.camera, 203, 117)
    print("NO ERROR")
except host.PortrayerHostError as e:
    print("ERR", e)
"""


def test_stack_overflow_is_an_error_not_a_wrong_answer():
    """PORTRAYER_STACK_CAP=2 makes the walk of a 1000-node scene run out of stack: the pass must fail with PT_ERR_TRAVERSAL, as a render does
    (test_gpu_multirank.test_stack_overflow_is_reported_without_the_counting_build)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", _OVERFLOW % root], env=dict(os.environ, PORTRAYER_STACK_CAP="2"), capture_output=True, text=True, timeout=300)
    assert "ERR" in out.stdout and "overflow" in out.stdout and "NO ERROR" not in out.stdout, out.stdout + out.stderr
