"""pt_chart / Renderer.chart / ao_chart / gather_chart on the GPU: the chart equals the numpy restatement of the contract
(tests/chart_restate.py) in every bit of position, normal, tri and covered, in flat, hierarchical and k-d traversal; it reads the vertices and matrices that are
RESIDENT (after deform, deform_device and update: the new ones); ao_chart and gather_chart equal ao and gather fed with the chart's arrays; the owner does
not depend on the schedule; and the device form keeps the pass protocol.

The cross-check against the ray queries (a pass pinned to the oracle): for texels well inside their triangle, the ray from P + h N along -N hits the chart's
node and triangle within TOL of P. TOL is not fitted to the kernel: on these rays the ORACLE's hit point (po_cast_rays, the reference's arithmetic) deviates
from P by at most 4.44e-16 on the cube's 1,884 rays and 4.44e-16 on the grid's 2,465 (h = 0.5, 67 x 37), measured on the CPU by
profiles/chart/measure.py --oracle; with the project's factor of 64: 2.84e-14."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # (before the product's library is loaded: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import chart_restate as R  # noqa: E402
import host_glue  # noqa: E402
from example_scenes import load_mesh, soft_shadows, transmission_refraction  # noqa: E402
from scene_dsl import Cube, KDMesh, Light, Material, Mesh, MeshData, Node, Scene, Sphere  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ["flat", "hier", "kd"]
SIZES = [(1, 1), (7, 5), (64, 64), (67, 37)]
ORACLE_DEVIATION = 4.44e-16   # the oracle's hit point against P on the cross-check's rays (see above)
TOL = 64 * ORACLE_DEVIATION
LIFT = 0.5                    # h of the cross-check's rays
RED = Material(diffuse=(0.8, 0.25, 0.2), specular=(0.5, 0.5, 0.5), shininess=40.0)
GREY = Material(diffuse=(0.6, 0.6, 0.6))
CASES = R.cases()


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def traverse_of(H, mode):
    return {"flat": H.TRAVERSE_FLAT, "hier": H.TRAVERSE_HIER, "kd": H.TRAVERSE_KD}[mode]


def corner_mesh(tri_v, tri_n):
    """a mesh with three vertices of its own per triangle: the case's records are the mesh's"""
    t = len(tri_v)
    return MeshData(np.ascontiguousarray(tri_v.reshape(3 * t, 3)), np.arange(3 * t, dtype=np.uint32).reshape(t, 3), np.ascontiguousarray(tri_n.reshape(3 * t, 3)), "chart-case")


def cube_mesh():
    """12 triangles, 24 vertices (a face's four are its own, with the face's normal bent a little so that smooth and flat differ) and six charts: a 3 x 2 atlas
    with a margin, per vertex"""
    pos, nrm, uv, tris = [], [], [], []
    faces = [((1, 0, 0), (0, 1, 0), (0, 0, 1)), ((-1, 0, 0), (0, 0, 1), (0, 1, 0)), ((0, 1, 0), (0, 0, 1), (1, 0, 0)),
             ((0, -1, 0), (1, 0, 0), (0, 0, 1)), ((0, 0, 1), (1, 0, 0), (0, 1, 0)), ((0, 0, -1), (0, 1, 0), (1, 0, 0))]
    for f, (n, a, b) in enumerate(faces):
        n, a, b = np.array(n, float), np.array(a, float), np.array(b, float)
        cx, cy = f % 3, f // 3
        for k, (sa, sb) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):
            pos.append(0.5 * (n + sa * a + sb * b))
            m = n + 0.2 * (sa * a + sb * b)
            nrm.append(m / np.linalg.norm(m))
            uv.append(((cx + 0.06 + 0.88 * (sa + 1) / 2) / 3.0, (cy + 0.07 + 0.86 * (sb + 1) / 2) / 2.0))
        tris += [[4 * f, 4 * f + 1, 4 * f + 2], [4 * f, 4 * f + 2, 4 * f + 3]]
    return MeshData(np.array(pos), np.array(tris, dtype=np.uint32), np.array(nrm), "cube", np.array(uv))


def under_a_group(prims, lights=None):
    """the mesh nodes under a rotated, non-uniformly scaled group, a floor and a ball beside them"""
    group = Node.group(list(prims)).rotated_z(0.4).scaled((1.3, 0.7, 2.0)).rotated_x(-0.3).translated((0.2, -0.1, 0.3))
    floor = Node.geo(Cube(), GREY).scaled((12.0, 0.2, 12.0)).translated((0.0, -2.6, 0.0))
    ball = Node.geo(Sphere(), GREY).scaled(0.4).translated((2.4, 0.2, 0.5))
    return Scene(root=Node.group([group, floor, ball]), lights=lights or [Light(position=(3.0, 4.0, 9.0), color=(0.9, 0.9, 0.9))], ambient=(0.15, 0.15, 0.15))


def mesh_nodes(hs):
    return [int(i) for i in np.nonzero(np.isin(hs.flatten()["prim_type"], (2, 3)))[0]]


def expected(hs, node, mesh, smooth, uv, w, h, flags=0):
    """the restatement on flattened node `node`: its composed matrices as Scene.flatten() gives them, the mesh's records, `uv` per corner or per vertex"""
    fl = hs.flatten()
    fwd, nrm = fl["trans"][node][:3, :4].reshape(12), fl["normal_trans"][node][:3, :3].reshape(9)
    idx = mesh.triangles.astype(np.int64)
    tri_v = mesh.positions[idx].reshape(-1, 9)
    tri_n = mesh.normals[idx].reshape(-1, 9) if smooth else None
    uv = np.asarray(uv)
    uv6 = uv[idx].reshape(-1, 6) if uv.shape == (len(mesh.positions), 2) and uv.shape != (len(idx), 6) else uv.reshape(-1, 6)
    return R.chart(fwd, nrm, tri_v, tri_n, uv6, w, h, flags)


def assert_same(got, want, where):
    for k in ("position", "normal", "tri", "covered"):
        assert R.same_bits(got[k], want[k]), "%s: %s differs at %d texels" % (where, k, int(np.sum(np.any((got[k] != want[k]).reshape(want["tri"].size, -1), axis=1))))


_open = []


def renderer(host, H, key, make, mode):
    """(host scene, renderer) of a scene in a traversal; closed behind the test that asked for it (a context holds streams and events: a module that kept every
    one of its fifty open would leave the device's queues to nobody else in the process)"""
    hs = host_glue.host_scene(make())
    _open.append(host.Renderer(hs, traverse_of(H, mode)))
    return hs, _open[-1]


@pytest.fixture(autouse=True)
def close_renderers():
    yield
    while _open:
        _open.pop().close()


# ---- 1. exactness
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_cpu_cases_equal_the_restatement_in_every_bit(host, H, name, mode):
    v, n, uv, sizes = CASES[name]
    mesh = corner_mesh(v, n)
    for smooth in (False, True):
        hs, r = renderer(host, H, (name, smooth), lambda: under_a_group([Node.geo(Mesh(mesh, smooth), RED)]), mode)
        node = mesh_nodes(hs)[0]
        for (w, h) in sizes:
            for flip in (False, True):
                got = r.chart(node, w, h, uv, flip_normal=flip)
                assert_same(got, expected(hs, node, mesh, smooth, uv, w, h, 1 if flip else 0), "%s %s %dx%d smooth %d flip %d" % (name, mode, w, h, smooth, flip))
                assert got["kernel_ms"] > 0.0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("smooth", [False, True])
def test_a_cube_with_six_charts_under_a_rotated_scaled_group(host, H, mode, smooth):
    mesh = cube_mesh()
    prim = (KDMesh if mode == "kd" else Mesh)(mesh, smooth)
    hs, r = renderer(host, H, ("cube", smooth, mode == "kd"), lambda: under_a_group([Node.geo(prim, RED)]), mode)
    node = mesh_nodes(hs)[0]
    for (w, h) in SIZES:
        want = expected(hs, node, mesh, smooth, mesh.tex_coords, w, h)
        assert_same(r.chart(node, w, h, mesh.tex_coords), want, "cube %s %dx%d" % (mode, w, h))  # per vertex: expanded through the mesh's indices
        assert_same(r.chart(node, w, h, mesh.tex_coords[mesh.triangles.astype(np.int64)]), want, "cube per corner")  # (T, 3, 2)
    want = expected(hs, node, mesh, smooth, mesh.tex_coords, 67, 37)
    assert sorted(np.unique(want["tri"])) == list(range(-1, 12)), "every chart owns texels, and the margins none"
    only = r.chart(node, 67, 37, mesh.tex_coords, want=("tri",))
    assert sorted(only) == ["kernel_ms", "tri"] and R.same_bits(only["tri"], want["tri"])
    into = {"normal": np.full((37, 67, 3), 9.0)}
    assert r.chart(node, 67, 37, mesh.tex_coords, want=("normal",), into=into)["normal"] is into["normal"] and R.same_bits(into["normal"], want["normal"])


def test_the_nodes_mesh_is_the_exports_and_a_node_that_is_no_mesh_is_refused(host, H):
    mesh = cube_mesh()
    hs, r = renderer(host, H, ("cube", False, False), lambda: under_a_group([Node.geo(Mesh(mesh, False), RED)]), "flat")
    node = mesh_nodes(hs)[0]
    ex = hs.export()
    _, n_verts, n_tris, idx = r._chart_node(node)
    assert (n_verts, n_tris) == (24, 12) and np.array_equal(idx, ex["mesh_indices"][:12]) and np.array_equal(idx, mesh.triangles)
    other = [i for i in range(len(hs.flatten()["prim_type"])) if i != node]
    for bad in other + [len(other) + 1, 1 << 20]:
        with pytest.raises(ValueError, match="node"):
            r.chart(bad, 8, 8, mesh.tex_coords)
    with pytest.raises(host.PortrayerHostError, match="uv is NULL"):
        r.chart(node, 8, 8)  # no textured material: the scene keeps no texture coordinates on the device


@pytest.mark.parametrize("mode", MODES)
def test_an_assets_own_coordinates_in_a_textured_scene(host, H, mode):
    """fish.obj as a KDMesh in transmission-refraction: uv=None reads tri_uv, and equals the same coordinates passed explicitly"""
    fish = load_mesh("fish.obj")
    hs, r = renderer(host, H, "tank", lambda: transmission_refraction()[0], mode)
    nodes = [i for i in mesh_nodes(hs) if hs.flatten()["prim_type"][i] == 3]
    assert len(nodes) == 2
    for node in nodes:
        want = expected(hs, node, fish, True, fish.tex_coords, 67, 37)
        cov = int(want["covered"].sum())
        assert 0.1 * 2479 <= cov <= 0.9 * 2479, "the guard on the reference: %d of 2479 texels covered" % cov
        assert_same(r.chart(node, 67, 37), want, "fish, its own coordinates, %s" % mode)
        assert_same(r.chart(node, 67, 37, fish.tex_coords), want, "fish, explicit coordinates, %s" % mode)
    assert not R.same_bits(r.chart(nodes[0], 67, 37)["position"], r.chart(nodes[1], 67, 37)["position"])


@pytest.mark.parametrize("mode", MODES)
def test_an_asset_as_a_mesh_with_explicit_coordinates_instanced_twice(host, H, mode):
    """monkey.obj under two nodes with different transforms: one mesh, two charts"""
    monkey = load_mesh("monkey.obj")
    assert monkey.tex_coords is not None and monkey.normals is not None
    prim = Mesh(monkey, True)
    make = lambda: under_a_group([Node.geo(prim, RED).scaled(0.8).translated((-1.2, 0.0, 0.0)), Node.geo(prim, RED).scaled((0.5, 0.9, 0.7)).rotated_y(1.1).translated((1.3, 0.2, 0.1))])
    hs, r = renderer(host, H, "monkeys", make, mode)
    nodes = mesh_nodes(hs)
    assert len(nodes) == 2
    got = []
    for node in nodes:
        want = expected(hs, node, monkey, True, monkey.tex_coords, 67, 37)
        cov = int(want["covered"].sum())
        assert 0.1 * 2479 <= cov <= 0.9 * 2479, "the guard on the reference: %d of 2479 texels covered" % cov
        got.append(r.chart(node, 67, 37, monkey.tex_coords))
        assert_same(got[-1], want, "monkey node %d %s" % (node, mode))
    assert R.same_bits(got[0]["tri"], got[1]["tri"]) and not R.same_bits(got[0]["position"], got[1]["position"])


def test_one_triangle_whose_box_is_a_whole_256_map(host, H):
    """the split path of the own kernel: the box is 64 tiles, dealt to 16 wavefronts"""
    uv = np.array([[-0.2, 0.05, 1.6, 0.3, 0.3, 1.5]])
    v, n = R._tri_from_uv(uv)
    mesh = corner_mesh(v, n)
    hs, r = renderer(host, H, "big-triangle", lambda: under_a_group([Node.geo(Mesh(mesh, True), RED)]), "flat")
    node = mesh_nodes(hs)[0]
    want = expected(hs, node, mesh, True, uv, 256, 256)
    assert int(want["covered"].sum()) > 0.6 * 65536 and int(want["covered"].sum()) < 65536
    assert_same(r.chart(node, 256, 256, uv), want, "one triangle over 256 x 256")


# ---- 2. the cross-check against the ray queries
@pytest.mark.parametrize("which", ["cube", "grid"])
def test_rays_cast_back_at_the_points_hit_the_charts_node_and_triangle(host, H, which):
    if which == "cube":
        mesh, smooth = cube_mesh(), False
        uv = mesh.tex_coords[mesh.triangles.astype(np.int64)].reshape(-1, 6)
    else:
        v, n, uv, _ = CASES["grid"]
        mesh, smooth = corner_mesh(v, n), False
    hs, r = renderer(host, H, ("cross", which), lambda: under_a_group([Node.geo(Mesh(mesh, smooth), RED)]), "flat")
    node = mesh_nodes(hs)[0]
    got = r.chart(node, 67, 37, uv)
    inside = (R.min_weight_ratio(uv, 67, 37, got["tri"]) >= 2.0 ** -10).ravel()
    assert int(inside.sum()) > 500
    P, N, tri = got["position"].reshape(-1, 3)[inside], got["normal"].reshape(-1, 3)[inside], got["tri"].ravel()[inside]
    hit = r.rays(P + LIFT * N, -N, want=("t", "position", "node", "sub"))
    assert np.array_equal(hit["node"], np.full(len(P), node)) and np.array_equal(hit["sub"], tri)
    dev = float(np.max(np.abs(hit["position"] - P)))
    print("%s: %d rays, largest deviation of the hit point from P %.3g (tolerance %.3g)" % (which, len(P), dev, TOL))
    assert dev <= TOL


# ---- 3. resident data
def _sheet(phase, normals=True):
    n = 6
    xs = np.linspace(-1.0, 1.0, n + 1)
    x, y = np.meshgrid(xs, xs)
    x, y = x.ravel(), y.ravel()
    arg = 2.2 * x + 0.7 * y + phase
    pos = np.stack([x, y, 0.3 * np.sin(arg)], axis=1)
    g = np.stack([-0.66 * np.cos(arg), -0.21 * np.cos(arg), np.ones_like(x)], axis=1)
    idx = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            idx += [[a, a + 1, a + n + 2], [a, a + n + 2, a + n + 1]]
    uv = np.stack([(x + 1.0) / 2.0 * 0.9 + 0.05, (y + 1.0) / 2.0 * 0.8 + 0.1], axis=1)
    return MeshData(pos, np.array(idx, dtype=np.uint32), g / np.linalg.norm(g, axis=1, keepdims=True) if normals else None, "sheet", uv)


@pytest.mark.parametrize("mode", ["flat", "hier"])
def test_after_a_deform_from_the_host_and_from_the_device_the_chart_is_of_the_new_vertices(host, H, mode):
    a, b, c = _sheet(0.0), _sheet(1.3), _sheet(2.1)
    make = lambda m: under_a_group([Node.geo(Mesh(m, True), RED)])
    hs_a, hs_b, hs_c = (host_glue.host_scene(make(m)) for m in (a, b, c))
    r = host.Renderer(hs_a, traverse_of(H, mode))
    node = mesh_nodes(hs_a)[0]
    assert_same(r.chart(node, 67, 37, a.tex_coords), expected(hs_a, node, a, True, a.tex_coords, 67, 37), "before")
    r.deform(hs_b)
    want_b = expected(hs_b, node, b, True, b.tex_coords, 67, 37)
    assert_same(r.chart(node, 67, 37, b.tex_coords), want_b, "after deform")
    assert not R.same_bits(want_b["position"], expected(hs_a, node, a, True, a.tex_coords, 67, 37)["position"])
    dev = torch.device("cuda", 0)
    r.deform_device({0: torch.from_numpy(c.positions).to(dev)}, {0: torch.from_numpy(c.normals).to(dev)})
    assert_same(r.chart(node, 67, 37, c.tex_coords), expected(hs_c, node, c, True, c.tex_coords, 67, 37), "after deform_device")
    r.close()


@pytest.mark.parametrize("mode", MODES)
def test_after_an_update_the_chart_is_of_the_new_matrices(host, H, mode):
    mesh = cube_mesh()
    first = lambda: under_a_group([Node.geo(Mesh(mesh, True), RED)])

    def moved():
        s = under_a_group([Node.geo(Mesh(mesh, True), RED).rotated_y(0.8).scaled((0.7, 1.4, 1.1)).translated((0.3, 0.5, -0.2))])
        return s
    hs_a, hs_b = host_glue.host_scene(first()), host_glue.host_scene(moved())
    r = host.Renderer(hs_a, traverse_of(H, mode))
    node = mesh_nodes(hs_a)[0]
    before = r.chart(node, 67, 37, mesh.tex_coords)
    r.update(hs_b)
    want = expected(hs_b, node, mesh, True, mesh.tex_coords, 67, 37)
    assert_same(r.chart(node, 67, 37, mesh.tex_coords), want, "after update, %s" % mode)
    assert not R.same_bits(before["position"], want["position"]) and R.same_bits(before["tri"], want["tri"])
    r.close()


# ---- 4. composition
def _cube_among_soft_shadows_lights():
    scene = soft_shadows()[0]
    return under_a_group([Node.geo(Mesh(cube_mesh(), True), RED)], lights=scene.lights)


@pytest.mark.parametrize("which", ["cube", "fish"])
@pytest.mark.parametrize("samples", [1, 16, 64])
def test_ao_chart_and_gather_chart_equal_the_passes_fed_with_the_charts_arrays(host, H, which, samples):
    if which == "cube":
        hs, r = renderer(host, H, "soft-cube", _cube_among_soft_shadows_lights, "flat")
        node, uv = mesh_nodes(hs)[0], cube_mesh().tex_coords
    else:
        hs, r = renderer(host, H, "tank", lambda: transmission_refraction()[0], "flat")
        node, uv = [i for i in mesh_nodes(hs) if hs.flatten()["prim_type"][i] == 3][0], None
    w, h = 67, 37
    ch = r.chart(node, w, h, uv)
    P, N = ch["position"].reshape(-1, 3), ch["normal"].reshape(-1, 3)
    kw = dict(samples=samples, bias=1e-3, seed=5, pass_index=1)
    ao = r.ao(P, N, radius=3.0, first_index=0, want=("occluded", "valid", "bent"), **kw)
    got = r.ao_chart(node, w, h, uv, radius=3.0, want=("occluded", "valid", "bent"), **kw)
    for k in ("occluded", "valid", "bent"):
        assert R.same_bits(got[k].reshape(ao[k].shape), ao[k]), "ao_chart %s" % k
    assert np.array_equal(got["valid"] == 0, ch["covered"] == 0), "valid is 0 exactly on the uncovered texels"
    assert got["visibility"].shape == (h, w) and 0 < int(got["occluded"].sum())
    bg = (0.25, 0.5, 1.0)
    ga = r.gather(P, N, bg, first_index=0, want=("sum", "valid"), **kw)
    gg = r.gather_chart(node, w, h, bg, uv, want=("sum", "valid"), **kw)
    for k in ("sum", "valid"):
        assert R.same_bits(gg[k].reshape(ga[k].shape), ga[k]), "gather_chart %s" % k
    assert np.array_equal(gg["valid"] == 0, ch["covered"] == 0) and gg["mean"].shape == (h, w, 3)
    flipped = r.ao_chart(node, w, h, uv, radius=3.0, flip_normal=True, want=("bent",), **kw)
    flip_ch = r.chart(node, w, h, uv, flip_normal=True)
    assert R.same_bits(flipped["bent"].reshape(-1, 3), r.ao(flip_ch["position"].reshape(-1, 3), flip_ch["normal"].reshape(-1, 3), radius=3.0, want=("bent",), **kw)["bent"])


# ---- 5. schedule independence
def test_the_same_chart_twice_and_overlapping_charts_ten_times_give_the_same_bits(host, H):
    v, n, uv, _ = CASES["overlap"]
    mesh = corner_mesh(v, n)
    hs, r = renderer(host, H, ("overlap", True), lambda: under_a_group([Node.geo(Mesh(mesh, True), RED)]), "flat")
    node = mesh_nodes(hs)[0]
    first = r.chart(node, 67, 37, uv)
    again = r.chart(node, 67, 37, uv)
    assert_same(again, first, "the same chart queued twice")
    for k in range(10):
        assert R.same_bits(r.chart(node, 64, 64, uv, want=("tri",))["tri"], expected(hs, node, mesh, True, uv, 64, 64)["tri"]), "run %d" % k


# ---- 6. the device form
def test_device_tensors_on_a_torch_stream_and_the_pass_protocol(H):
    """pt_chart_device with the UV set and the results in torch tensors on a stream of torch's, in a process of its own in which torch initialises its GPU side
    first. While it is open a second aov, guides or chart pass is refused; a render on each slot and a rays pass are in flight around it; pt_aov_finish closes
    it; a tensor that is too short is refused before any kernel runs; Renderer.chart takes tensors."""
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
import chart_restate as R
import host_glue
import test_gpu_chart as T
from scene_dsl import Mesh, Node, default_background
lib = H.lib()
mesh = T.cube_mesh()
hs = host_glue.host_scene(T.under_a_group([Node.geo(Mesh(mesh, True), T.RED)]))
r = host.Renderer(hs, H.TRAVERSE_FLAT)
cx = r.context
node = T.mesh_nodes(hs)[0]
W, HT = 67, 37
uv = np.ascontiguousarray(mesh.tex_coords[mesh.triangles.astype(np.int64)].reshape(-1, 6))
want = T.expected(hs, node, mesh, True, uv, W, HT)
ref = r.chart(node, W, HT, uv)
T.assert_same(ref, want, "host path")
ptr = lambda tensor: C.c_void_p(tensor.data_ptr())
dp = lambda a: a.ctypes.data_as(H._dp)
d_uv = torch.from_numpy(uv).to(dev)
kinds = {"position": torch.float64, "normal": torch.float64, "tri": torch.int32, "covered": torch.uint8}
w, h = 160, 96
cam = host.camera(np.array([0.8, 1.5, 7.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.7]), w, h)
bg = default_background(w, h)
d_bg = torch.from_numpy(np.ascontiguousarray(bg)).to(dev)
P = np.ascontiguousarray(ref["position"].reshape(-1, 3) + 0.5 * ref["normal"].reshape(-1, 3)); N = np.ascontiguousarray(-ref["normal"].reshape(-1, 3))
d_P, d_N = torch.from_numpy(P).to(dev), torch.from_numpy(N).to(dev)
n = W * HT
p = H.PtChartParams(node, W, HT, 0)
rp = H.PtRaysParams(n, 1, 0)
results = []
for overlapped in (False, True):
    t = {k: torch.full((HT, W) + ((3,) if k in ("position", "normal") else ()), 5, dtype=kinds[k], device=dev) for k in kinds}
    t_occ = torch.full((n,), 5, dtype=torch.uint8, device=dev)
    imgs = [torch.zeros((h, w, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != 0
    b = H.PtChartBuffers(C.cast(ptr(t["position"]), H._dp), C.cast(ptr(t["normal"]), H._dp), C.cast(ptr(t["tri"]), H._ip), C.cast(ptr(t["covered"]), H._u8p))
    rb = H.PtRaysBuffers(occluded=C.cast(ptr(t_occ), H._u8p))
    st = H.PtStats()

    def render(k):
        q = H.PtRenderParams(w, h, H.PtRect(0, 0, w - 1, h - 1), 2, 10 + k, H.SAMPLE_RNG, 1, 0, 1, 0)
        return lib.pt_render_device(cx, C.byref(cam), ptr(d_bg), C.byref(q), 0, ptr(imgs[k]), C.c_void_p(lib.pt_context_stream(cx, k)))
    rays = lambda: lib.pt_rays_device(cx, C.byref(rp), ptr(d_P), ptr(d_N), C.byref(rb), None)
    chart = lambda: lib.pt_chart_device(cx, C.byref(p), ptr(d_uv), C.byref(b), C.c_void_p(stream.cuda_stream))
    if overlapped:
        assert render(0) == H.OK and render(1) == H.OK and rays() == H.OK, lib.pt_last_error(cx)
        assert chart() == H.OK, lib.pt_last_error(cx)
        assert chart() == H.ERR_ARGUMENT and b"pt_chart_device pass is in flight" in lib.pt_last_error(cx)  # one aov / guides / chart pass in flight per context ...
        ht = np.full((HT, W), 9, dtype=np.int32)
        hb = H.PtChartBuffers(tri=ht.ctypes.data_as(H._ip))
        assert lib.pt_chart(cx, C.byref(p), dp(uv), C.byref(hb), None) == H.ERR_ARGUMENT  # ... the host path included,
        ap = H.PtAovParams(w, h, H.PtRect(0, 0, w - 1, h - 1), (C.c_double * 2)(0.5, 0.5))
        depth = np.full((h, w), 9.0)
        ab = H.PtAovBuffers(depth=dp(depth))
        assert lib.pt_aov(cx, C.byref(cam), C.byref(ap), C.byref(ab), None) == H.ERR_ARGUMENT  # the aov pass
        assert lib.pt_aov_device(cx, C.byref(cam), C.byref(ap), C.byref(ab), None) == H.ERR_ARGUMENT
        alb = np.full((h, w, 3), 9.0)
        gb = H.PtGuidesBuffers(albedo=dp(alb))
        assert lib.pt_guides(cx, C.byref(cam), C.byref(ap), C.byref(gb), None) == H.ERR_ARGUMENT  # and the guides pass
        assert lib.pt_guides_device(cx, C.byref(cam), C.byref(ap), C.byref(gb), None) == H.ERR_ARGUMENT
        assert np.all(ht == 9) and np.all(depth == 9.0) and np.all(alb == 9.0)
        ms = C.c_double(-1.0)
        assert lib.pt_aov_finish(cx, C.byref(ms)) == H.OK and ms.value > 0.0, lib.pt_last_error(cx)
        assert lib.pt_aov_finish(cx, None) == H.ERR_ARGUMENT  # nothing in flight any more
        assert lib.pt_render_finish(cx, C.byref(st)) == H.OK and lib.pt_render_finish(cx, C.byref(st)) == H.OK and lib.pt_rays_finish(cx, None) == H.OK, lib.pt_last_error(cx)
    else:
        for k in (0, 1):
            assert render(k) == H.OK and lib.pt_render_finish(cx, C.byref(st)) == H.OK, lib.pt_last_error(cx)
        assert rays() == H.OK and lib.pt_rays_finish(cx, None) == H.OK, lib.pt_last_error(cx)
        assert chart() == H.OK and lib.pt_aov_finish(cx, None) == H.OK, lib.pt_last_error(cx)
    stream.synchronize(); torch.cuda.synchronize()
    results.append(dict({k: t[k].cpu().numpy().tobytes() for k in t}, occ=t_occ.cpu().numpy().tobytes(), img0=imgs[0].cpu().numpy().tobytes(), img1=imgs[1].cpu().numpy().tobytes()))
for k in results[0]:
    assert results[0][k] == results[1][k], k
for k in kinds:
    assert results[1][k] == want[k].tobytes(), k
assert any(results[1]["img0"]) and any(results[1]["img1"]) and 1 in results[1]["occ"] and 5 not in results[1]["occ"]
# a tensor that is too short, host memory and a pointer inside an allocation: refused before any kernel runs, nothing written, the pass stays free
# (allocations of the library's own, whose size is exact: a small tensor of torch's is a piece of a larger allocation, and the check sees the allocation)
short, short_uv = C.c_void_p(), C.c_void_p()
assert lib.pt_device_alloc(cx, 4096, C.byref(short)) == H.OK and lib.pt_device_alloc(cx, 4096, C.byref(short_uv)) == H.OK  # 9,916 and 576 bytes are needed
short_uv = C.c_void_p(short_uv.value + 4096 - 64)  # ... of which 64 lie behind this pointer
assert lib.pt_chart_device(cx, C.byref(p), ptr(d_uv), C.byref(H.PtChartBuffers(tri=C.cast(short, H._ip))), None) == H.ERR_ARGUMENT
assert b"tri" in lib.pt_last_error(cx)
tri_t = torch.full((HT, W), 5, dtype=torch.int32, device=dev)
tb = H.PtChartBuffers(tri=C.cast(ptr(tri_t), H._ip))
assert lib.pt_chart_device(cx, C.byref(p), short_uv, C.byref(tb), None) == H.ERR_ARGUMENT and b"d_uv" in lib.pt_last_error(cx)
assert lib.pt_chart_device(cx, C.byref(p), C.c_void_p(uv.ctypes.data), C.byref(tb), None) == H.ERR_ARGUMENT
torch.cuda.synchronize()
assert bool((tri_t == 5).all())
assert lib.pt_device_free(cx, short) == H.OK and lib.pt_device_free(cx, C.c_void_p(short_uv.value - 4096 + 64)) == H.OK
assert lib.pt_aov_finish(cx, None) == H.ERR_ARGUMENT  # no pass was opened
# Renderer.chart with tensors
out = r.chart(node, W, HT, d_uv, into={"tri": tri_t})
assert out["tri"] is tri_t and isinstance(out["position"], torch.Tensor)
for k in kinds:
    assert out[k].cpu().numpy().tobytes() == want[k].tobytes(), k
r.close()
assert (x * 2).sum().item() == 2048.0
print("chart into torch tensors ok")
""" % (root, root)
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "chart into torch tensors ok" in done.stdout, done.stdout[-2000:] + done.stderr[-4000:]


# ---- 7. refusals on a context
def test_argument_errors_with_a_context(host, H):
    lib = H.lib()
    mesh = cube_mesh()
    hs, r = renderer(host, H, ("cube", False, False), lambda: under_a_group([Node.geo(Mesh(mesh, False), RED)]), "flat")
    cx = r.context
    node = mesh_nodes(hs)[0]
    n_nodes = len(hs.flatten()["prim_type"])
    uv = np.ascontiguousarray(mesh.tex_coords[mesh.triangles.astype(np.int64)].reshape(-1, 6))
    tri = np.full((4, 4), 7, dtype=np.int32)
    b = H.PtChartBuffers(tri=tri.ctypes.data_as(H._ip))
    dp = uv.ctypes.data_as(H._dp)
    ok = dict(node=node, width=4, height=4, flags=0)
    call = lambda p, u=dp, bufs=b: lib.pt_chart(cx, C.byref(p) if p is not None else None, u, C.byref(bufs) if bufs is not None else None, None)
    assert call(None) == H.ERR_ARGUMENT and call(H.PtChartParams(**ok), dp, None) == H.ERR_ARGUMENT
    words = [(dict(flags=2), b"unknown flags"), (dict(width=0), b"positive"), (dict(height=0), b"positive"), (dict(width=8192, height=4096), b"PT_AO_MAX"),
             (dict(node=n_nodes), b"flattened nodes"), (dict(node=[i for i in range(n_nodes) if i != node][0]), b"is no mesh")]
    for change, word in words:
        assert call(H.PtChartParams(**dict(ok, **change))) == H.ERR_ARGUMENT and word in lib.pt_last_error(cx), change
    assert call(H.PtChartParams(**ok), dp, H.PtChartBuffers()) == H.ERR_ARGUMENT and b"no output buffer" in lib.pt_last_error(cx)
    assert call(H.PtChartParams(**ok), None) == H.ERR_ARGUMENT and b"uv is NULL" in lib.pt_last_error(cx)
    assert np.all(tri == 7)
    n = C.c_uint64(0)
    assert lib.pt_chart_triangles(cx, node, C.byref(n)) == H.OK and n.value == 12
    assert lib.pt_chart_triangles(cx, n_nodes, C.byref(n)) == H.ERR_ARGUMENT and lib.pt_chart_triangles(cx, node, None) == H.ERR_ARGUMENT
    assert call(H.PtChartParams(**ok)) == H.OK and set(np.unique(tri)) <= set(range(-1, 12))
    empty = H.Context()
    assert lib.pt_chart(empty.handle, C.byref(H.PtChartParams(**ok)), dp, C.byref(b), None) == H.ERR_NO_SCENE
    assert lib.pt_chart_triangles(empty.handle, 0, C.byref(n)) == H.ERR_NO_SCENE
    empty.close()
