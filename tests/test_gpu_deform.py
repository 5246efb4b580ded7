"""pt_scene_deform / Renderer.deform on the GPU: a renderer created on scene A whose meshes are then deformed to scene B's answers exactly as a fresh
Renderer on B and as the oracle's render of B - u8 image, f64 linear means, the six ray counters, kernel mode and variant - in all three traversals, with
the mesh trees built on the host and on the device at upload (PORTRAYER_BUILD), refitted and - where the device built them - rebuilt in place. Every
comparison is exact. The base object is a sheet: a grid of quads with z = a sin(k x + phase); `phase` is the deformation."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_glue  # noqa: E402
from device_glue import bbox_invtrans  # noqa: E402
from example_scenes import fish, macho_cows  # noqa: E402
from scene_dsl import Camera, Cube, KDMesh, Light, Material, Mesh, MeshData, Node, Scene, Sphere, default_background  # noqa: E402
from test_gpu_update import COUNTERS, HT, KW, MODES, W, equals_oracle, kd_of, motion_of, same_render, shoot, traverse  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ARG, NO_SCENE = -1, -3


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def sheet(tris, phase=0.0, normals=False, flat=False, shift=0.0, permute=False, amp=0.35):
    """the first `tris` triangles of an n x n grid of quads over [-1.5, 1.5]^2, z = amp sin(2.2 x + 0.7 y + phase)"""
    n = max(1, int(np.ceil(np.sqrt(tris / 2.0))))
    xs = np.linspace(-1.5, 1.5, n + 1)
    x, y = np.meshgrid(xs, xs)
    x, y = x.ravel(), y.ravel()
    arg = 2.2 * x + 0.7 * y + phase
    z = np.zeros_like(x) if flat else amp * np.sin(arg)
    pos = np.stack([x + shift, y, z], axis=1).astype(np.float64)
    if permute:
        pos = pos[np.random.default_rng(11).permutation(len(pos))]
    idx = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            idx += [[a, a + 1, a + n + 2], [a, a + n + 2, a + n + 1]]
    nrm = None
    if normals:
        g = np.stack([-amp * 2.2 * np.cos(arg), -amp * 0.7 * np.cos(arg), np.ones_like(x)], axis=1)
        nrm = g / np.linalg.norm(g, axis=1, keepdims=True)
    return MeshData(pos, np.array(idx[:tris], dtype=np.uint32), nrm, "sheet")


RED = Material(diffuse=(0.8, 0.25, 0.2), specular=(0.5, 0.5, 0.5), shininess=40.0)
BLUE = Material(diffuse=(0.2, 0.3, 0.8), specular=(0.3, 0.3, 0.3), shininess=25.0)
GREY = Material(diffuse=(0.6, 0.6, 0.6))
LIGHTS = [Light(position=(3.0, 4.0, 9.0), color=(0.9, 0.9, 0.9)), Light(position=(-5.0, 2.0, 6.0), color=(0.3, 0.3, 0.4))]


def scene_of(kids, shift=0.0):
    """the sheets in front of a wall that takes their shadows, a sphere beside them"""
    wall = Node.geo(Cube(), GREY).scaled((12.0, 12.0, 0.2)).translated((shift, 0.0, -1.6))
    ball = Node.geo(Sphere(), BLUE).scaled(0.5).translated((shift + 2.3, -1.0, 0.4))
    return (Scene(root=Node.group(list(kids) + [wall, ball]), lights=[dataclasses.replace(l, position=(l.position[0] + shift, l.position[1], l.position[2])) for l in LIGHTS],
                  ambient=(0.15, 0.15, 0.15)),
            Camera(eye=(shift + 0.8, -2.5, 7.0), center=(shift, 0.0, 0.0), fovy_degrees=40.0))


def one_sheet(tris, smooth=False, **kw):
    return lambda: scene_of([Node.geo(Mesh(sheet(tris, normals=smooth, **kw), smooth), RED).rotated_y(0.3)], shift=kw.get("shift", 0.0))


def instanced(phase):
    def make():
        prim = Mesh(sheet(128, phase=phase))
        kids = [Node.geo(prim, RED).scaled(0.6).translated((-1.5, 0.9, 0.0)), Node.geo(prim, BLUE).scaled((0.9, 0.4, 1.7)).rotated_y(-0.5).translated((1.2, 0.8, 0.2)),
                Node.geo(prim, RED).scaled(0.5).rotated_x(0.6).translated((0.0, -1.2, 0.5))]
        return scene_of(kids)
    return make


def two_sheets(phase_left, phase_right):
    def make():
        kids = [Node.geo(Mesh(sheet(128, phase=phase_left)), RED).scaled(0.6).translated((-1.3, 0.0, 0.0)),
                Node.geo(Mesh(sheet(17, phase=phase_right)), BLUE).scaled(0.6).translated((1.3, 0.3, 0.0))]
        return scene_of(kids)
    return make


def meshes_of(scene):
    """the scene's distinct meshes in the order the flattened nodes first use them (breadth-first: the upload's numbering)"""
    out, seen, level = [], set(), [scene.root]
    while level:
        nxt = []
        for node in level:
            if node.geometry is not None and node.geometry[0].mesh is not None and id(node.geometry[0].mesh) not in seen:
                seen.add(id(node.geometry[0].mesh)); out.append(node.geometry[0].mesh)
            nxt += node.children
        level = nxt
    return out


def displaced(make):
    """an example scene with every mesh's vertices moved by a smooth function of their position"""
    def build():
        scene, cam = make()[:2]
        new, done = {}, set()

        def walk(node):
            if id(node) in done:
                return
            done.add(id(node))
            if node.geometry is not None and node.geometry[0].mesh is not None:
                prim, mat = node.geometry
                m = prim.mesh
                if id(m) not in new:
                    ext = (m.positions.max(axis=0) - m.positions.min(axis=0)).max()
                    p = m.positions + 0.06 * ext * np.sin(4.0 * m.positions[:, [1, 2, 0]] / ext + 0.5)
                    new[id(m)] = dataclasses.replace(m, positions=np.ascontiguousarray(p))
                node.geometry = (dataclasses.replace(prim, mesh=new[id(m)]), mat)
            for c in node.children:
                walk(c)
        walk(scene.root)
        return scene, cam
    return build


_CACHE = {}


def case(oracle, key, make):
    if key not in _CACHE:
        scene, cam = make()[:2]
        _CACHE[key] = (scene, cam, oracle.pack(scene), host_glue.host_scene(scene))
    return _CACHE[key]


def reference(oracle, key, mode):
    k = ("ref", key, mode)
    if k not in _CACHE:
        _, cam, ps, _ = _CACHE[key]
        ref = oracle.render(ps, cam, W, HT, samples=KW["samples"], seed=KW["seed"], jitter=oracle.JITTER_RNG, mode={"flat": oracle.MODE_FLAT, "kd": oracle.MODE_KD, "hier": oracle.MODE_HIER}[mode], kd_depth=8)
        assert np.isfinite(ref.linear).all(), f"{key}: the oracle's image has non-finite values: pick another deformation"
        _CACHE[k] = ref
    return _CACHE[k]


def fresh_render(H, host, oracle, key, mode, build):
    k = ("fresh", key, mode, build)
    if k not in _CACHE:
        _, cam, _, hs = _CACHE[key]
        f = host.Renderer(hs, traverse(H, oracle, mode)[0], kd_depth=8)
        try:
            _CACHE[k] = shoot(H, f, cam, W, HT)
        finally:
            f.close()
    return _CACHE[k]


def deform_and_compare(H, host, oracle, monkeypatch, name, make_a, make_b, mode, build, rebuild, differ=0.0):
    monkeypatch.setenv("PORTRAYER_BUILD", build)
    _, cam_a, _, host_a = case(oracle, (name, "A"), make_a)
    _, cam_b, _, host_b = case(oracle, (name, "B"), make_b)
    where = f"{name}, {mode}, {build} build, {'rebuild' if rebuild else 'refit'}"
    ref_b = reference(oracle, (name, "B"), mode)
    if differ:
        assert (reference(oracle, (name, "A"), mode).rgb != ref_b.rgb).any(axis=2).mean() >= differ, f"{where}: A and B must look different, or doing nothing would pass"
    want = fresh_render(H, host, oracle, (name, "B"), mode, build)
    r = host.Renderer(host_a, traverse(H, oracle, mode)[0], kd_depth=8)
    try:
        shoot(H, r, cam_a, W, HT)  # the scene has been in use before it is deformed
        r.deform(host_b, rebuild=rebuild)
        got = shoot(H, r, cam_b, W, HT)
    finally:
        r.close()
    same_render(got, want, where)
    equals_oracle(got, ref_b, where)


def raw_deform(H, mesh, index, keep, rebuild=0, normals=True):
    """a pt_mesh_deform for the test-DSL mesh `mesh` as mesh `index` of the uploaded scene"""
    d = H.PtMeshDeform()
    pos = np.ascontiguousarray(mesh.positions, dtype=np.float64)
    box = np.ascontiguousarray(bbox_invtrans(pos.min(axis=0), pos.max(axis=0)).reshape(16))
    nrm = np.ascontiguousarray(mesh.normals, dtype=np.float64) if normals and mesh.normals is not None else None
    keep.append((pos, box, nrm))
    d.mesh, d.positions, d.bounds_invtrans, d.rebuild = index, H._p(pos, H._dp), H._p(box, H._dp), rebuild
    d.normals = H._p(nrm, H._dp) if nrm is not None else None
    return d


def call_deform(H, ctx, deforms, mo, kd=None):
    arr = (H.PtMeshDeform * max(len(deforms), 1))(*deforms)
    return H.lib().pt_scene_deform(ctx, len(deforms), arr, C.byref(mo) if mo is not None else None, C.byref(kd) if kd is not None else None)


# ---- 1. sizes where the code can go wrong: the root a leaf (1, 2 triangles), one node (3), the device builder's threshold (16), several blocks of a refit (128)
@pytest.mark.parametrize("build", ["host", "device"])
@pytest.mark.parametrize("tris", [1, 2, 3, 15, 16, 17, 128])
def test_sizes(H, host, oracle, monkeypatch, tris, build):
    for mode in MODES:
        for rebuild in ([False, True] if build == "device" and tris >= 16 else [False]):
            deform_and_compare(H, host, oracle, monkeypatch, f"sheet-{tris}", one_sheet(tris), one_sheet(tris, phase=1.4), mode, build, rebuild,
                               differ=0.01 if tris >= 15 else 0.0)


@pytest.mark.parametrize("mode", MODES)
def test_rebuilding_a_host_built_tree_is_refused(H, host, oracle, monkeypatch, mode):
    monkeypatch.setenv("PORTRAYER_BUILD", "host")
    _, cam_a, _, host_a = case(oracle, ("sheet-128", "A"), one_sheet(128))
    scene_b, cam_b, _, host_b = case(oracle, ("sheet-128", "B"), one_sheet(128, phase=1.4))
    keep = []
    r = host.Renderer(host_a, traverse(H, oracle, mode)[0], kd_depth=8)
    try:
        before = shoot(H, r, cam_a, W, HT)
        kdt = kd_of(H, host_b, keep) if mode == "kd" else None
        assert call_deform(H, r.context, [raw_deform(H, meshes_of(scene_b)[0], 0, keep, rebuild=1)], motion_of(H, host_b, mode, keep), kdt) == ARG
        assert b"built on the host" in H.lib().pt_last_error(r.context)
        same_render(shoot(H, r, cam_a, W, HT), before, f"after the refused rebuild, {mode}")
        r.deform(host_b, rebuild=True)  # the host layer asks for what the tree allows: a refit
        got = shoot(H, r, cam_b, W, HT)
    finally:
        r.close()
    equals_oracle(got, reference(oracle, ("sheet-128", "B"), mode), f"refit after the refused rebuild, {mode}")


# ---- 2. instancing: one mesh under three nodes, one of them scaled non-uniformly
@pytest.mark.parametrize("build,rebuild", [("host", False), ("device", False), ("device", True)])
@pytest.mark.parametrize("mode", MODES)
def test_instances_follow_the_one_deform(H, host, oracle, monkeypatch, mode, build, rebuild):
    deform_and_compare(H, host, oracle, monkeypatch, "instanced", instanced(0.0), instanced(1.9), mode, build, rebuild, differ=0.02)


# ---- 3. smooth shading
@pytest.mark.parametrize("build,rebuild", [("host", False), ("device", False), ("device", True)])
@pytest.mark.parametrize("mode", MODES)
def test_normals_are_replaced_with_the_positions(H, host, oracle, monkeypatch, mode, build, rebuild):
    deform_and_compare(H, host, oracle, monkeypatch, "smooth", one_sheet(128, smooth=True), one_sheet(128, smooth=True, phase=1.4), mode, build, rebuild, differ=0.02)


def _old_normals_new_positions():
    scene, cam = one_sheet(128, smooth=True, phase=1.4)()
    node = scene.root.children[0]
    prim, mat = node.geometry
    node.geometry = (dataclasses.replace(prim, mesh=dataclasses.replace(prim.mesh, normals=sheet(128, normals=True).normals)), mat)
    return scene, cam


@pytest.mark.parametrize("build", ["host", "device"])
@pytest.mark.parametrize("mode", MODES)
def test_normals_null_keeps_the_resident_normals(H, host, oracle, monkeypatch, mode, build):
    monkeypatch.setenv("PORTRAYER_BUILD", build)
    _, cam_a, _, host_a = case(oracle, ("smooth", "A"), one_sheet(128, smooth=True))
    scene_b, cam_b, _, host_b = case(oracle, ("kept-normals", "B"), _old_normals_new_positions)
    want = fresh_render(H, host, oracle, ("kept-normals", "B"), mode, build)
    keep = []
    r = host.Renderer(host_a, traverse(H, oracle, mode)[0], kd_depth=8)
    try:
        kdt = kd_of(H, host_b, keep) if mode == "kd" else None
        assert call_deform(H, r.context, [raw_deform(H, meshes_of(scene_b)[0], 0, keep, normals=False)], motion_of(H, host_b, mode, keep), kdt) == 0, H.lib().pt_last_error(r.context)
        got = shoot(H, r, cam_b, W, HT)
    finally:
        r.close()
    same_render(got, want, f"normals = NULL, {mode}, {build} build")
    equals_oracle(got, reference(oracle, ("kept-normals", "B"), mode), f"normals = NULL, {mode}, {build} build")


# ---- 4. the examples
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,make", [("fish", fish), ("macho-cows", macho_cows)])
def test_examples(H, host, oracle, monkeypatch, name, make, mode):
    for build, rebuild in (("host", False), ("device", False), ("device", True)):
        deform_and_compare(H, host, oracle, monkeypatch, name, lambda: make()[:2], displaced(make), mode, build, rebuild, differ=0.01)


# ---- 5. hard deformations of the 128-triangle sheet
HARD = {"flattened": dict(flat=True), "carried-away": dict(phase=0.6, shift=1e3), "permuted": dict(phase=0.3, permute=True)}


@pytest.mark.parametrize("build,rebuild", [("host", False), ("device", False), ("device", True)])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", list(HARD))
def test_hard_deformations(H, host, oracle, monkeypatch, kind, mode, build, rebuild):
    """onto the plane z = 0 (no extent on one axis); 1e3 units out of A's root box, the camera following; vertex positions permuted at random: the refitted
    tree is as bad as a tree gets and must still be exact"""
    deform_and_compare(H, host, oracle, monkeypatch, "hard-" + kind, one_sheet(128), one_sheet(128, **HARD[kind]), mode, build, rebuild, differ=0.01)


# ---- 6. no state leaks
@pytest.mark.parametrize("build,rebuild", [("host", False), ("device", False), ("device", True)])
@pytest.mark.parametrize("mode", MODES)
def test_no_state_leaks(H, host, oracle, monkeypatch, mode, build, rebuild):
    monkeypatch.setenv("PORTRAYER_BUILD", build)
    steps = [(0.0, 0.0), (1.4, 0.0), (0.0, 0.0), (0.7, 0.0), (0.7, 2.0), (1.4, 0.0)]  # (the fifth names the OTHER mesh alone)
    for p in set(steps):
        case(oracle, ("two-sheets", p), two_sheets(*p))
    r = host.Renderer(_CACHE[("two-sheets", steps[0])][3], traverse(H, oracle, mode)[0], kd_depth=8)
    try:
        sizes = []
        for step, p in enumerate(steps):
            if step:
                r.deform(_CACHE[("two-sheets", p)][3], rebuild=rebuild)
                sizes.append(H.lib().pt_test_scene_bytes(r.context))
            want = fresh_render(H, host, oracle, ("two-sheets", p), mode, build)
            same_render(shoot(H, r, _CACHE[("two-sheets", p)][1], W, HT), want, f"step {step} {p}, {mode}, {build} build, rebuild {rebuild}")
        if mode != "kd":  # (the k-d arrays follow the scene and never shrink)
            assert sizes[0] == sizes[1], f"the second deform of a mesh made the context's scene buffers grow: {sizes}"
            assert len(set(sizes[:4])) == 1, f"the context's scene buffers grew between deforms of the same mesh: {sizes}"
        assert sizes[-1] == sizes[-2], f"the context's scene buffers grew: {sizes}"
    finally:
        r.close()


def test_a_context_that_is_never_deformed_holds_no_more_memory(H, host, oracle, monkeypatch):
    monkeypatch.setenv("PORTRAYER_BUILD", "device")
    _, _, _, host_a = case(oracle, ("two-sheets", (0.0, 0.0)), two_sheets(0.0, 0.0))
    _, _, _, host_b = case(oracle, ("two-sheets", (1.4, 0.0)), two_sheets(1.4, 0.0))
    r = host.Renderer(host_a, H.TRAVERSE_FLAT, kd_depth=8)
    try:
        uploaded = H.lib().pt_test_scene_bytes(r.context)
        r.update(host_a)
        assert H.lib().pt_test_scene_bytes(r.context) == uploaded
        r.deform(host_b)
        first = H.lib().pt_test_scene_bytes(r.context)
        assert first > uploaded  # the indices, the parents and counters, the staging buffer
        r.deform(host_a)
        assert H.lib().pt_test_scene_bytes(r.context) == first
    finally:
        r.close()


# ---- 7. the other passes after a deform
@pytest.mark.parametrize("build,rebuild", [("host", False), ("device", False), ("device", True)])
@pytest.mark.parametrize("mode", MODES)
def test_the_other_passes_after_a_deform(H, host, oracle, monkeypatch, mode, build, rebuild):
    from test_gpu_rays import incoherent_batch
    monkeypatch.setenv("PORTRAYER_BUILD", build)
    _, _, _, host_a = case(oracle, ("instanced", "A"), instanced(0.0))
    _, cam_b, ps_b, host_b = case(oracle, ("instanced", "B"), instanced(1.9))
    if "batch" not in _CACHE:
        _CACHE["batch"] = incoherent_batch(oracle, ps_b, oracle.flatten(ps_b), 4242, n=4096)
    o, d = _CACHE["batch"]
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
        r.deform(host_b, rebuild=rebuild)
        got, want = everything(r), everything(fresh)
    finally:
        r.close(); fresh.close()
    assert len(got) == 6 + 2 * 7 + 2 + 2
    for k in want:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{mode}, {build} build, rebuild {rebuild}: {k} differs"
    assert (got["aov.sub"] > 0).any() and np.isfinite(got["rays0.t"]).any()


# ---- 8. every listed error leaves the scene rendering A
def _with_a_kdmesh(phase, kd_phase=None):
    def make():
        kids = [Node.geo(Mesh(sheet(128, phase=phase, normals=True), True), RED).scaled(0.6).translated((-1.3, 0.0, 0.0)),
                Node.geo(KDMesh(sheet(17, phase=phase if kd_phase is None else kd_phase)), BLUE).scaled(0.6).translated((1.3, 0.3, 0.0)),
                Node.geo(Mesh(sheet(15, phase=phase)), BLUE).scaled(0.4).translated((0.0, -1.4, 0.3))]
        return scene_of(kids)
    return make


@pytest.mark.parametrize("mode", MODES)
def test_errors_leave_the_scene_usable(H, host, oracle, monkeypatch, mode):
    monkeypatch.setenv("PORTRAYER_BUILD", "device")  # mesh 0 (128 triangles) is device-built, mesh 2 (15) host-built; mesh 1 has a KDMesh tree
    L = H.lib()
    _, cam_a, _, host_a = case(oracle, ("errors", "A"), _with_a_kdmesh(0.0))
    scene_b, cam_b, _, host_b = case(oracle, ("errors", "B"), _with_a_kdmesh(1.4))
    mb = meshes_of(scene_b)
    assert [len(m.triangles) for m in mb] == [128, 17, 15]
    keep = []
    kdt = kd_of(H, host_b, keep) if mode == "kd" else None
    good = lambda: motion_of(H, host_b, mode, keep)  # noqa: E731
    fresh_ctx = H.Context()
    assert call_deform(H, fresh_ctx.handle, [raw_deform(H, mb[0], 0, keep)], good(), kdt) == NO_SCENE
    fresh_ctx.close()
    r = host.Renderer(host_a, traverse(H, oracle, mode)[0], kd_depth=8)
    try:
        before = shoot(H, r, cam_a, W, HT)
        ctx = r.context

        def refused(deforms, mo="good", kd=kdt, says=None):
            rc = call_deform(H, ctx, deforms, good() if mo == "good" else mo, kd)
            assert rc == ARG, (rc, L.pt_last_error(ctx))
            assert says is None or says in L.pt_last_error(ctx), L.pt_last_error(ctx)
        ok = lambda **kw: raw_deform(H, mb[0], 0, keep, **kw)  # noqa: E731
        assert L.pt_scene_deform(ctx, 1, None, C.byref(good()), C.byref(kdt) if kdt is not None else None) == ARG
        refused([ok()], mo=None)
        d = ok(); d.positions = None
        refused([d], says=b"required")
        d = ok(); d.bounds_invtrans = None
        refused([d], says=b"required")
        d = ok(); d.mesh = 3
        refused([d], says=b"out of range")
        refused([ok(), ok()], says=b"twice")
        d = raw_deform(H, mb[2], 2, keep); d.normals = ok().normals
        refused([d], says=b"without normals")
        refused([raw_deform(H, mb[1], 1, keep)], says=b"KDMesh")
        refused([raw_deform(H, mb[2], 2, keep, rebuild=1)], says=b"built on the host")
        d = ok(); d.rebuild = 2
        refused([d], says=b"0 or 1")
        far = dataclasses.replace(mb[0], positions=mb[0].positions * 1e19)
        refused([raw_deform(H, far, 0, keep)], says=b"1e18")
        nan = mb[0].positions.copy(); nan[5, 1] = np.nan
        refused([raw_deform(H, dataclasses.replace(mb[0], positions=nan), 0, keep)], says=b"not finite")
        # everything pt_scene_update refuses about motion or kd
        mo = good(); mo.n_nodes += 1
        refused([ok()], mo=mo)
        mo = good(); mo.trans = None
        refused([ok()], mo=mo)
        if mode == "kd":
            refused([ok()], kd=None)
        else:
            refused([ok()], kd=H.PtKdTree())
        # a pass in flight: refused until its _finish
        o = np.ascontiguousarray(np.tile([0.0, 0.0, 50.0], (64, 1))); dd = np.ascontiguousarray(np.tile([0.0, 0.0, -1.0], (64, 1)))
        d_o, d_d, d_t = C.c_void_p(), C.c_void_p(), C.c_void_p()
        for ptr, nbytes in ((d_o, o.nbytes), (d_d, dd.nbytes), (d_t, 64 * 8)):
            assert L.pt_device_alloc(ctx, nbytes, C.byref(ptr)) == 0
        assert L.pt_copy_to_device(ctx, d_o, o.ctypes.data_as(C.c_void_p), o.nbytes) == 0 and L.pt_copy_to_device(ctx, d_d, dd.ctypes.data_as(C.c_void_p), dd.nbytes) == 0
        rp = H.PtRaysParams(64, 0, 0)
        rb = H.PtRaysBuffers(); rb.t = C.cast(d_t, H._dp)
        assert L.pt_rays_device(ctx, C.byref(rp), d_o, d_d, C.byref(rb), None) == 0
        refused([ok()], says=b"in flight")
        assert L.pt_rays_finish(ctx, None) == 0
        for ptr in (d_o, d_d, d_t):
            assert L.pt_device_free(ctx, ptr) == 0
        # every refusal came before the first write
        same_render(shoot(H, r, cam_a, W, HT), before, f"after the refused deforms, {mode}")
        # n_deforms = 0 is a plain update
        assert call_deform(H, ctx, [], motion_of(H, host_a, mode, keep), kd_of(H, host_a, keep) if mode == "kd" else None) == 0, L.pt_last_error(ctx)
        same_render(shoot(H, r, cam_a, W, HT), before, f"after a deform of no mesh, {mode}")
        # then the two meshes that can be deformed, one rebuilt and one refitted, in one call; the mesh with the KDMesh tree stays as it is
        assert [L.pt_scene_mesh_rebuildable(ctx, m) for m in range(4)] == [1, 1, 0, ARG]
        scene_c, cam_c, _, _ = case(oracle, ("errors", "C"), lambda: _with_a_kdmesh(1.4, kd_phase=0.0)())
        mc = meshes_of(scene_c)
        host_c = _CACHE[("errors", "C")][3]
        deforms = [raw_deform(H, mc[2], 2, keep), raw_deform(H, mc[0], 0, keep, rebuild=1)]
        assert call_deform(H, ctx, deforms, motion_of(H, host_c, mode, keep), kd_of(H, host_c, keep) if mode == "kd" else None) == 0, L.pt_last_error(ctx)
        got = shoot(H, r, cam_c, W, HT)
    finally:
        r.close()
    same_render(got, fresh_render(H, host, oracle, ("errors", "C"), mode, "device"), f"two of three meshes deformed beside a KDMesh tree, {mode}")
    equals_oracle(got, reference(oracle, ("errors", "C"), mode), f"two of three meshes deformed beside a KDMesh tree, {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_two_meshes_in_one_call(H, host, oracle, monkeypatch, mode):
    """through the C ABI: the device-built mesh rebuilt and the host-built one refitted by one pt_scene_deform"""
    monkeypatch.setenv("PORTRAYER_BUILD", "device")
    _, _, _, host_a = case(oracle, ("pair", "A"), lambda: scene_of([Node.geo(Mesh(sheet(128)), RED).scaled(0.6).translated((-1.3, 0.0, 0.0)),
                                                                       Node.geo(Mesh(sheet(15)), BLUE).scaled(0.6).translated((1.3, 0.3, 0.0))]))
    scene_b, cam_b, _, host_b = case(oracle, ("pair", "B"), lambda: scene_of([Node.geo(Mesh(sheet(128, phase=1.4)), RED).scaled(0.6).translated((-1.3, 0.0, 0.0)),
                                                                                Node.geo(Mesh(sheet(15, phase=2.0)), BLUE).scaled(0.6).translated((1.3, 0.3, 0.0))]))
    mb, keep = meshes_of(scene_b), []
    r = host.Renderer(host_a, traverse(H, oracle, mode)[0], kd_depth=8)
    try:
        kdt = kd_of(H, host_b, keep) if mode == "kd" else None
        deforms = [raw_deform(H, mb[1], 1, keep), raw_deform(H, mb[0], 0, keep, rebuild=1)]
        assert call_deform(H, r.context, deforms, motion_of(H, host_b, mode, keep), kdt) == 0, H.lib().pt_last_error(r.context)
        got = shoot(H, r, cam_b, W, HT)
    finally:
        r.close()
    same_render(got, fresh_render(H, host, oracle, ("pair", "B"), mode, "device"), f"two meshes, {mode}")
    equals_oracle(got, reference(oracle, ("pair", "B"), mode), f"two meshes, {mode}")


# ---- 9. two ranks on one device
@pytest.mark.parametrize("build,rebuild", [("host", False), ("device", True)])
@pytest.mark.parametrize("mode", MODES)
def test_a_node_of_two_ranks(H, host, oracle, monkeypatch, mode, build, rebuild):
    """pt_node_scene_deform on two ranks of one device, then pt_node_render: the single context's image"""
    monkeypatch.setenv("PORTRAYER_BUILD", build)
    _, _, _, host_a = case(oracle, ("instanced", "A"), instanced(0.0))
    _, cam_b, _, host_b = case(oracle, ("instanced", "B"), instanced(1.9))
    ref = reference(oracle, ("instanced", "B"), mode)
    monkeypatch.setenv("PORTRAYER_DEVICES", "0,0")
    r = host.Renderer(host_a, traverse(H, oracle, mode)[0], kd_depth=8)
    try:
        assert r.ranks == 2 and r.node
        r.deform(host_b, rebuild=rebuild)
        rgb, _, _ = r.render(host_glue.cam10(cam_b), W, HT, np.ascontiguousarray(default_background(W, HT)), sample_mode=H.SAMPLE_RNG, want_linear=False, **KW)
    finally:
        r.close()
    assert np.array_equal(rgb, ref.rgb), f"{mode}, {build} build: {(rgb != ref.rgb).any(axis=2).sum()} pixels differ"
