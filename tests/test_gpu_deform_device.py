"""pt_vertex_bounds_device / pt_scene_deform_device / Renderer.deform_device on the GPU: resident meshes deformed from vertices that are already in device
memory. The reduction's box is compared, bit for bit, with a replay of the host loop (pt_mesh_vertex_box: ascending index, `x < lo`, `hi < x`); a renderer
deformed from device memory answers exactly as one deformed by pt_scene_deform from host arrays, as a fresh Renderer on the deformed scene and as the oracle,
in all three traversals, with the mesh trees built on the host and on the device, refitted and rebuilt. Every comparison is exact. Device buffers are torch
tensors or pt_device_alloc allocations. Scenes, frames and helpers are those of test_gpu_deform.py and test_gpu_update.py.

Deliberately not tested: a buffer that is too short for the mesh. If the range check were wrong, such a test would read past an allocation on a machine
others use. The interior-pointer case exercises the check's base-and-size arithmetic instead, and the refusals that are tested (pinned host memory) could
not fault even without the check."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_glue  # noqa: E402
from device_glue import bbox_invtrans  # noqa: E402
from scene_dsl import Mesh, Node  # noqa: E402
from test_gpu_deform import (RED, _old_normals_new_positions, _with_a_kdmesh, call_deform, case, fresh_render, instanced, meshes_of, one_sheet,  # noqa: E402
                             raw_deform, reference, scene_of, sheet, two_sheets)
from test_gpu_update import HT, MODES, W, equals_oracle, kd_of, motion_of, same_render, shoot, traverse  # noqa: E402

pytestmark = pytest.mark.gpu

ARG = -1


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


@pytest.fixture(scope="module")
def ctx(H):
    c = H.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def shape(H, ctx):
    """(vertices a block takes per step, most blocks launched): the kernel's own constants"""
    out = (C.c_uint64 * 2)()
    assert H.lib().pt_test_vertex_box_shape(ctx.handle, C.byref(out)) == 0
    assert out[0] % 64 == 0 and out[0] >= 128 and out[1] >= 2
    return int(out[0]), int(out[1])


def on_device(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), dtype=torch.float64, device="cuda")


# ---- 1. the reduction against the host loop, bits compared
def replay_loop(pos):
    """pt_mesh_vertex_box's loop, literally, over the finite coordinates; (box, non_finite)"""
    lo, hi, bad = [np.float64(np.inf)] * 3, [np.float64(-np.inf)] * 3, 0
    for v in range(len(pos)):
        for k in range(3):
            x = pos[v, k]
            if not np.isfinite(x):
                bad += 1
                continue
            if x < lo[k]:
                lo[k] = x
            if hi[k] < x:
                hi[k] = x
    return np.array(lo + hi, dtype=np.float64), bad


def replay(pos):
    """the same result without a Python loop: the loop keeps the FIRST element that equals the extreme (+0.0 == -0.0)"""
    box = np.array([np.inf] * 3 + [-np.inf] * 3)
    fin = np.isfinite(pos)
    for k in range(3):
        x = pos[fin[:, k], k]
        if len(x):
            box[k], box[3 + k] = x[np.argmax(x == x.min())], x[np.argmax(x == x.max())]
    return box, int((~fin).sum())


def check_box(ctx, pos, where):
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    want, want_bad = replay(pos)
    if len(pos) <= 600:
        slow, slow_bad = replay_loop(pos)
        assert np.array_equal(slow.view(np.uint64), want.view(np.uint64)) and slow_bad == want_bad, "the test's two replays disagree"
    t = on_device(pos)
    got, bad = ctx.vertex_bounds_device(t.data_ptr() if len(pos) else 0, len(pos))
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"{where}: box {got!r}, the host loop gives {want!r}"
    assert bad == want_bad, f"{where}: non_finite {bad}, want {want_bad}"


def sizes_of(shape):
    block, blocks = shape
    return sorted({1, 2, 3, 63, 64, 65, block - 1, block, block + 1, block * blocks - 1, block * blocks, block * blocks + 1})


def test_the_sizes_come_from_the_kernel(shape):
    block, blocks = shape
    assert len(sizes_of(shape)) == 12 and block * blocks + 1 < 1 << 22  # (a test of a few MB, not of gigabytes)


@pytest.mark.parametrize("which", range(12))
def test_the_box_equals_the_host_loop(ctx, shape, which):
    """vertex counts around a wavefront, the block and the count from which the grid strides; the extremes at the first vertex, at the last, and at a lane of
    the last, partly filled wavefront"""
    n = sizes_of(shape)[which]
    rng = np.random.default_rng(100 + which)
    base = rng.uniform(-1.0, 1.0, size=(n, 3))
    in_last_wave = (n - 1) - ((n - 1) % 64) // 2
    check_box(ctx, base, f"n = {n}, random")
    for at in sorted({0, n - 1, in_last_wave}):
        for sign in (-1.0, 1.0):
            pos = base.copy()
            pos[at] = sign * np.array([5.0, 6.0, 7.0])
            check_box(ctx, pos, f"n = {n}, the {'minimum' if sign < 0 else 'maximum'} of every axis at vertex {at}")
        pos = base.copy()
        pos[at] = [-5.0, 6.0, -7.0]
        pos[(at + n // 2) % n] = [5.0, -6.0, 7.0] if n > 1 else pos[at]
        check_box(ctx, pos, f"n = {n}, minima and maxima split between vertices {at} and {(at + n // 2) % n}")


@pytest.mark.parametrize("first", ["+", "-"])
def test_the_sign_of_a_zero_extreme_is_the_first_vertexs(ctx, shape, first):
    block, blocks = shape
    assert blocks >= 3
    n = 2 * block + 37
    rng = np.random.default_rng(7)
    s1, s2 = (0.0, -0.0) if first == "+" else (-0.0, 0.0)
    places = {"the first wavefront": 5, "another wavefront of the first block": 64 + 9, "another block": block + 70}
    # a mesh flat on z: zeros of sign s1 up to vertex b, where the first s2 sits, then both in mixed order
    for name, b in places.items():
        pos = rng.uniform(-1.0, 1.0, size=(n, 3))
        pos[:, 2] = np.where(rng.random(n) < 0.5, s1, s2)
        pos[:b, 2] = s1
        pos[b, 2] = s2
        check_box(ctx, pos, f"flat on z, {first}0 first, the other sign first at vertex {b} ({name})")
    # zero as the extreme of an axis that is not flat: the first zero of all at vertex a, the first of the other sign at vertex b > a
    for value_sign, axis in ((1.0, 0), (-1.0, 1)):  # x: positive values, zero is the minimum; y: negative values, zero is the maximum
        for na, a in places.items():
            for nb, b in places.items():
                if b < a:
                    continue
                b = b + 3 if b == a else b
                pos = rng.uniform(-1.0, 1.0, size=(n, 3))
                pos[:, axis] = value_sign * rng.uniform(0.5, 1.0, size=n)
                later = np.arange(n) > b
                zeros = later & (rng.random(n) < 0.3)
                pos[zeros, axis] = np.where(rng.random(int(zeros.sum())) < 0.5, s1, s2)
                pos[a, axis], pos[b, axis] = s1, s2
                check_box(ctx, pos, f"axis {axis}: {first}0 first at vertex {a} ({na}), the other sign at {b} ({nb})")


@pytest.mark.parametrize("kind", ["nan", "+inf", "-inf"])
def test_non_finite_coordinates_are_counted_and_left_out(ctx, shape, kind):
    block, _ = shape
    n = 3 * block + 5
    bad = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[kind]
    base = np.random.default_rng(3).uniform(-1.0, 1.0, size=(n, 3))
    for axis in range(3):
        extreme = int(np.argmin(base[:, axis]) if kind == "-inf" else np.argmax(base[:, axis]))
        for where, at in (("the first vertex", 0), ("the last vertex of the last block", n - 1), ("the axis' would-be extreme", extreme)):
            pos = base.copy()
            pos[at, axis] = bad
            check_box(ctx, pos, f"one {kind} on axis {axis} at {where}")


def test_nan_and_both_infinities_together_and_nothing_finite(ctx, shape):
    block, _ = shape
    n = 3 * block + 5
    pos = np.random.default_rng(4).uniform(-1.0, 1.0, size=(n, 3))
    pos[0, 0], pos[n - 1, 1], pos[int(np.argmax(pos[:, 2])), 2] = np.nan, np.inf, -np.inf
    check_box(ctx, pos, "one NaN, one +inf, one -inf")
    empty = np.array([np.inf] * 3 + [-np.inf] * 3)
    for n_all in (1, 65, n):
        t = on_device(np.full((n_all, 3), np.nan))
        got, bad = ctx.vertex_bounds_device(t.data_ptr(), n_all)
        assert np.array_equal(got.view(np.uint64), empty.view(np.uint64)) and bad == 3 * n_all
    got, bad = ctx.vertex_bounds_device(0, 0)
    assert np.array_equal(got.view(np.uint64), empty.view(np.uint64)) and bad == 0


# ---- helpers of the deform tests
def device_box(H, handle, t):
    box, bad = np.zeros(6), C.c_uint64(0)
    rc = H.lib().pt_vertex_bounds_device(handle, t.shape[0], C.c_void_p(t.data_ptr()), H._p(box, H._dp), C.byref(bad))
    assert rc == 0, H.lib().pt_last_error(handle)
    return box, int(bad.value)


def device_deform(H, handle, mesh, index, keep, rebuild=0, normals=True):
    """a pt_mesh_deform_device for the test-DSL mesh `mesh` as mesh `index` of the uploaded scene: the vertices as torch tensors, the box from the device"""
    d = H.PtMeshDeformDevice()
    pos = on_device(mesh.positions)
    box, bad = device_box(H, handle, pos)
    assert bad == 0
    inv = np.ascontiguousarray(bbox_invtrans(box[:3], box[3:]).reshape(16))
    nrm = on_device(mesh.normals) if normals and mesh.normals is not None else None
    keep.append((pos, inv, nrm))
    d.mesh, d.d_positions, d.bounds_invtrans, d.rebuild = index, pos.data_ptr(), H._p(inv, H._dp), rebuild
    d.d_normals = nrm.data_ptr() if nrm is not None else None
    return d


def call_deform_device(H, handle, deforms, mo, kd=None):
    arr = (H.PtMeshDeformDevice * max(len(deforms), 1))(*deforms)
    return H.lib().pt_scene_deform_device(handle, len(deforms), arr, C.byref(mo) if mo is not None else None, C.byref(kd) if kd is not None else None)


def device_deform_and_compare(H, host, oracle, monkeypatch, name, make_a, make_b, mode, build, rebuild, differ=0.0, which=None, normals=True):
    monkeypatch.setenv("PORTRAYER_BUILD", build)
    _, cam_a, _, host_a = case(oracle, (name, "A"), make_a)
    scene_b, cam_b, _, host_b = case(oracle, (name, "B"), make_b)
    where = f"{name}, {mode}, {build} build, {'rebuild' if rebuild else 'refit'}, from device memory"
    ref_b = reference(oracle, (name, "B"), mode)
    if differ:
        assert (reference(oracle, (name, "A"), mode).rgb != ref_b.rgb).any(axis=2).mean() >= differ, f"{where}: A and B must look different, or doing nothing would pass"
    want = fresh_render(H, host, oracle, (name, "B"), mode, build)
    keep = []
    r = host.Renderer(host_a, traverse(H, oracle, mode)[0], kd_depth=8)
    try:
        shoot(H, r, cam_a, W, HT)  # the scene has been in use before it is deformed
        mb = meshes_of(scene_b)
        deforms = [device_deform(H, r.context, mb[m], m, keep, rebuild=int(rebuild), normals=normals) for m in (range(len(mb)) if which is None else which)]
        kdt = kd_of(H, host_b, keep) if mode == "kd" else None
        assert call_deform_device(H, r.context, deforms, motion_of(H, host_b, mode, keep), kdt) == 0, H.lib().pt_last_error(r.context)
        got = shoot(H, r, cam_b, W, HT)
    finally:
        r.close()
    same_render(got, want, where)
    equals_oracle(got, ref_b, where)


# ---- 2. device deform == host deform == fresh upload == oracle
@pytest.mark.parametrize("build", ["host", "device"])
@pytest.mark.parametrize("tris", [1, 2, 3, 15, 16, 17, 128])
def test_sizes(H, host, oracle, monkeypatch, tris, build):
    for mode in MODES:
        for rebuild in ([False, True] if build == "device" and tris >= 16 else [False]):
            device_deform_and_compare(H, host, oracle, monkeypatch, f"sheet-{tris}", one_sheet(tris), one_sheet(tris, phase=1.4), mode, build, rebuild,
                                      differ=0.01 if tris >= 15 else 0.0)


@pytest.mark.parametrize("mode", MODES)
def test_two_contexts_one_deformed_from_the_host_one_from_the_device(H, host, oracle, monkeypatch, mode):
    from test_gpu_rays import incoherent_batch
    monkeypatch.setenv("PORTRAYER_BUILD", "device")
    _, _, _, host_a = case(oracle, ("instanced", "A"), instanced(0.0))
    scene_b, cam_b, ps_b, host_b = case(oracle, ("instanced", "B"), instanced(1.9))
    o, d = incoherent_batch(oracle, ps_b, oracle.flatten(ps_b), 4242, n=4096)
    tr = traverse(H, oracle, mode)[0]
    keep = []
    from_host, from_device = host.Renderer(host_a, tr, kd_depth=8), host.Renderer(host_a, tr, kd_depth=8)

    def everything(x):
        out = {"aov." + k: v for k, v in x.aov(host_glue.cam10(cam_b), W, HT, want=("depth", "node", "sub")).items()}
        out.update({"rays." + k: v for k, v in x.rays(o, d).items()})
        return {k: v for k, v in out.items() if not k.endswith("kernel_ms")}
    try:
        mesh = meshes_of(scene_b)[0]
        kdt = kd_of(H, host_b, keep) if mode == "kd" else None
        assert call_deform(H, from_host.context, [raw_deform(H, mesh, 0, keep, rebuild=1)], motion_of(H, host_b, mode, keep), kdt) == 0
        assert call_deform_device(H, from_device.context, [device_deform(H, from_device.context, mesh, 0, keep, rebuild=1)], motion_of(H, host_b, mode, keep), kdt) == 0
        same_render(shoot(H, from_device, cam_b, W, HT), shoot(H, from_host, cam_b, W, HT), f"two contexts, {mode}")
        got, want = everything(from_device), everything(from_host)
    finally:
        from_host.close(); from_device.close()
    assert len(want) == 3 + 7
    for k in want:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{mode}: {k} differs between the two contexts"
    assert (got["aov.sub"] > 0).any() and np.isfinite(got["rays.t"]).any()


# ---- 3. what rides along
@pytest.mark.parametrize("build,rebuild", [("host", False), ("device", True)])
@pytest.mark.parametrize("mode", MODES)
def test_device_normals_are_used(H, host, oracle, monkeypatch, mode, build, rebuild):
    device_deform_and_compare(H, host, oracle, monkeypatch, "smooth", one_sheet(128, smooth=True), one_sheet(128, smooth=True, phase=1.4), mode, build, rebuild, differ=0.02)


@pytest.mark.parametrize("mode", MODES)
def test_null_normals_keep_the_resident_ones(H, host, oracle, monkeypatch, mode):
    monkeypatch.setenv("PORTRAYER_BUILD", "device")
    _, _, _, host_a = case(oracle, ("smooth", "A"), one_sheet(128, smooth=True))
    scene_b, cam_b, _, host_b = case(oracle, ("kept-normals", "B"), _old_normals_new_positions)
    want = fresh_render(H, host, oracle, ("kept-normals", "B"), mode, "device")
    keep = []
    r = host.Renderer(host_a, traverse(H, oracle, mode)[0], kd_depth=8)
    try:
        kdt = kd_of(H, host_b, keep) if mode == "kd" else None
        d = device_deform(H, r.context, meshes_of(scene_b)[0], 0, keep, normals=False)
        assert not d.d_normals
        assert call_deform_device(H, r.context, [d], motion_of(H, host_b, mode, keep), kdt) == 0, H.lib().pt_last_error(r.context)
        got = shoot(H, r, cam_b, W, HT)
    finally:
        r.close()
    same_render(got, want, f"d_normals = NULL, {mode}")
    equals_oracle(got, reference(oracle, ("kept-normals", "B"), mode), f"d_normals = NULL, {mode}")


def test_normals_for_a_mesh_uploaded_without_are_refused(H, host, oracle, monkeypatch):
    monkeypatch.setenv("PORTRAYER_BUILD", "device")
    _, cam_a, _, host_a = case(oracle, ("sheet-128", "A"), one_sheet(128))
    scene_b, _, _, host_b = case(oracle, ("sheet-128", "B"), one_sheet(128, phase=1.4))
    keep = []
    r = host.Renderer(host_a, H.TRAVERSE_FLAT, kd_depth=8)
    try:
        before = shoot(H, r, cam_a, W, HT)
        d = device_deform(H, r.context, meshes_of(scene_b)[0], 0, keep)
        nrm = on_device(sheet(128, normals=True).normals)
        d.d_normals = nrm.data_ptr()
        assert call_deform_device(H, r.context, [d], motion_of(H, host_b, "flat", keep)) == ARG
        assert b"without normals" in H.lib().pt_last_error(r.context)
        same_render(shoot(H, r, cam_a, W, HT), before, "after the refused normals")
    finally:
        r.close()


@pytest.mark.parametrize("build,rebuild", [("host", False), ("device", True)])
@pytest.mark.parametrize("mode", MODES)
def test_instances_follow_the_one_deform(H, host, oracle, monkeypatch, mode, build, rebuild):
    device_deform_and_compare(H, host, oracle, monkeypatch, "instanced", instanced(0.0), instanced(1.9), mode, build, rebuild, differ=0.02)


@pytest.mark.parametrize("mode", MODES)
def test_only_the_mesh_named_changes(H, host, oracle, monkeypatch, mode):
    """two_sheets with the right mesh (mesh 1) named alone: the fresh render of that scene, and under the left sheet's pixels nothing has changed"""
    monkeypatch.setenv("PORTRAYER_BUILD", "device")
    key_a, key_b = ("two-sheets", (0.7, 0.0)), ("two-sheets", (0.7, 2.0))
    _, cam_a, _, host_a = case(oracle, key_a, two_sheets(0.7, 0.0))
    scene_b, cam_b, _, host_b = case(oracle, key_b, two_sheets(0.7, 2.0))
    keep = []
    r = host.Renderer(host_a, traverse(H, oracle, mode)[0], kd_depth=8)
    try:
        before = r.aov(host_glue.cam10(cam_b), W, HT, want=("depth", "node", "sub"))
        kdt = kd_of(H, host_b, keep) if mode == "kd" else None
        assert call_deform_device(H, r.context, [device_deform(H, r.context, meshes_of(scene_b)[1], 1, keep)], motion_of(H, host_b, mode, keep), kdt) == 0, H.lib().pt_last_error(r.context)
        after = r.aov(host_glue.cam10(cam_b), W, HT, want=("depth", "node", "sub"))
        got = shoot(H, r, cam_b, W, HT)
    finally:
        r.close()
    same_render(got, fresh_render(H, host, oracle, key_b, mode, "device"), f"the right sheet alone, {mode}")
    equals_oracle(got, reference(oracle, key_b, mode), f"the right sheet alone, {mode}")
    left = before["node"] == 0  # the left sheet is the first flattened node
    assert left.sum() > 50 and (before["sub"][left] >= 0).all()
    for k in ("depth", "node", "sub"):
        assert np.array_equal(before[k][left].view(np.uint8), after[k][left].view(np.uint8)), f"{mode}: {k} changed under the left sheet"
    assert not np.array_equal(before["depth"].view(np.uint64), after["depth"].view(np.uint64))


def _bent_turned_and_relit():
    scene, cam = scene_of([Node.geo(Mesh(sheet(128, phase=1.4)), RED).rotated_y(0.9).translated((0.2, 0.1, 0.0))])
    l = scene.lights[0]
    scene.lights[0] = dataclasses.replace(l, position=(l.position[0] - 5.0, l.position[1] + 1.0, l.position[2] - 2.0), color=(0.5, 0.9, 0.6))
    return scene, cam


@pytest.mark.parametrize("mode", MODES)
def test_a_node_and_a_light_move_in_the_same_call(H, host, oracle, monkeypatch, mode):
    monkeypatch.setenv("PORTRAYER_BUILD", "device")
    _, _, _, host_a = case(oracle, ("sheet-128", "A"), one_sheet(128))
    scene_b, cam_b, _, host_b = case(oracle, ("bent-turned-relit", "B"), _bent_turned_and_relit)
    assert (reference(oracle, ("sheet-128", "B"), mode).rgb != reference(oracle, ("bent-turned-relit", "B"), mode).rgb).any(axis=2).mean() >= 0.02, "the motion must show"
    keep = []
    r = host.Renderer(host_a, traverse(H, oracle, mode)[0], kd_depth=8)
    try:
        mo = motion_of(H, host_b, mode, keep)
        lights = np.ascontiguousarray([l.row() for l in scene_b.lights], dtype=np.float64)
        keep.append(lights)
        mo.lights, mo.n_lights = H._p(lights, H._dp), len(scene_b.lights)
        kdt = kd_of(H, host_b, keep) if mode == "kd" else None
        assert call_deform_device(H, r.context, [device_deform(H, r.context, meshes_of(scene_b)[0], 0, keep)], mo, kdt) == 0, H.lib().pt_last_error(r.context)
        got = shoot(H, r, cam_b, W, HT)
    finally:
        r.close()
    same_render(got, fresh_render(H, host, oracle, ("bent-turned-relit", "B"), mode, "device"), f"deform, node and light in one call, {mode}")
    equals_oracle(got, reference(oracle, ("bent-turned-relit", "B"), mode), f"deform, node and light in one call, {mode}")


# ---- 4. through the host layer and torch
def _moved_a():
    scene, cam = one_sheet(128)()
    scene.root.children[0].rotated_x(0.4).translated((0.3, -0.2, 0.1))
    return scene, cam


@pytest.mark.parametrize("mode", ["flat", "hier"])
@pytest.mark.parametrize("build,rebuild", [("host", False), ("device", True)])
def test_a_tensor_made_on_another_torch_stream(H, host, oracle, monkeypatch, mode, build, rebuild):
    """The vertices are written by torch kernels on a stream of torch's own, behind work that keeps that stream busy, immediately before the call; the test
    synchronises nothing: the library's opening hipDeviceSynchronize is what orders the read behind them. Then deform() back to A (the host layer must
    remember that its copy of the mesh is stale: A's bits equal that copy's, and without the mark nothing would be sent), then update()."""
    monkeypatch.setenv("PORTRAYER_BUILD", build)
    _, cam_a, _, host_a = case(oracle, ("sheet-128", "A"), one_sheet(128))
    scene_b, cam_b, _, host_b = case(oracle, ("sheet-128", "B"), one_sheet(128, phase=1.4))
    _, cam_m, _, host_m = case(oracle, ("sheet-128-moved", "A"), _moved_a)
    tr = traverse(H, oracle, mode)[0]
    pos_b = meshes_of(scene_b)[0].positions
    r = host.Renderer(host_a, tr, kd_depth=8)
    try:
        assert r.mesh_count() == 1 and r.mesh_vertices(0) == len(pos_b)
        shoot(H, r, cam_a, W, HT)
        half = on_device(pos_b * 0.5)  # (x / 2 + x / 2 == x exactly)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            busy = torch.ones(1 << 26, device="cuda")
            for _ in range(60):
                busy.mul_(1.0001)
            t = torch.zeros((len(pos_b), 3), dtype=torch.float64, device="cuda")
            t.add_(half).add_(half)
        r.deform_device({0: t}, rebuild=rebuild)
        same_render(shoot(H, r, cam_b, W, HT), fresh_render(H, host, oracle, ("sheet-128", "B"), mode, build), f"tensor from a side stream, {mode}, {build} build")
        assert np.array_equal(t.cpu().numpy().view(np.uint64), np.ascontiguousarray(pos_b).view(np.uint64))
        r.deform(host_a)
        same_render(shoot(H, r, cam_a, W, HT), fresh_render(H, host, oracle, ("sheet-128", "A"), mode, build), f"deform() back to A after a device deform, {mode}, {build} build")
        r.update(host_m)
        same_render(shoot(H, r, cam_m, W, HT), fresh_render(H, host, oracle, ("sheet-128-moved", "A"), mode, build), f"update() after both, {mode}, {build} build")
        # and a moved scene riding along with the tensor
        r.deform_device({0: t}, moved=host_a)
        same_render(shoot(H, r, cam_b, W, HT), fresh_render(H, host, oracle, ("sheet-128", "B"), mode, build), f"moved=, {mode}, {build} build")
    finally:
        r.close()


def test_the_host_layer_refuses_the_kd_traversal_and_several_ranks(H, host, oracle, monkeypatch):
    _, cam_a, _, host_a = case(oracle, ("sheet-128", "A"), one_sheet(128))
    t = on_device(sheet(128, phase=1.4).positions)
    r = host.Renderer(host_a, H.TRAVERSE_KD, kd_depth=8)
    try:
        before = shoot(H, r, cam_a, W, HT)
        with pytest.raises(host.PortrayerHostError, match="k-d traversal's tree is built by the host"):
            r.deform_device({0: t})
        same_render(shoot(H, r, cam_a, W, HT), before, "after the refused k-d deform")
    finally:
        r.close()
    monkeypatch.setenv("PORTRAYER_DEVICES", "0,0")
    r = host.Renderer(host_a, H.TRAVERSE_FLAT, kd_depth=8)
    try:
        assert r.ranks == 2
        with pytest.raises(host.PortrayerHostError, match="each rank's device needs its own copy"):
            r.deform_device({0: t})
    finally:
        r.close()


# ---- 5. pointers
def test_a_pointer_into_the_middle_of_an_allocation(H, host, oracle, monkeypatch):
    monkeypatch.setenv("PORTRAYER_BUILD", "device")
    L = H.lib()
    _, _, _, host_a = case(oracle, ("sheet-128", "A"), one_sheet(128))
    scene_b, cam_b, _, host_b = case(oracle, ("sheet-128", "B"), one_sheet(128, phase=1.4))
    pos = np.ascontiguousarray(meshes_of(scene_b)[0].positions, dtype=np.float64)
    keep = []
    r = host.Renderer(host_a, H.TRAVERSE_FLAT, kd_depth=8)
    try:
        ctx = r.context
        for offset, slack in ((40, 4096), (8, 0)):  # (the second: the mesh ends exactly where the allocation ends)
            base = C.c_void_p()
            assert L.pt_device_alloc(ctx, offset + pos.nbytes + slack, C.byref(base)) == 0
            inside = base.value + offset
            assert L.pt_copy_to_device(ctx, C.c_void_p(inside), pos.ctypes.data_as(C.c_void_p), pos.nbytes) == 0
            box, bad = np.zeros(6), C.c_uint64(0)
            assert L.pt_vertex_bounds_device(ctx, len(pos), C.c_void_p(inside), H._p(box, H._dp), C.byref(bad)) == 0, L.pt_last_error(ctx)
            assert np.array_equal(box.view(np.uint64), np.concatenate([pos.min(axis=0), pos.max(axis=0)]).view(np.uint64)) and bad.value == 0
            inv = np.ascontiguousarray(bbox_invtrans(box[:3], box[3:]).reshape(16))
            d = H.PtMeshDeformDevice()
            d.mesh, d.d_positions, d.bounds_invtrans, d.rebuild = 0, inside, H._p(inv, H._dp), 0
            assert call_deform_device(H, ctx, [d], motion_of(H, host_b, "flat", keep)) == 0, L.pt_last_error(ctx)
            assert L.pt_device_free(ctx, base) == 0  # the caller's buffer is free again when the call returns
            same_render(shoot(H, r, cam_b, W, HT), fresh_render(H, host, oracle, ("sheet-128", "B"), "flat", "device"), f"a pointer {offset} bytes into its allocation")
    finally:
        r.close()


def test_pinned_host_memory_is_refused_by_both_entry_points(H, host, oracle, monkeypatch):
    """pinned, so that the GPU could read it even if the check were missing: this test cannot fault a machine"""
    L = H.lib()
    _, cam_a, _, host_a = case(oracle, ("sheet-128", "A"), one_sheet(128))
    scene_b, _, _, host_b = case(oracle, ("sheet-128", "B"), one_sheet(128, phase=1.4))
    pos = meshes_of(scene_b)[0].positions
    pinned = torch.empty((len(pos), 3), dtype=torch.float64).pin_memory()
    pinned.copy_(torch.from_numpy(np.ascontiguousarray(pos)))
    assert pinned.is_pinned()
    keep = []
    r = host.Renderer(host_a, H.TRAVERSE_FLAT, kd_depth=8)
    try:
        before = shoot(H, r, cam_a, W, HT)
        box, bad = np.zeros(6), C.c_uint64(0)
        assert L.pt_vertex_bounds_device(r.context, len(pos), C.c_void_p(pinned.data_ptr()), H._p(box, H._dp), C.byref(bad)) == ARG
        assert b"not device memory" in L.pt_last_error(r.context)
        inv = np.ascontiguousarray(bbox_invtrans(pos.min(axis=0), pos.max(axis=0)).reshape(16))
        d = H.PtMeshDeformDevice()
        d.mesh, d.d_positions, d.bounds_invtrans, d.rebuild = 0, pinned.data_ptr(), H._p(inv, H._dp), 0
        assert call_deform_device(H, r.context, [d], motion_of(H, host_b, "flat", keep)) == ARG
        assert b"not device memory" in L.pt_last_error(r.context)
        same_render(shoot(H, r, cam_a, W, HT), before, "after the refused pinned buffer")
        with pytest.raises(ValueError):
            r.deform_device({0: pinned})
    finally:
        r.close()


# ---- 6. refusals leave the scene as it was
@pytest.mark.parametrize("mode", MODES)
def test_refusals_leave_the_scene_usable(H, host, oracle, monkeypatch, mode):
    monkeypatch.setenv("PORTRAYER_BUILD", "device")  # mesh 0 (128 triangles) is device-built, mesh 2 (15) host-built; mesh 1 has a KDMesh tree
    L = H.lib()
    _, cam_a, _, host_a = case(oracle, ("errors", "A"), _with_a_kdmesh(0.0))
    scene_b, cam_b, _, host_b = case(oracle, ("errors", "B"), _with_a_kdmesh(1.4))
    mb = meshes_of(scene_b)
    keep = []
    kdt = kd_of(H, host_b, keep) if mode == "kd" else None
    good = lambda: motion_of(H, host_b, mode, keep)  # noqa: E731
    r = host.Renderer(host_a, traverse(H, oracle, mode)[0], kd_depth=8)
    try:
        before = shoot(H, r, cam_a, W, HT)
        ctx = r.context

        def refused(deforms, says):
            rc = call_deform_device(H, ctx, deforms, good(), kdt)
            assert rc == ARG, (rc, L.pt_last_error(ctx))
            assert says in L.pt_last_error(ctx), L.pt_last_error(ctx)
        ok = lambda **kw: device_deform(H, ctx, mb[0], 0, keep, **kw)  # noqa: E731
        nan = mb[0].positions.copy(); nan[-1, 2] = np.nan
        t = on_device(nan)
        keep.append(t)
        d = ok(); d.d_positions = t.data_ptr()
        refused([d], b"not finite")
        same_render(shoot(H, r, cam_a, W, HT), before, f"after the refused NaN, {mode}")
        d = ok(); d.d_positions = None
        refused([d], b"required")
        d = ok(); d.bounds_invtrans = None
        refused([d], b"required")
        refused([ok(), ok()], b"twice")
        d = ok(); d.mesh = 3
        refused([d], b"out of range")
        refused([device_deform(H, ctx, mb[2], 2, keep, rebuild=1)], b"built on the host")
        refused([device_deform(H, ctx, mb[1], 1, keep)], b"KDMesh")
        far = on_device(mb[0].positions * 1e19)
        keep.append(far)
        d = ok(); d.d_positions = far.data_ptr()
        refused([d], b"1e18")
        # a pass in flight: refused until its _finish
        o = np.ascontiguousarray(np.tile([0.0, 0.0, 50.0], (64, 1))); dd = np.ascontiguousarray(np.tile([0.0, 0.0, -1.0], (64, 1)))
        d_o, d_d, d_t = C.c_void_p(), C.c_void_p(), C.c_void_p()
        for ptr, nbytes in ((d_o, o.nbytes), (d_d, dd.nbytes), (d_t, 64 * 8)):
            assert L.pt_device_alloc(ctx, nbytes, C.byref(ptr)) == 0
        assert L.pt_copy_to_device(ctx, d_o, o.ctypes.data_as(C.c_void_p), o.nbytes) == 0 and L.pt_copy_to_device(ctx, d_d, dd.ctypes.data_as(C.c_void_p), dd.nbytes) == 0
        waiting = ok()
        rp = H.PtRaysParams(64, 0, 0)
        rb = H.PtRaysBuffers(); rb.t = C.cast(d_t, H._dp)
        assert L.pt_rays_device(ctx, C.byref(rp), d_o, d_d, C.byref(rb), None) == 0
        refused([waiting], b"in flight")
        assert L.pt_rays_finish(ctx, None) == 0
        same_render(shoot(H, r, cam_a, W, HT), before, f"after the refused deforms, {mode}")  # every refusal came before the first write
        scene_c, cam_c, _, host_c = case(oracle, ("errors", "C"), lambda: _with_a_kdmesh(1.4, kd_phase=0.0)())
        assert call_deform_device(H, ctx, [waiting, device_deform(H, ctx, meshes_of(scene_c)[2], 2, keep)], motion_of(H, host_c, mode, keep),
                                  kd_of(H, host_c, keep) if mode == "kd" else None) == 0, L.pt_last_error(ctx)
        for ptr in (d_o, d_d, d_t):
            assert L.pt_device_free(ctx, ptr) == 0
        got = shoot(H, r, cam_c, W, HT)
    finally:
        r.close()
    same_render(got, fresh_render(H, host, oracle, ("errors", "C"), mode, "device"), f"after pt_rays_finish, {mode}")
    equals_oracle(got, reference(oracle, ("errors", "C"), mode), f"after pt_rays_finish, {mode}")


# ---- 7. memory
@pytest.mark.parametrize("smooth", [False, True])
def test_no_staging_buffer_and_no_growth(H, host, oracle, monkeypatch, smooth):
    monkeypatch.setenv("PORTRAYER_BUILD", "device")
    name = "smooth" if smooth else "sheet-128"
    _, _, _, host_a = case(oracle, (name, "A"), one_sheet(128, smooth=smooth))
    scene_b, _, _, host_b = case(oracle, (name, "B"), one_sheet(128, smooth=smooth, phase=1.4))
    mesh = meshes_of(scene_b)[0]
    assert (mesh.normals is not None) == smooth
    keep = []
    from_device, from_host = host.Renderer(host_a, H.TRAVERSE_FLAT, kd_depth=8), host.Renderer(host_a, H.TRAVERSE_FLAT, kd_depth=8)
    try:
        sizes = []
        for _ in range(5):
            assert call_deform_device(H, from_device.context, [device_deform(H, from_device.context, mesh, 0, keep)], motion_of(H, host_b, "flat", keep)) == 0
            sizes.append(H.lib().pt_test_scene_bytes(from_device.context))
        assert sizes[0] == sizes[4], f"device deforms of the same mesh made the context's scene buffers grow: {sizes}"
        assert call_deform(H, from_host.context, [raw_deform(H, mesh, 0, keep)], motion_of(H, host_b, "flat", keep)) == 0
        staged = H.lib().pt_test_scene_bytes(from_host.context)
        stage_bytes = len(mesh.positions) * (48 if smooth else 24)
        assert staged - sizes[0] >= stage_bytes, f"the device path holds {sizes[0]} bytes, the host path {staged}: less than the staging buffer's {stage_bytes} apart"
    finally:
        from_device.close(); from_host.close()
