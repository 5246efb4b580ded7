#!/usr/bin/env python3
"""What deforming a mesh from vertices in device memory costs, against sending them from the host: python3 profiles/deform/measure_device.py [out.json]

A sheet (grid of quads, z = a sin(k x + phase)) of 2e3, 2e5 and 1.25e6 triangles in the flat_scene traversal, PORTRAYER_BUILD=device (so that every tree can
also be rebuilt), the same numbers on both paths, through the C ABI with the arrays prepared outside the timers:
  host deform      wall time of pt_scene_deform with the vertices in a numpy array (the parent commit's path: the yardstick)
  device bounds    wall time of pt_vertex_bounds_device on the torch tensor holding the same values
  device deform    wall time of pt_scene_deform_device on that tensor (it computes the box again)
  device total     the two device calls added up: what a caller pays per frame
each with rebuild = 0 (refit) and rebuild = 1, 20 calls after 3 warm-up calls, the variants alternating inside one loop; median, min and max.
The reduction alone: the bandwidth of pt_vertex_bounds_device (24 bytes per vertex over its wall time, its synchronisation and the copy of the result
included) beside pt_measure_copy_bandwidth of the same byte count (read + write counted)."""
import ctypes as C
import json
import os
import sys
import time

os.environ["PORTRAYER_BUILD"] = "device"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import host_glue  # noqa: E402
from device_glue import bbox_invtrans  # noqa: E402
from portrayer_amd import _hip as H  # noqa: E402
from portrayer_amd import host  # noqa: E402
from scene_dsl import Light, Material, Mesh, MeshData, Node, Scene  # noqa: E402

WARM, TIMED = 3, 20
SIZES = (2_000, 200_000, 1_250_000)


def sheet(tris, phase):
    n = max(1, int(np.ceil(np.sqrt(tris / 2.0))))
    xs = np.linspace(-1.5, 1.5, n + 1)
    x, y = np.meshgrid(xs, xs)
    x, y = x.ravel(), y.ravel()
    pos = np.stack([x, y, 0.35 * np.sin(2.2 * x + 0.7 * y + phase)], axis=1).astype(np.float64)
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (j * (n + 1) + i).ravel()
    idx = np.stack([np.stack([a, a + 1, a + n + 2], axis=1), np.stack([a, a + n + 2, a + n + 1], axis=1)], axis=1).reshape(-1, 3)
    return MeshData(np.ascontiguousarray(pos), np.ascontiguousarray(idx[:tris], dtype=np.uint32), None, "sheet")


def scene_of(mesh):
    red = Material(diffuse=(0.8, 0.25, 0.2), specular=(0.5, 0.5, 0.5), shininess=40.0)
    return Scene(root=Node.group([Node.geo(Mesh(mesh), red)]), lights=[Light(position=(3.0, 4.0, 9.0), color=(0.9, 0.9, 0.9))], ambient=(0.15, 0.15, 0.15))


def motion(hs, keep):
    f = hs.flatten()
    arrays = [np.ascontiguousarray(f[k].reshape(-1, 16)) for k in ("trans", "invtrans", "normal_trans")]
    mo = H.PtSceneMotion()
    mo.n_nodes = len(arrays[0])
    mo.trans, mo.invtrans, mo.normal_trans = (H._p(a, H._dp) for a in arrays)
    keep.append(arrays)
    return mo


def med(v):
    v = np.sort(np.asarray(v))
    return dict(median=float(np.median(v)), min=float(v[0]), max=float(v[-1]))


def measure(tris):
    L = H.lib()
    hs = host_glue.host_scene(scene_of(sheet(tris, 0.0)))
    r = host.Renderer(hs, H.TRAVERSE_FLAT)
    ctx = r.context
    assert L.pt_scene_mesh_rebuildable(ctx, 0) == 1
    keep = []
    mo = motion(hs, keep)
    times = {f"{what} {how}": [] for what in ("host deform", "device bounds", "device deform", "device total") for how in ("refit", "rebuild")}
    n_verts = 0
    for k in range(WARM + TIMED):
        pos = sheet(tris, 0.3 * (k + 1)).positions
        n_verts = len(pos)
        t = torch.tensor(pos, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        inv = np.ascontiguousarray(bbox_invtrans(pos.min(axis=0), pos.max(axis=0)).reshape(16))
        row = {}
        for how, rebuild in (("refit", 0), ("rebuild", 1)):
            d = H.PtMeshDeform()
            d.mesh, d.positions, d.bounds_invtrans, d.rebuild = 0, H._p(pos, H._dp), H._p(inv, H._dp), rebuild
            t0 = time.perf_counter()
            rc = L.pt_scene_deform(ctx, 1, C.byref(d), C.byref(mo), None)
            row["host deform " + how] = (time.perf_counter() - t0) * 1e3
            assert rc == 0, L.pt_last_error(ctx)
            box, bad = np.zeros(6), C.c_uint64(0)
            t0 = time.perf_counter()
            rc = L.pt_vertex_bounds_device(ctx, n_verts, C.c_void_p(t.data_ptr()), H._p(box, H._dp), C.byref(bad))
            row["device bounds " + how] = (time.perf_counter() - t0) * 1e3
            assert rc == 0 and bad.value == 0, L.pt_last_error(ctx)
            inv_d = np.ascontiguousarray(bbox_invtrans(box[:3], box[3:]).reshape(16))
            dd = H.PtMeshDeformDevice()
            dd.mesh, dd.d_positions, dd.bounds_invtrans, dd.rebuild = 0, t.data_ptr(), H._p(inv_d, H._dp), rebuild
            t0 = time.perf_counter()
            rc = L.pt_scene_deform_device(ctx, 1, C.byref(dd), C.byref(mo), None)
            row["device deform " + how] = (time.perf_counter() - t0) * 1e3
            assert rc == 0, L.pt_last_error(ctx)
            row["device total " + how] = row["device bounds " + how] + row["device deform " + how]
        if k >= WARM:
            for key, v in row.items():
                times[key].append(v)
    nbytes = 24 * n_verts
    bounds_ms = np.median(times["device bounds refit"] + times["device bounds rebuild"])
    copy = C.c_double(0.0)
    assert L.pt_measure_copy_bandwidth(ctx, nbytes, 5, C.byref(copy)) == 0
    r.close()
    return dict(triangles=tris, vertices=n_verts, vertex_bytes=nbytes, ms={k: med(v) for k, v in times.items()},
                reduction_gbps=nbytes / (bounds_ms * 1e-3) / 1e9, copy_gbps_same_bytes=copy.value)


if __name__ == "__main__":
    text = json.dumps(dict(build=os.environ["PORTRAYER_BUILD"], warm=WARM, timed=TIMED, results=[measure(n) for n in SIZES]), indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(text)
