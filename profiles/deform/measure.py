#!/usr/bin/env python3
"""What deforming a mesh costs, against uploading the deformed scene again: python3 profiles/deform/measure.py [out.json]

For macho-cows and big-soup (1.25 M triangles in one mesh), flat_scene traversal, PORTRAYER_BUILD as the environment says (unset: auto - macho-cows'
trees are built on the host, big-soup's on the device), every mesh's vertices displaced by a smooth function of position whose phase changes per step:
  upload        a new Renderer on the deformed scene: its own steady-clock timer around pt_scene_upload (prepare_ms()["upload_and_device_trees"])
  deform refit  host wall time around pt_scene_deform, rebuild = 0, through the C ABI (the arrays are prepared outside the timer)
  deform rebuild the same with rebuild = 1, where the device built the tree
  frame         kernel_ms of a 1920x1080, samples = 1 render on the refitted tree, on the rebuilt tree and on the freshly uploaded one
Median of 10 after 2 warm-ups; the variants alternate inside one loop."""
import ctypes as C
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import host_glue  # noqa: E402
from device_glue import bbox_invtrans  # noqa: E402
from example_scenes import big_soup, macho_cows  # noqa: E402
from portrayer_amd import _hip as H  # noqa: E402
from portrayer_amd import host  # noqa: E402
from scene_dsl import default_background  # noqa: E402

WARM, TIMED = 2, 10
W, HT = 1920, 1080


def meshes_of(scene):
    out, seen, level = [], set(), [scene.root]
    while level:
        nxt = []
        for node in level:
            if node.geometry is not None and node.geometry[0].mesh is not None and id(node.geometry[0].mesh) not in seen:
                seen.add(id(node.geometry[0].mesh)); out.append(node.geometry[0].mesh)
            nxt += node.children
        level = nxt
    return out


def displaced(make, phase):
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
                new[id(m)] = dataclasses.replace(m, positions=np.ascontiguousarray(m.positions + 0.03 * ext * np.sin(4.0 * m.positions[:, [1, 2, 0]] / ext + phase)))
            node.geometry = (dataclasses.replace(prim, mesh=new[id(m)]), mat)
        for c in node.children:
            walk(c)
    if phase is not None:
        walk(scene.root)
    return scene, cam


def motion(hs, keep):
    f = hs.flatten()
    arrays = [np.ascontiguousarray(f[k].reshape(-1, 16)) for k in ("trans", "invtrans", "normal_trans")]
    mo = H.PtSceneMotion()
    mo.n_nodes = len(arrays[0])
    mo.trans, mo.invtrans, mo.normal_trans = (H._p(a, H._dp) for a in arrays)
    keep.append(arrays)
    return mo


def deforms_of(scene, rebuild, allowed, keep):
    out = []
    for i, m in enumerate(meshes_of(scene)):
        d = H.PtMeshDeform()
        pos = np.ascontiguousarray(m.positions, dtype=np.float64)
        box = np.ascontiguousarray(bbox_invtrans(pos.min(axis=0), pos.max(axis=0)).reshape(16))
        keep.append((pos, box))
        d.mesh, d.positions, d.bounds_invtrans, d.rebuild = i, H._p(pos, H._dp), H._p(box, H._dp), 1 if rebuild and allowed[i] else 0
        out.append(d)
    return (H.PtMeshDeform * len(out))(*out), len(out)


def med(v):
    v = np.sort(np.asarray(v))
    return dict(median=float(np.median(v)), min=float(v[0]), max=float(v[-1])) if len(v) else None


def measure(name, make):
    scene_a, cam = displaced(make, None)
    r = host.Renderer(host_glue.host_scene(scene_a), H.TRAVERSE_FLAT)
    allowed = [H.lib().pt_scene_mesh_rebuildable(r.context, i) == 1 for i in range(len(meshes_of(scene_a)))]
    bg = default_background(W, HT)
    times = {"upload": [], "deform refit": [], "deform rebuild": [], "frame refit": [], "frame rebuild": [], "frame fresh": []}
    L = H.lib()
    for k in range(WARM + TIMED):
        scene_b, _ = displaced(make, 0.3 * (k + 1))
        hs_b = host_glue.host_scene(scene_b)
        keep = []
        mo = motion(hs_b, keep)
        row = {}
        for what, rebuild in (("refit", False), ("rebuild", True)):
            if rebuild and not any(allowed):
                continue
            arr, n = deforms_of(scene_b, rebuild, allowed, keep)
            t0 = time.perf_counter()
            rc = L.pt_scene_deform(r.context, n, arr, C.byref(mo), None)
            row["deform " + what] = (time.perf_counter() - t0) * 1e3
            assert rc == 0, L.pt_last_error(r.context)
            row["frame " + what] = r.render(host_glue.cam10(cam), W, HT, bg, samples=1, seed=1, sample_mode=H.SAMPLE_CENTRE, want_linear=False)[2]["kernel_ms"]
        fresh = host.Renderer(hs_b, H.TRAVERSE_FLAT)
        row["upload"] = fresh.prepare_ms()["upload_and_device_trees"]
        row["frame fresh"] = fresh.render(host_glue.cam10(cam), W, HT, bg, samples=1, seed=1, sample_mode=H.SAMPLE_CENTRE, want_linear=False)[2]["kernel_ms"]
        fresh.close()
        if k >= WARM:
            for key, v in row.items():
                times[key].append(v)
    r.close()
    return dict(scene=name, triangles=[len(m.triangles) for m in meshes_of(scene_a)], device_built=allowed, ms={k: med(v) for k, v in times.items()})


if __name__ == "__main__":
    results = [measure("macho-cows", macho_cows), measure("big-soup", big_soup)]
    text = json.dumps(dict(build=os.environ.get("PORTRAYER_BUILD", "auto"), results=results), indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(text)
