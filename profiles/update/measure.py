#!/usr/bin/env python3
"""What moving a scene costs, against uploading it again: python3 profiles/update/measure.py [out.json]

Per scene and traversal (flat_scene, hierarchical), host wall time around the synchronous call, median of 20 after 3 warm-ups:
  upload         pt_scene_upload (a new Renderer on the scene; the Renderer's own steady-clock timer around that one call,
                 prepare_ms()["upload_and_device_trees"]: the same wall time as below less the ctypes call's few microseconds, which the
                 millisecond-scale figures here do not resolve)
  update host    pt_scene_update with PORTRAYER_BUILD=host   (the scene-level tree by pt_bvh_build)
  update device  pt_scene_update with PORTRAYER_BUILD=device (pt_device_build_scene_tree)
Scenes: big-scene, macho-cows, big-mesh (216 cow instances), big-soup; then n unit spheres on a jittered grid for n = 1e3, 1e4, 1e5, 1e6 (flat_scene
only): where the device builder overtakes the host's is where PORTRAYER_BUILD=auto should switch (PORTRAYER_BUILD_MIN, 65536 today). Last, big-scene
at 1920x1080, samples = 1, on each builder's tree: kernel_ms of 20 renders, the walk-quality cost of the clustering tree at scene level.
One process, the variants alternating inside one loop, so that clocks and caches are shared fairly."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from portrayer_amd import _hip as H  # noqa: E402
from portrayer_amd import host  # noqa: E402

WARM, TIMED = 3, 20


def motion(hs, hier, keep):
    f = hs.flatten()
    arrays = [np.ascontiguousarray(f[k].reshape(-1, 16)) for k in ("trans", "invtrans", "normal_trans")]
    mo = H.PtSceneMotion()
    mo.n_nodes = len(arrays[0])
    mo.trans, mo.invtrans, mo.normal_trans = (H._p(a, H._dp) for a in arrays)
    if hier:
        g = hs.graph()
        ga = [np.ascontiguousarray(g[k].reshape(-1, 16)) for k in ("trans", "invtrans", "normal_trans")]
        mo.n_graph_nodes = len(ga[0])
        mo.graph_trans, mo.graph_invtrans, mo.graph_normal_trans = (H._p(a, H._dp) for a in ga)
        arrays += ga
    keep.append(arrays)
    return mo


def med(v):
    v = np.sort(np.asarray(v))
    return dict(median=float(np.median(v)), min=float(v[0]), max=float(v[-1]))


def measure(hs, tr, uploads=True):
    keep, out = [], {}
    mo = motion(hs, tr == H.TRAVERSE_HIER, keep)
    r = host.Renderer(hs, tr)
    times = {"upload": [], "update host": [], "update device": []}
    for k in range(WARM + TIMED):
        if uploads:
            fresh = host.Renderer(hs, tr)
            ms = fresh.prepare_ms()["upload_and_device_trees"]
            fresh.close()
            if k >= WARM:
                times["upload"].append(ms)
        for name, mode in (("update host", "host"), ("update device", "device")):
            os.environ["PORTRAYER_BUILD"] = mode
            t0 = time.perf_counter()
            rc = H.lib().pt_scene_update(r.context, C.byref(mo), None)
            ms = (time.perf_counter() - t0) * 1e3
            assert rc == 0, H.lib().pt_last_error(r.context)
            if k >= WARM:
                times[name].append(ms)
        os.environ.pop("PORTRAYER_BUILD", None)
    for name, v in times.items():
        if v:
            out[name] = med(v)
    return r, mo, out


def spheres(n):
    from scene_dsl import Light, Material, Node, Scene, Sphere
    import host_glue
    rng = np.random.default_rng(3)
    side = int(np.ceil(n ** (1 / 3)))
    mat = Material(diffuse=(0.7, 0.7, 0.7))
    p = rng.uniform(-0.3, 0.3, size=(n, 3))
    kids = [Node.geo(Sphere(), mat).translated((2.5 * (i % side) + p[i, 0], 2.5 * ((i // side) % side) + p[i, 1], 2.5 * (i // (side * side)) + p[i, 2])) for i in range(n)]
    return host_glue.host_scene(Scene(root=Node.group(kids), lights=[Light(position=(0.0, 1e4, 1e4), color=(1.0, 1.0, 1.0))], ambient=(0.1, 0.1, 0.1)))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    import host_glue
    from example_scenes import big_mesh, big_soup
    result = {"warm": WARM, "timed": TIMED, "scenes": {}, "sweep": {}}
    scenes = {"big-scene": host.Scene.example("big-scene"), "macho-cows": host.Scene.example("macho-cows"),
              "big-mesh": host_glue.host_scene(big_mesh()[0]), "big-soup": host_glue.host_scene(big_soup()[0])}
    for name, hs in scenes.items():
        result["scenes"][name] = {}
        for tname, tr in (("flat", H.TRAVERSE_FLAT), ("hier", H.TRAVERSE_HIER)):
            r, _, row = measure(hs, tr)
            r.close()
            result["scenes"][name][tname] = row
            print(name, tname, json.dumps(row), flush=True)
    for n in (1000, 10000, 100000, 1000000):
        r, _, row = measure(spheres(n), H.TRAVERSE_FLAT, uploads=n <= 100000)
        r.close()
        result["sweep"][str(n)] = row
        print("spheres", n, json.dumps(row), flush=True)
    sc = scenes["big-scene"]
    r, mo, _ = measure(sc, H.TRAVERSE_FLAT, uploads=False)
    bg = np.zeros((1080, 3))
    walk = {"host": [], "device": []}
    for k in range(WARM + TIMED):
        for mode in walk:
            os.environ["PORTRAYER_BUILD"] = mode
            assert H.lib().pt_scene_update(r.context, C.byref(mo), None) == 0
            _, _, st = r.render(sc.camera, 1920, 1080, bg, samples=1, want_linear=False)
            if k >= WARM:
                walk[mode].append(st["kernel_ms"])
    os.environ.pop("PORTRAYER_BUILD", None)
    r.close()
    result["big-scene 1920x1080 samples=1 kernel_ms"] = {k: med(v) for k, v in walk.items()}
    print(json.dumps(result["big-scene 1920x1080 samples=1 kernel_ms"]), flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
