#!/usr/bin/env python3
"""What the chart pass costs: python3 profiles/chart/measure.py [--case NAME] [--reps 5] [--no-host] [--no-compose] [--out F.json]   (needs a GPU)
                              python3 profiles/chart/measure.py --oracle                                                       (needs none)

Cases: teapot (teapot.obj, 6,320 triangles) and big-soup (1,253,664 triangles in one mesh); the UV set is GENERATED: triangle t gets a cell of its own in a
square atlas of ceil(sqrt(T / 2)) cells a side, two triangles per cell with a margin - every triangle small and every texel's owner unique. One more case,
`one`, is a single triangle over the whole map: the own kernel's split path alone. Maps of 1024 x 1024 and 4096 x 4096. Per case and size, kernel times
between HIP events (pt_chart_device ... pt_aov_finish), the variants alternating inside one loop after two warm-up rounds, median [min .. max] of --reps:
  all      the three kernels
  own      seed + own      (PORTRAYER_CHART_PHASES=1)
  resolve  resolve alone   (PORTRAYER_CHART_PHASES=2, over the owner map the round's `own` left)
and, unless --no-compose, at 1024 x 1024 x 16 rays: Renderer.ao_chart and gather_chart (wall time, and the AO / gather pass's kernel time) against Renderer.ao
and gather's kernel time on the same points; unless --no-host the host path: pt_test_chart_host's wall time plus the upload of position and normal
(pt_copy_to_device of W x H x 48 bytes).
--oracle: the cross-check's tolerance (tests/test_gpu_chart.py): on the rays from P + 0.5 N along -N, for the cube's and the grid's texels well inside their
triangle at 67 x 37, the largest deviation of the oracle's hit point (po_cast_rays) from P."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

SIZES = ((1024, 1024), (4096, 4096))


def summary(v):
    v = np.asarray(v)
    return dict(min=float(v.min()), median=float(np.median(v)), max=float(v.max()), n=int(len(v)))


def atlas_uv(n_tris):
    side = int(np.ceil(np.sqrt(n_tris / 2.0)))
    t = np.arange(n_tris)
    cell, half = t // 2, t % 2
    cx, cy = (cell % side).astype(np.float64), (cell // side).astype(np.float64)
    lo, hi = 0.05, 0.95
    a = np.stack([cx + lo, cy + lo], axis=1)
    b = np.stack([cx + hi, cy + lo], axis=1)
    c = np.stack([cx + hi, cy + hi], axis=1)
    d = np.stack([cx + lo, cy + hi], axis=1)
    uv = np.where(half[:, None] == 0, np.concatenate([a, b, c], axis=1), np.concatenate([a, c, d], axis=1))
    return np.ascontiguousarray(uv / side)


def oracle_deviation():
    import chart_restate as R
    import host_glue
    import oracle_lib as O
    import test_gpu_chart as T
    from scene_dsl import Mesh, Node
    for which in ("cube", "grid"):
        if which == "cube":
            mesh = T.cube_mesh()
            uv = mesh.tex_coords[mesh.triangles.astype(np.int64)].reshape(-1, 6)
        else:
            v, n, uv, _ = T.CASES["grid"]
            mesh = T.corner_mesh(v, n)
        scene = T.under_a_group([Node.geo(Mesh(mesh, False), T.RED)])
        hs = host_glue.host_scene(scene)
        node = T.mesh_nodes(hs)[0]
        want = T.expected(hs, node, mesh, False, uv, 67, 37)
        inside = (R.min_weight_ratio(uv, 67, 37, want["tri"]) >= 2.0 ** -10).ravel()
        P, N = want["position"].reshape(-1, 3)[inside], want["normal"].reshape(-1, 3)[inside]
        t, ids, pt, _ = O.cast_rays(scene, P + T.LIFT * N, -N)
        assert np.all(ids == node)
        print("%s: %d rays, the oracle's hit point deviates from P by at most %.3g; x 64 = %.3g" % (which, len(P), np.max(np.abs(pt - P)), 64 * np.max(np.abs(pt - P))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-compose", action="store_true")
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.oracle:
        return oracle_deviation()
    import torch
    import host_glue
    from example_scenes import big_soup, load_mesh
    from portrayer_amd import _hip as H
    from portrayer_amd import host
    from scene_dsl import Light, Material, Mesh, MeshData, Node, Scene
    lib = H.lib()
    dev = torch.device("cuda", 0)
    mat = Material(diffuse=(0.7, 0.6, 0.5))
    report = {}
    for case in args.case or ["teapot", "big-soup", "one"]:
        if case == "teapot":
            mesh = load_mesh("teapot.obj")
            scene = Scene(root=Node.group([Node.geo(Mesh(mesh), mat)]), lights=[Light(position=(3.0, 4.0, 9.0), color=(0.9, 0.9, 0.9))], ambient=(0.2, 0.2, 0.2))
        elif case == "big-soup":
            scene = big_soup()[0]
            mesh = scene.root.children[0].geometry[0].mesh
        else:
            mesh = MeshData(np.array([[-1.0, -1.0, 0.0], [3.0, -1.0, 0.0], [-1.0, 3.0, 0.5]]), np.array([[0, 1, 2]], dtype=np.uint32), None, "one")
            scene = Scene(root=Node.group([Node.geo(Mesh(mesh), mat)]), lights=[Light(position=(3.0, 4.0, 9.0), color=(0.9, 0.9, 0.9))], ambient=(0.2, 0.2, 0.2))
        n_tris = len(mesh.triangles)
        uv = atlas_uv(n_tris) if case != "one" else np.array([[-0.5, -0.5, 2.5, -0.5, -0.5, 2.5]])
        hs = host_glue.host_scene(scene)
        r = host.Renderer(hs, H.TRAVERSE_FLAT)
        cx = r.context
        node = [int(i) for i in np.nonzero(np.isin(hs.flatten()["prim_type"], (2, 3)))[0]][0]
        d_uv = torch.from_numpy(uv).to(dev)
        report[case] = {"triangles": n_tris}
        for (w, h) in SIZES:
            d_pos = torch.zeros((h, w, 3), dtype=torch.float64, device=dev)
            d_nrm = torch.zeros((h, w, 3), dtype=torch.float64, device=dev)
            b = H.PtChartBuffers(C.cast(C.c_void_p(d_pos.data_ptr()), H._dp), C.cast(C.c_void_p(d_nrm.data_ptr()), H._dp), None, None)
            p = H.PtChartParams(node, w, h, 0)
            times = {"all": [], "own": [], "resolve": []}
            for rep in range(args.reps + 2):
                for name, phases in (("all", None), ("own", "1"), ("resolve", "2")):
                    if phases is None:
                        os.environ.pop("PORTRAYER_CHART_PHASES", None)
                    else:
                        os.environ["PORTRAYER_CHART_PHASES"] = phases
                    ms = C.c_double(0.0)
                    assert lib.pt_chart_device(cx, C.byref(p), C.c_void_p(d_uv.data_ptr()), C.byref(b), None) == H.OK, lib.pt_last_error(cx)
                    assert lib.pt_aov_finish(cx, C.byref(ms)) == H.OK, lib.pt_last_error(cx)
                    if rep >= 2:
                        times[name].append(ms.value)
            os.environ.pop("PORTRAYER_CHART_PHASES", None)
            covered = int((d_nrm.abs().sum(dim=2) > 0).sum().item())
            entry = {k: summary(v) for k, v in times.items()}
            entry["covered"] = covered
            if not args.no_host and case != "big-soup" and w == 1024:
                fl = hs.flatten()
                fwd, nrm = np.ascontiguousarray(fl["trans"][node][:3, :4].reshape(12)), np.ascontiguousarray(fl["normal_trans"][node][:3, :3].reshape(9))
                tri_v = np.ascontiguousarray(mesh.positions[mesh.triangles.astype(np.int64)].reshape(-1, 9))
                pos, nor = np.zeros((h, w, 3)), np.zeros((h, w, 3))
                hb = H.PtChartBuffers(H._p(pos, H._dp), H._p(nor, H._dp), None, None)
                t0 = time.perf_counter()
                assert lib.pt_test_chart_host(H._p(fwd, H._dp), H._p(nrm, H._dp), n_tris, H._p(tri_v, H._dp), None, H._p(uv, H._dp), w, h, 0, C.byref(hb)) == 0
                t1 = time.perf_counter()
                d_pos.copy_(torch.from_numpy(pos)); d_nrm.copy_(torch.from_numpy(nor)); torch.cuda.synchronize()
                t2 = time.perf_counter()
                entry["host_ms"] = dict(replay=(t1 - t0) * 1e3, upload=(t2 - t1) * 1e3)
                assert pos.tobytes() == r.chart(node, w, h, uv, want=("position",))["position"].tobytes()
            if not args.no_compose and w == 1024 and case != "one":
                comp = {"ao_chart_wall": [], "ao_chart_kernel": [], "ao_kernel": [], "gather_chart_wall": [], "gather_chart_kernel": [], "gather_kernel": []}
                ch = r.chart(node, w, h, uv, want=("position", "normal"))
                P, N = ch["position"].reshape(-1, 3), ch["normal"].reshape(-1, 3)
                for rep in range(min(args.reps, 3) + 1):
                    t0 = time.perf_counter(); a = r.ao_chart(node, w, h, uv, samples=16, radius=2.0, bias=1e-3, seed=7); t1 = time.perf_counter()
                    o = r.ao(P, N, samples=16, radius=2.0, bias=1e-3, seed=7)
                    t2 = time.perf_counter(); g = r.gather_chart(node, w, h, (0.25, 0.5, 1.0), uv, samples=16, bias=1e-3, seed=7); t3 = time.perf_counter()
                    q = r.gather(P, N, (0.25, 0.5, 1.0), samples=16, bias=1e-3, seed=7)
                    assert a["occluded"].tobytes() == o["occluded"].tobytes() and g["sum"].tobytes() == q["sum"].tobytes()
                    if rep >= 1:
                        comp["ao_chart_wall"].append((t1 - t0) * 1e3); comp["ao_chart_kernel"].append(a["kernel_ms"]); comp["ao_kernel"].append(o["kernel_ms"])
                        comp["gather_chart_wall"].append((t3 - t2) * 1e3); comp["gather_chart_kernel"].append(g["kernel_ms"]); comp["gather_kernel"].append(q["kernel_ms"])
                entry["compose"] = {k: summary(v) for k, v in comp.items()}
            report[case]["%dx%d" % (w, h)] = entry
            print(case, "%dx%d" % (w, h), json.dumps(entry), flush=True)
            del d_pos, d_nrm
        r.close()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
