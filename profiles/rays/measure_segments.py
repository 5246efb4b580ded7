#!/usr/bin/env python3
"""What a bound per ray buys ambient-occlusion rays: python3 profiles/rays/measure_segments.py [repetitions per variant, default 7] [out.json] [--rays N]

big-scene and macho-cows in the flat_scene and hierarchical semantics (the k-d semantics filter an unbounded walk: nothing to gain, by contract). The rays:
2^22 (--rays) ambient-occlusion rays - origins drawn with a seed from the surface points of a 1920x1080 pt_aov pass, unit directions uniform over the hemisphere
about the point's normal - in that random order, resident on the GPU with their results. Lengths L = 2 %, 10 % and 50 % of the diagonal of the scene's box.
Kernel times from the passes' own HIP events, every variant warmed twice first, all variants alternating inside one loop of ONE process:
  a  r0 / r1      pt_rays_device, any_hit = 0, `t` only: what a caller had to do before there was a bound (and then compare t with L), reorder 0 / 1
  b L r0 / r1     pt_segments_device, any_hit = 0, `t` only, t_max = L
  c L r0 / r1     pt_segments_device, any_hit = 1 (`occluded`), t_max = L
Reported per variant: median [min .. max] of the repetitions; for (a) also the medians of the two halves of the loop taken apart, as the spread to read every
difference against. The whole command is meant to be run twice (measuring guide: the same command on the same code first). Results are checked while timing: (b)'s
t equals (a)'s where that is below L and is +inf elsewhere, and (c)'s flag equals (b)'s t < inf."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from portrayer_amd import _hip as H  # noqa: E402
from portrayer_amd import host  # noqa: E402

W, HT = 1920, 1080
FRACTIONS = (0.02, 0.10, 0.50)


def summary(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(len(v)))


def scene_diagonal(sc):
    """Diagonal of a finite box around the flattened nodes' bounds (an unbounded primitive does not widen it beyond 1e3 per axis)."""
    b = np.nan_to_num(np.asarray(sc.flatten()["bounds"], dtype=np.float64).reshape(-1, 6), nan=0.0, posinf=1e3, neginf=-1e3)
    lo, hi = np.clip(b[:, :3].min(axis=0), -1e3, 1e3), np.clip(b[:, 3:].max(axis=0), -1e3, 1e3)
    return float(np.linalg.norm(hi - lo))


def ao_rays(r, sc, n, seed):
    prim = r.aov(sc.camera, W, HT, want=("position", "normal", "node"))
    hit = prim["node"] >= 0
    p, nrm = prim["position"][hit], prim["normal"][hit]
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(p), size=n)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    v *= np.where(np.sum(v * nrm[pick], axis=1) < 0.0, -1.0, 1.0)[:, None]
    return np.ascontiguousarray(p[pick]), np.ascontiguousarray(v)


def main():
    argv = sys.argv[1:]
    n = 1 << 22
    if "--rays" in argv:
        k = argv.index("--rays")
        n = int(argv[k + 1])
        del argv[k:k + 2]
    reps = int(argv[0]) if argv else 7
    out_path = argv[1] if len(argv) > 1 else None
    assert reps >= 5, "the median of at least 5 warm repetitions"
    lib = H.lib()
    result = {"rays": n, "repetitions": reps, "fractions": list(FRACTIONS), "scenes": {}}
    for scene_name in ("big-scene", "macho-cows"):
        sc = host.Scene.example(scene_name)
        diag = scene_diagonal(sc)
        result["scenes"][scene_name] = {"diagonal": diag}
        for name, tr in (("flat", H.TRAVERSE_FLAT), ("hier", H.TRAVERSE_HIER)):
            r = host.Renderer(sc, tr)
            c = r.context
            o, d = ao_rays(r, sc, n, seed=1)

            def alloc(nbytes):
                p = C.c_void_p()
                assert lib.pt_device_alloc(c, nbytes, C.byref(p)) == 0, lib.pt_last_error(c)
                return p

            def upload(a):
                p = alloc(a.nbytes)
                assert lib.pt_copy_to_device(c, p, a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
                return p

            def download(p, a):
                assert lib.pt_copy_from_device(c, a.ctypes.data_as(C.c_void_p), p, a.nbytes) == 0
                return a
            d_o, d_d = upload(o), upload(d)
            d_tm = {f: upload(np.full(n, f * diag)) for f in FRACTIONS}
            d_t, d_occ = alloc(n * 8), alloc(n)
            tb, ob = H.PtRaysBuffers(t=C.cast(d_t, H._dp)), H.PtRaysBuffers(occluded=C.cast(d_occ, H._u8p))
            ms = C.c_double(0.0)

            def run(any_hit, reorder, f=None):
                p = H.PtRaysParams(n, any_hit, reorder)
                b = ob if any_hit else tb
                if f is None:
                    rc = lib.pt_rays_device(c, C.byref(p), d_o, d_d, C.byref(b), None)
                else:
                    rc = lib.pt_segments_device(c, C.byref(p), d_o, d_d, d_tm[f], C.byref(b), None)
                assert rc == 0 and lib.pt_rays_finish(c, C.byref(ms)) == 0, lib.pt_last_error(c)
                return ms.value
            variants = {"a r0": lambda: run(0, 0), "a r1": lambda: run(0, 1)}
            for f in FRACTIONS:
                for ro in (0, 1):
                    variants["b %g r%d" % (f, ro)] = lambda f=f, ro=ro: run(0, ro, f)
                    variants["c %g r%d" % (f, ro)] = lambda f=f, ro=ro: run(1, ro, f)
            # the results, once: the bounded passes answer what the unbounded pass and a comparison answer
            run(0, 0)
            t_a = download(d_t, np.zeros(n))
            shares = {}
            for f in FRACTIONS:
                run(0, 1, f)
                t_b = download(d_t, np.zeros(n))
                want = np.where(t_a < f * diag, t_a, np.inf)
                assert t_b.tobytes() == want.tobytes(), "bounded nearest hit != filtered unbounded pass"
                run(1, 0, f)
                assert np.array_equal(download(d_occ, np.zeros(n, dtype=np.uint8)), np.isfinite(t_b).astype(np.uint8)), "bounded occlusion != bounded nearest hit"
                shares[f] = float(np.isfinite(t_b).mean())
            for _ in range(2):  # warm-up of every variant
                for fn in variants.values():
                    fn()
            t = {k: [] for k in variants}
            for _ in range(reps):
                for k, fn in variants.items():
                    t[k].append(fn())
            m = {k: summary(v) for k, v in t.items()}
            for k in ("a r0", "a r1"):
                m[k]["median_first_half"] = float(np.median(t[k][:reps // 2]))
                m[k]["median_second_half"] = float(np.median(t[k][reps // 2:]))
            m["occluded_share"] = shares
            m["unbounded_hit_share"] = float(np.isfinite(t_a).mean())
            result["scenes"][scene_name][name] = m
            print("%s %s: %d AO rays, diagonal %.4g, hit share unbounded %.3f, inside 2 / 10 / 50 %%: %s" % (
                scene_name, name, n, diag, m["unbounded_hit_share"], " ".join("%.3f" % shares[f] for f in FRACTIONS)))
            for k in variants:
                extra = "   halves %.3f / %.3f" % (m[k]["median_first_half"], m[k]["median_second_half"]) if k.startswith("a ") else ""
                print("  %-12s %9.3f ms  [%.3f .. %.3f]%s" % (k, m[k]["median"], m[k]["min"], m[k]["max"], extra), flush=True)
            for p in [d_o, d_d, d_t, d_occ] + list(d_tm.values()):
                lib.pt_device_free(c, p)
            r.close()
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
