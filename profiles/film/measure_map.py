#!/usr/bin/env python3
"""What a budget per pixel costs and buys, against its yardstick: python3 profiles/film/measure_map.py [repeats per side, default 5] [out.json] [scene,scene,...]

big-scene, entering-the-mirror-dimension and transmission-refraction at 1920x1080 and macho-cows at its bench size (1280x720), flat_scene traversal,
PT_SAMPLE_RNG, the sides alternating in ONE process after a warm-up of each. Every figure is device time between the pass's two HIP events (kernel_ms): plan,
sampling and fold kernels of all launch rounds. The yardstick is pt_film_add of the same build on a film without moments, whose kernels are byte-identical to
the parent commit's (tools/compare_render_objects.py).
  add8            reset, Film.add(samples=8)                                                      the yardstick of (a), (b)
  (a) map8        reset, add_map with a budget of 8 everywhere: the same samples through the list
      plan        a DEVICE map of zeros, max_samples = 8: the plan kernels, a sampling launch that finds an empty list, the fold - an upper bound of the plan
  (b) map1to8     reset, add_map with budgets uniform in 1 .. 8 (4.5 on average): what full lanes buy where add() would have to take 8 everywhere
  add8_second     a film that holds 8 samples, add(samples=8)                                     the yardstick of (c)
  (c) map_top10   a film with moments that holds 8 samples, add_map with a budget of 8 on the tenth of the pixels with the largest error()
  (d) refine      a film with moments, refine(threshold = the median positive error after 8 samples, min_count 8, step 8, max_count 64): device time and samples,
      uniform     against ONE add of as many samples as refine's worst pixel reached
Prints one line per side with medians [p10 .. p90], then one JSON line."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from portrayer_amd import _hip as H  # noqa: E402
from portrayer_amd import host  # noqa: E402
from scene_dsl import ASSETS, default_background  # noqa: E402

SCENES = {"big-scene": (1920, 1080), "entering-the-mirror-dimension": (1920, 1080), "transmission-refraction": (1920, 1080), "macho-cows": (1280, 720)}
SEED, MODE = 0, H.SAMPLE_RNG


def stats(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return dict(median=float(np.median(v)), p10=float(v[len(v) // 10]), p90=float(v[(9 * len(v)) // 10]), min=float(v[0]), max=float(v[-1]))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
    scenes = tuple(sys.argv[3].split(",")) if len(sys.argv) > 3 else tuple(SCENES)
    lib = H.lib()
    result = {"repeats_per_side": n, "runs": {}}
    for scene in scenes:
        w, h = SCENES[scene]
        px = w * h
        bg = default_background(w, h)
        rows = 1 if bg.shape == (h, 3) else 0
        sc = host.Scene.example(scene, assets=ASSETS)
        r = host.Renderer(sc, H.TRAVERSE_FLAT)
        c = r.context
        cam10 = sc.camera
        cam = host.camera(cam10, w, h)
        plain, noisy = r.film(w, h), r.film(w, h, moments=True)
        rng = np.random.default_rng(1)
        eight = np.full((h, w), 8, dtype=np.uint32)
        one_to_eight = rng.integers(1, 9, size=(h, w)).astype(np.uint32)

        # the state (c) and (d) start from, and what they are asked for
        noisy.add(cam10, bg, samples=8, seed=SEED, sample_mode=MODE)
        e8 = noisy.error()
        top = np.zeros((h, w), dtype=np.uint32)
        top.ravel()[np.argsort(e8.ravel(), kind="stable")[-(px // 10):]] = 8
        threshold = float(np.median(e8[e8 > 0.0]))

        # the plan alone: a device map of zeros through the library's own calls
        def alloc(nbytes, src=None):
            p = C.c_void_p()
            assert lib.pt_device_alloc(c, nbytes, C.byref(p)) == 0, lib.pt_last_error(c)
            if src is not None:
                assert lib.pt_copy_to_device(c, p, src.ctypes.data_as(C.c_void_p), src.nbytes) == 0
            return p
        d_bg, d_zero = alloc(bg.nbytes, bg), alloc(px * 4, np.zeros(px, dtype=np.uint32))
        raw = C.c_void_p()
        assert lib.pt_film_create(c, w, h, C.byref(raw)) == 0, lib.pt_last_error(c)
        mp = H.PtFilmMapParams(H.PtRect(0, 0, w - 1, h - 1), 8, SEED, MODE, rows)
        ms = C.c_double(0.0)

        def plan():
            assert lib.pt_film_add_map_device(c, raw, C.byref(cam), d_bg, C.byref(mp), d_zero, None) == 0, lib.pt_last_error(c)
            assert lib.pt_radiance_finish(c, C.byref(ms)) == 0, lib.pt_last_error(c)
            return ms.value

        def add8():
            plain.reset()
            return plain.add(cam10, bg, samples=8, seed=SEED, sample_mode=MODE)

        def add8_second():
            plain.reset()
            plain.add(cam10, bg, samples=8, seed=SEED, sample_mode=MODE)
            return plain.add(cam10, bg, samples=8, seed=SEED, sample_mode=MODE)

        def mapped(budget):
            plain.reset()
            return plain.add_map(cam10, bg, budget, seed=SEED, sample_mode=MODE, max_samples=8)

        def map_top10():
            noisy.reset()
            noisy.add(cam10, bg, samples=8, seed=SEED, sample_mode=MODE)
            return noisy.add_map(cam10, bg, top, seed=SEED, sample_mode=MODE, max_samples=8)
        refined = {}

        def refine():
            noisy.reset()
            out = noisy.refine(cam10, bg, threshold, min_count=8, max_count=64, step=8, max_passes=16, seed=SEED, sample_mode=MODE)
            refined.update(out)
            return out["kernel_ms"]
        refine()
        counts = noisy.counts()
        worst = int(counts.max())
        refined["worst"], refined["mean_count"] = worst, float(counts.mean())
        refined["histogram"] = {str(int(k)): int(v) for k, v in zip(*np.unique(counts, return_counts=True))}

        def uniform():
            plain.reset()
            return plain.add(cam10, bg, samples=worst, seed=SEED, sample_mode=MODE)
        sides = {"add8": add8, "map8": lambda: mapped(eight), "plan": plan, "map1to8": lambda: mapped(one_to_eight), "add8_second": add8_second, "map_top10": map_top10,
                 "refine": refine, "uniform": uniform}
        for f in sides.values():  # warm-up of each side
            f()
        t = {k: [] for k in sides}
        for _ in range(n):
            for k, f in sides.items():
                t[k].append(f())
        m = {k: stats(v) for k, v in t.items()}
        m["refine_result"] = refined
        m["samples"] = {"add8": 8 * px, "map8": 8 * px, "map1to8": int(one_to_eight.sum()), "map_top10": int(top.sum()), "refine": refined["samples"], "uniform": worst * px}
        spread = m["add8"]["p90"] - m["add8"]["p10"]
        m["a_slower_than_allowed"] = bool(m["map8"]["median"] - m["add8"]["median"] > 3.0 * spread + m["plan"]["median"])
        result["runs"][scene] = m
        print("%-30s %dx%d" % (scene, w, h), flush=True)
        for k in sides:
            print("    %-12s %9.3f ms [%9.3f .. %9.3f]  %12d samples" % (k, m[k]["median"], m[k]["p10"], m[k]["p90"], m["samples"].get(k, 0)), flush=True)
        print("    (a) map8 / add8 %.3f   (b) map1to8 / add8 %.3f   (c) map_top10 / add8_second %.3f   (d) refine / uniform(%d) %.3f time, %.3f samples; passes %d, mean count %.2f" % (
            m["map8"]["median"] / m["add8"]["median"], m["map1to8"]["median"] / m["add8"]["median"], m["map_top10"]["median"] / m["add8_second"]["median"], worst,
            m["refine"]["median"] / m["uniform"]["median"], refined["samples"] / (worst * px), refined["passes"], refined["mean_count"]), flush=True)
        assert lib.pt_film_destroy(c, raw) == 0
        for p in (d_bg, d_zero):
            lib.pt_device_free(c, p)
        plain.close(); noisy.close()
        r.close()
    print(json.dumps(result))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
