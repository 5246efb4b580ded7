"""Kernel time of the six shading passes - what bench.py does not time: per pass the median kernel_ms of LAUNCHES launches after WARM warm-up launches, at
sizes where each kernel runs for milliseconds: the film passes (film, film_map with a uniform budget, lens) at 1920 x 1080 x 8 samples, radiance on the
1920 x 1080 pixel-centre rays, gather at 2^18 points x 16, probe at 4096 x 256. Scenes and traversals: big-scene (flat, kd), transmission-refraction (flat),
water-glass (flat; textured). One process is one repeat. PACKAGE_ROOT: the directory whose portrayer_amd/ (the Python layer and the two libraries) is
measured - another commit's build, for an A/B; default: this tree's.
usage: python profiles/r17/pass_times.py LABEL OUT.json [PACKAGE_ROOT]"""
import json
import os
import sys

import numpy as np
import torch  # noqa: F401  (one HIP runtime in the process: torch's)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else ROOT)

from lens_restate import replay  # noqa: E402
from portrayer_amd import _hip as H  # noqa: E402
from portrayer_amd import host  # noqa: E402
from scene_dsl import ASSETS  # noqa: E402

WARM, LAUNCHES = 3, 20
W, HT, SAMPLES = 1920, 1080, 8
CASES = (("big-scene", "flat"), ("big-scene", "kd"), ("transmission-refraction", "flat"), ("water-glass", "flat"))
BG = (0.25, 0.5, 1.0)


def median_ms(launch):
    for _ in range(WARM):
        launch()
    return round(float(np.median([launch() for _ in range(LAUNCHES)])), 4)


def main(label, out_path):
    result = {"label": label, "warm": WARM, "launches": LAUNCHES, "kernel_ms": {}}
    for name, mname in CASES:
        sc = host.Scene.example(name, assets=ASSETS)
        r = host.Renderer(sc, {"flat": H.TRAVERSE_FLAT, "kd": H.TRAVERSE_KD}[mname], kd_depth=10)
        c10 = np.asarray(sc.camera, dtype=np.float64)
        bg = np.tile(np.array(BG), (HT, 1))
        focus = float(np.linalg.norm(c10[3:6] - c10[0:3]))
        lens = host.Lens.thin(0.04 * focus, focus)
        budget = np.full((HT, W), SAMPLES, dtype=np.uint32)
        ys, xs = np.mgrid[0:HT, 0:W]
        xy = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.uint32)
        O, D = replay(H, host.camera(c10, W, HT), (H.LENS_THIN, 0.0, focus, 1.0), W, HT, 0, H.SAMPLE_CENTRE, xy, np.zeros(len(xy), dtype=np.uint32))  # no aperture: the pinhole
        rgb = np.zeros((len(xy), 3))
        aov = r.aov(c10, 512, 512, want=("position", "normal"))
        P, N = np.ascontiguousarray(aov["position"].reshape(-1, 3)), np.ascontiguousarray(aov["normal"].reshape(-1, 3))
        small = r.aov(c10, 64, 64, want=("position", "normal"))
        probes = np.ascontiguousarray((small["position"] + 0.25 * small["normal"]).reshape(-1, 3))
        eye = np.array(list(host.camera(c10, 512, 512).eye))
        film = r.film(W, HT)

        def fresh(add):
            film.reset()
            return add()
        passes = {
            "film": lambda: fresh(lambda: film.add(c10, bg, samples=SAMPLES, seed=1, sample_mode=H.SAMPLE_RNG)),
            "film_map": lambda: fresh(lambda: film.add_map(c10, bg, budget, seed=1, sample_mode=H.SAMPLE_RNG)),
            "lens": lambda: fresh(lambda: film.add(c10, bg, samples=SAMPLES, seed=1, sample_mode=H.SAMPLE_RNG, lens=lens)),
            "radiance": lambda: r.radiance(O, D, BG, seed=1, into=rgb)["kernel_ms"],
            "gather": lambda: r.gather(P, N, BG, samples=16, seed=1, eye=eye, want=("sum",))["kernel_ms"],
            "probe": lambda: r.probe(probes, BG, samples=256, seed=1, want=("sh",))["kernel_ms"],
        }
        for what, launch in passes.items():
            key = "%s/%s/%s" % (name, mname, what)
            result["kernel_ms"][key] = median_ms(launch)
            print(label, key, result["kernel_ms"][key], flush=True)
            with open(out_path, "w") as fh:
                json.dump(result, fh, indent=1)
        film.close()
        r.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
