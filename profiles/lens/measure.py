#!/usr/bin/env python3
"""What a lens costs a film's add: python3 profiles/lens/measure.py [repeats per side, default 7] [out.json] [scene,scene,...]

big-scene, soft-shadows and transmission-refraction at 1920x1080, add(8) (one launch of 8 samples per pixel and its fold), flat_scene traversal, seed 0,
PT_SAMPLE_RNG, everything resident on the GPU, the sides alternating in ONE process after a warm-up of each. Every side resets the film, queues ONE add of 8
with the background in device memory and closes it with pt_radiance_finish -> kernel_ms (HIP events around the sampling launch and its fold):
  film          pt_film_add_device: the pinhole through pt_film_kernel, the yardstick (byte-identical to the parent commit's kernel)
  thin0         pt_film_add_lens_device, PT_LENS_THIN with aperture 0: the same rays through pt_lens_kernel - what the lens' frame and set-up cost
  thin          ... aperture = 2 % of the distance to the point the camera looks at, focused there: a lane's eight samples leave from eight lens points
  ortho         ... PT_LENS_ORTHO framed like the perspective view at that distance
  stereo        ... PT_LENS_STEREO, 150 degrees across the image height
thin0 against film is the cost of the ray set-up and of the kernel's shape (same rays, same bits); thin, ortho and stereo against thin0 is what OTHER rays cost -
other coherence of the primary rays, other things seen. Prints one line per scene with medians [min .. max] and the ratios, then one JSON line."""
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

W, HT, SAMPLES = 1920, 1080, 8
SCENES = ("big-scene", "soft-shadows", "transmission-refraction")


def stats(v):
    v = np.sort(np.asarray(v))
    return dict(median=float(np.median(v)), min=float(v[0]), max=float(v[-1]))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
    scenes = tuple(sys.argv[3].split(",")) if len(sys.argv) > 3 else SCENES
    lib = H.lib()
    result = {"width": W, "height": HT, "samples": SAMPLES, "repeats_per_side": n, "runs": {}}
    for scene in scenes:
        bg = default_background(W, HT)
        rows = 1 if bg.shape == (HT, 3) else 0
        sc = host.Scene.example(scene, assets=ASSETS)
        r = host.Renderer(sc, H.TRAVERSE_FLAT)
        c = r.context
        cam = host.camera(sc.camera, W, HT)
        c10 = np.asarray(sc.camera, dtype=np.float64)
        focus = float(np.linalg.norm(c10[3:6] - c10[0:3]))
        lenses = {"thin0": host.Lens.thin(0.0, focus), "thin": host.Lens.thin(0.02 * focus, focus), "ortho": host.Lens.ortho(focus * float(np.tan(c10[9] / 2.0))),
                  "stereo": host.Lens.fisheye(150.0)}
        d_bg = C.c_void_p()
        assert lib.pt_device_alloc(c, bg.nbytes, C.byref(d_bg)) == 0, lib.pt_last_error(c)
        assert lib.pt_copy_to_device(c, d_bg, bg.ctypes.data_as(C.c_void_p), bg.nbytes) == 0
        full = H.PtRect(0, 0, W - 1, HT - 1)
        p = H.PtFilmParams(full, SAMPLES, 0, H.SAMPLE_RNG, rows)
        ms = C.c_double(0.0)
        film = C.c_void_p()
        assert lib.pt_film_create(c, W, HT, C.byref(film)) == 0, lib.pt_last_error(c)

        def side(lens):
            assert lib.pt_film_reset(c, film) == 0, lib.pt_last_error(c)
            if lens is None:
                assert lib.pt_film_add_device(c, film, C.byref(cam), d_bg, C.byref(p), None) == 0, lib.pt_last_error(c)
            else:
                assert lib.pt_film_add_lens_device(c, film, C.byref(cam), C.byref(lens), d_bg, C.byref(p), None) == 0, lib.pt_last_error(c)
            assert lib.pt_radiance_finish(c, C.byref(ms)) == 0, lib.pt_last_error(c)
            return ms.value
        sides = {"film": (lambda: side(None))}
        for name, lens in lenses.items():
            sides[name] = (lambda l=lens.struct(): side(l))
        for f in sides.values():  # warm-up of each side
            f()
        t = {k: [] for k in sides}
        for _ in range(n):
            for k, f in sides.items():
                t[k].append(f())
        m = {k: stats(v) for k, v in t.items()}
        m["ratio_to_film"] = {k: m[k]["median"] / m["film"]["median"] for k in sides if k != "film"}
        m["ratio_to_thin0"] = {k: m[k]["median"] / m["thin0"]["median"] for k in ("thin", "ortho", "stereo")}
        m["focus"] = focus
        result["runs"][scene] = m
        print("%-26s film %.2f ms [%.2f .. %.2f]" % (scene, m["film"]["median"], m["film"]["min"], m["film"]["max"]), flush=True)
        for k in lenses:
            print("    %-8s %.2f ms [%.2f .. %.2f]  x%.3f of film%s" % (k, m[k]["median"], m[k]["min"], m[k]["max"], m["ratio_to_film"][k],
                                                                       "" if k == "thin0" else "  x%.3f of thin0" % m["ratio_to_thin0"][k]), flush=True)
        assert lib.pt_film_destroy(c, film) == 0
        lib.pt_device_free(c, d_bg)
        r.close()
    print(json.dumps(result))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
