"""Host time of the render launch path - what bench.py's 1920 x 1080 frames hide: the median wall time of CALLS pairs pt_render_device + pt_render_finish of a
16 x 16, one-sample frame of the five-primitive scene of tests/test_gpu_launch_plan.py (flat_scene: the launch with every table and list). At that size the frame is
almost all launch path. One process is one repeat. PACKAGE_ROOT: the directory whose portrayer_amd/ (the Python layer and the two libraries) is measured - another
commit's build, for an A/B; default: this tree's.
usage: python profiles/r18/launch_path.py LABEL OUT.json [PACKAGE_ROOT]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (one HIP runtime in the process: torch's)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else ROOT)

import host_glue  # noqa: E402
import test_gpu_launch_plan as T  # noqa: E402
from portrayer_amd import _hip as H  # noqa: E402
from portrayer_amd import host  # noqa: E402
from scene_dsl import default_background  # noqa: E402

CALLS = 200
W = HGT = 16


def main(label, out_path):
    scene, _ = T.build_scene("two lights")
    r = host.Renderer(host_glue.host_scene(scene), H.TRAVERSE_FLAT)
    lib, c = H.lib(), r.context
    bg = np.ascontiguousarray(default_background(W, HGT))
    d_bg, d_img = C.c_void_p(), C.c_void_p()
    assert lib.pt_device_alloc(c, bg.nbytes, C.byref(d_bg)) == 0 and lib.pt_copy_to_device(c, d_bg, bg.ctypes.data_as(C.c_void_p), bg.nbytes) == 0
    assert lib.pt_device_alloc(c, W * HGT * 3, C.byref(d_img)) == 0
    p = H.PtRenderParams(W, HGT, H.PtRect(0, 0, W - 1, HGT - 1), 1, 1, H.SAMPLE_RNG, 1 if bg.shape == (HGT, 3) else 0, 0, 1, 0)
    camera = host.camera(host_glue.cam10(T.CAMERA), W, HGT)
    st = H.PtStats()

    def pair():
        slot = int(lib.pt_context_next_slot(c))
        assert lib.pt_render_device(c, C.byref(camera), d_bg, C.byref(p), 0, d_img, C.c_void_p(lib.pt_context_stream(c, slot))) == 0, lib.pt_last_error(c)
        assert lib.pt_render_finish(c, C.byref(st)) == 0, lib.pt_last_error(c)

    for _ in range(20):
        pair()
    times = np.empty(CALLS)
    for k in range(CALLS):
        t0 = time.perf_counter()
        pair()
        times[k] = time.perf_counter() - t0
    result = {"label": label, "calls": CALLS, "median_us": round(float(np.median(times)) * 1e6, 1), "min_us": round(float(times.min()) * 1e6, 1),
              "kernel_mode": int(st.kernel_mode), "kernel_variant": int(st.kernel_variant)}
    lib.pt_device_free(c, d_img)
    lib.pt_device_free(c, d_bg)
    r.close()
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
