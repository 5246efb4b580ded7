"""Wall time of the host forms of the passes - what bench.py does not time: the median of CALLS calls of every form of tests/test_gpu_point_forms.py, all of its
buffers asked for, at that test's small shapes, in the flat and the k-d traversal. One process is one repeat. PACKAGE_ROOT: the directory whose portrayer_amd/
(the Python layer and the two libraries) is measured - another commit's build, for an A/B; default: this tree's.
usage: python profiles/r16/host_forms.py LABEL OUT.json [PACKAGE_ROOT]"""
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (one HIP runtime in the process: torch's)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else ROOT)

import test_gpu_point_forms as T  # noqa: E402
from portrayer_amd import _hip as H  # noqa: E402
from portrayer_amd import host  # noqa: E402

CALLS = 200


def main(label, out_path):
    result = {"label": label, "calls": CALLS, "median_us": {}}
    for mode in T.MODES:
        c = T.Ctx(host, H, mode)
        for form, (table, call) in T.FORMS.items():
            names = tuple(getattr(H, table) if isinstance(table, str) else table)
            for _ in range(10):
                call(c, T.SMALL, names, None)
            times = np.empty(CALLS)
            for k in range(CALLS):
                t0 = time.perf_counter()
                call(c, T.SMALL, names, None)
                times[k] = time.perf_counter() - t0
            result["median_us"]["%s/%s" % (mode, form)] = round(float(np.median(times)) * 1e6, 1)
        c.r.close()
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
