#!/usr/bin/env python3
"""Are the kernels of two builds the same machine code?

    python3 tools/compare_render_objects.py <dir of the other build's objects> [<dir of this build's objects>]

Extracts the gfx950 code object from every HIP object of both directories (llvm-objdump --offloading, as tests/test_kernel_resources.py does) and compares
them byte for byte: the nine per-mode objects of the render kernel and of every pass beside it (pt_<pass>_m1.o .. m9.o) and the single objects (pt_api.o,
pt_scene.o, pt_build.o, pt_node.o, pt_rays_sort.o, pt_film.o, pt_film_map.o, pt_denoise.o, pt_denoise_albedo.o, pt_chart.o, pt_probe.o). Only pt_render_m*.o must exist in the other build; an object it lacks (a build
from before that pass existed) or one that holds no device code in either build is skipped. A change that claims to leave kernels alone (a new pass beside
them, host code) runs this against a build of its parent commit: identical code objects mean identical behaviour and speed of every kernel, without a GPU.
Exit status 0: all identical; 1: some differ (named)."""
import filecmp
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


PASSES = ("render", "aov", "guides", "rays", "segments", "ao", "radiance", "gather", "direct", "probe", "film", "film_map", "lens")
SINGLES = ("pt_api.o", "pt_scene.o", "pt_build.o", "pt_node.o", "pt_rays_sort.o", "pt_film.o", "pt_film_map.o", "pt_denoise.o", "pt_denoise_albedo.o", "pt_chart.o", "pt_probe.o")


def code_object(obj: str, tmp: str):
    """Path of the gfx950 code object extracted from the host object `obj` (into a directory of its own under tmp); None where it holds no device code."""
    d = tempfile.mkdtemp(dir=tmp)
    shutil.copy(obj, os.path.join(d, "k.o"))
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "k.o"], cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)
    cos = [f for f in os.listdir(d) if "gfx950" in f]
    return os.path.join(d, cos[0]) if cos else None


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    other = argv[1]
    mine = argv[2] if len(argv) > 2 else os.path.join(ROOT, "portrayer_amd", "csrc")
    names = ["pt_%s_m%d.o" % (p, m) for p in PASSES for m in range(1, 10)] + list(SINGLES)
    differ, compared = [], 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in names:
            if not name.startswith("pt_render_m") and not os.path.exists(os.path.join(other, name)):
                continue  # (a build from before that object existed)
            a, b = code_object(os.path.join(other, name), tmp), code_object(os.path.join(mine, name), tmp)
            if a is None and b is None and name in SINGLES:
                print("%-20s no device code, skipped" % name)
                continue
            if a is None or b is None:
                raise SystemExit("no gfx950 code object in %s" % os.path.join(other if a is None else mine, name))
            same = filecmp.cmp(a, b, shallow=False)
            print("%-20s %9d bytes  %s" % (name, os.path.getsize(b), "identical" if same else "DIFFERENT"))
            compared += 1
            if not same:
                differ.append(name)
    print("code objects of %s and the single objects: %s" % (", ".join(PASSES), "all %d byte-identical" % compared if not differ else "differ: " + ", ".join(differ)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
