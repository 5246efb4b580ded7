#!/usr/bin/env python3
"""Are the render kernels of two builds the same machine code?

    python3 tools/compare_render_objects.py <dir of the other build's objects> [<dir of this build's objects>]

Extracts the gfx950 code object from pt_render_m1.o .. pt_render_m9.o of both directories (llvm-objdump --offloading, as
tests/test_kernel_resources.py does) and compares them byte for byte; likewise the primary-visibility pass's (pt_aov_m*.o), the ray-query passes'
(pt_rays_m*.o, pt_segments_m*.o), the radiance pass's (pt_radiance_m*.o), the film's (pt_film_m*.o, pt_film.o) and the single objects' (pt_api.o, pt_build.o,
pt_rays_sort.o), where the other build has them. A change that claims to leave the render path alone
(a new pass beside it, host code) runs this against a build of its parent commit: identical code objects mean identical
behaviour and speed of every render kernel, without a GPU. Exit status 0: all identical; 1: some differ (named)."""
import filecmp
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def code_object(obj: str, tmp: str) -> str:
    """Path of the gfx950 code object extracted from the host object `obj` (into a directory of its own under tmp)."""
    d = tempfile.mkdtemp(dir=tmp)
    shutil.copy(obj, os.path.join(d, "k.o"))
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "k.o"], cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)
    cos = [f for f in os.listdir(d) if "gfx950" in f]
    if not cos:
        raise SystemExit("no gfx950 code object in %s" % obj)
    return os.path.join(d, cos[0])


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    other = argv[1]
    mine = argv[2] if len(argv) > 2 else os.path.join(ROOT, "portrayer_amd", "csrc")
    differ, compared = [], 0
    with tempfile.TemporaryDirectory() as tmp:
        for prefix in ("pt_render", "pt_aov", "pt_rays", "pt_segments", "pt_radiance"):
            for m in range(1, 10):
                name = "%s_m%d.o" % (prefix, m)
                if prefix != "pt_render" and not os.path.exists(os.path.join(other, name)):
                    continue  # (a build from before that pass existed)
                a, b = code_object(os.path.join(other, name), tmp), code_object(os.path.join(mine, name), tmp)
                same = filecmp.cmp(a, b, shallow=False)
                print("%-18s %9d bytes  %s" % (name, os.path.getsize(b), "identical" if same else "DIFFERENT"))
                compared += 1
                if not same:
                    differ.append(name)
        # the film's objects (pt_film_m*.o and its fold / resolve kernels) and the single objects, where the other build has them
        singles = ["pt_film_m%d.o" % m for m in range(1, 10)] + ["pt_film.o", "pt_api.o", "pt_build.o", "pt_rays_sort.o"]  # (pt_node.o holds no device code)
        for name in singles:
            if not os.path.exists(os.path.join(other, name)):
                continue
            a, b = code_object(os.path.join(other, name), tmp), code_object(os.path.join(mine, name), tmp)
            same = filecmp.cmp(a, b, shallow=False)
            print("%-18s %9d bytes  %s" % (name, os.path.getsize(b), "identical" if same else "DIFFERENT"))
            compared += 1
            if not same:
                differ.append(name)
    print("render, aov, rays, segments, radiance, film and single code objects: %s" % ("all %d byte-identical" % compared if not differ else "differ: " + ", ".join(differ)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
