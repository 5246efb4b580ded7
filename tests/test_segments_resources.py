"""Register budgets of the bounded-segment pass's kernels (pt_segments_m1..m9.o), read from the code objects' metadata (no GPU needed), as
tests/test_rays_resources.py reads the ray-query pass's. pt_segments_waves (csrc/pt_segments_inst.h) is pt_rays_waves: the instantiations that carry
the per-lane KDMesh walker (modes 2, 4, 5) are compiled for 3 waves per SIMD and the others for 4; none may outgrow that, and the mesh-free ones
(3, 6, 7) use no scratch memory."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "portrayer_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
BUDGET = {3: 168, 4: 128}
WAVES = {1: 4, 2: 3, 3: 4, 4: 3, 5: 3, 6: 4, 7: 4, 8: 4, 9: 4}  # pt_segments_waves = pt_rays_waves
MESH_FREE = (3, 6, 7)


def kernel_of(mode):
    obj = os.path.join(CSRC, "pt_segments_m%d.o" % mode)
    assert os.path.exists(obj), "%s is missing: the build makes one object per traversal mode" % obj
    assert os.path.exists(os.path.join(LLVM, "llvm-readelf")), "the llvm tools the build itself runs"
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(obj, os.path.join(tmp, "k.o"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "k.o"], cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)
        cos = [f for f in os.listdir(tmp) if "gfx950" in f]
        assert cos, "no gfx950 code object in %s" % obj
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, cos[0])], capture_output=True, text=True, check=True).stdout
    found, names = {}, []
    for blk in notes.split("- .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        get = lambda key: re.search(r"\." + key + r":\s*(\S+)", blk).group(1)
        names.append(get("name"))
        m = re.match(r"_Z18pt_segments_kernelILi(\d+)EEv", get("name"))
        if m:
            found[int(m.group(1))] = {"vgpr": int(get("vgpr_count")), "agpr": int(get("agpr_count")), "spill": int(get("vgpr_spill_count")), "scratch": int(get("private_segment_fixed_size"))}
    assert list(found) == [mode] and len(names) == 1, "pt_segments_m%d.o must hold exactly the kernel of its mode, found %r" % (mode, names)
    return found[mode]


def test_the_wave_counts_are_the_ray_query_passs():
    src = open(os.path.join(CSRC, "pt_segments_inst.h")).read()
    assert re.search(r"constexpr int pt_segments_waves\(int mode\) \{ return pt_rays_waves\(mode\); \}", src), "pt_segments_waves changed: update WAVES here knowingly"
    src = open(os.path.join(CSRC, "pt_rays_inst.h")).read()
    assert re.search(r"constexpr int pt_rays_waves\(int mode\) \{ return \(mode == PT_MODE_KD \|\| mode == PT_MODE_FLAT_KDMESH \|\| mode == PT_MODE_HIER\) \? 3 : 4; \}", src)


@pytest.mark.parametrize("mode", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_every_instantiation_fits_the_registers_of_its_wave_count(mode):
    r = kernel_of(mode)
    assert r["vgpr"] + r["agpr"] <= BUDGET[WAVES[mode]], (mode, r)
    if mode in MESH_FREE:
        assert r["scratch"] == 0 and r["spill"] == 0, (mode, r)
