"""Resources of the guides pass's kernels (pt_guides_m<mode>.o) and of the demodulated denoise's (pt_denoise_albedo.o), read from the code objects' metadata (no
GPU needed), as tests/test_denoise_resources.py reads the denoiser's: no instantiation of a mesh-free traversal mode - and neither of the two denoise kernels -
spills a vector register or uses scratch memory, the denoise kernels declare no LDS, and every one's registers are what DESIGN 4.16's table states."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "portrayer_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
MESH_FREE = (3, 6, 7)  # PT_MODE_FLAT_NOMESH, PT_MODE_HIER_NOMESH, PT_MODE_KD_NOMESH
ALBEDO_KERNELS = ["pt_albedo_seed_kernel", "pt_albedo_finish_kernel"]


def notes_of(name):
    obj = os.path.join(CSRC, name)
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no device object / llvm tools here: run __graft_entry__.build() first")
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(obj, os.path.join(tmp, "k.o"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "k.o"], cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)
        cos = [f for f in os.listdir(tmp) if "gfx950" in f]
        assert cos, "no gfx950 code object in %s" % obj
        return subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, cos[0])], capture_output=True, text=True, check=True).stdout


def kernels_of(name):
    """mangled kernel name -> its resources, for every kernel of the object."""
    found = {}
    for blk in notes_of(name).split("- .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        get = lambda key: re.search(r"\." + key + r":\s*(\S+)", blk).group(1)
        found[get("name")] = {"vgpr": int(get("vgpr_count")), "agpr": int(get("agpr_count")), "spill": int(get("vgpr_spill_count")), "scratch": int(get("private_segment_fixed_size")),
                              "lds": int(get("group_segment_fixed_size")), "max_flat_workgroup_size": int(get("max_flat_workgroup_size"))}
    return found


def guides_kernels(mode):
    """`pt_guides_kernel<mode, tex>` -> resources: the two instantiations of one mode's object, and nothing else in it."""
    found = {}
    for name, r in kernels_of("pt_guides_m%d.o" % mode).items():
        m = re.fullmatch(r"_Z16pt_guides_kernelILi(\d)ELb([01])EEv12PtGuidesArgs", name)
        assert m and int(m.group(1)) == mode, "pt_guides_m%d.o holds another kernel: %s" % (mode, name)
        found["pt_guides_kernel<%d, %s>" % (mode, "true" if m.group(2) == "1" else "false")] = r
    assert sorted(found) == ["pt_guides_kernel<%d, false>" % mode, "pt_guides_kernel<%d, true>" % mode]
    return found


def albedo_kernels():
    found = {}
    for name, r in kernels_of("pt_denoise_albedo.o").items():
        short = [k for k in ALBEDO_KERNELS if k in name]
        assert len(short) == 1, "pt_denoise_albedo.o holds another kernel: %s" % name
        found[short[0]] = r
    assert sorted(found) == sorted(ALBEDO_KERNELS)
    return found


def design_table():
    """DESIGN 4.16's table: kernel -> (VGPRs + AGPRs, LDS bytes per block, scratch bytes per lane)."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.16 "):]
    sec = sec[:sec.index("\n## ")]
    rows = re.findall(r"^\|\s*`(pt_guides_kernel<\d, (?:true|false)>|pt_albedo_\w+_kernel)`\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", sec, flags=re.M)
    return {name: (int(v), int(lds), int(scratch)) for name, v, lds, scratch in rows}


def test_every_mode_has_its_two_instantiations():
    for mode in range(1, 10):
        guides_kernels(mode)


def test_no_mesh_free_guides_instantiation_spills_or_uses_scratch():
    for mode in MESH_FREE:
        for name, r in sorted(guides_kernels(mode).items()):
            print(name, r)
            assert r["spill"] == 0 and r["scratch"] == 0, (name, r)
            assert r["lds"] == 0, "the traversal stacks are dynamic LDS, sized at the launch"


def test_the_albedo_kernels_spill_nothing_and_use_neither_scratch_nor_lds():
    for name, r in sorted(albedo_kernels().items()):
        print(name, r)
        assert r["spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0, (name, r)
        assert r["max_flat_workgroup_size"] == 256, (name, r)


def test_the_design_states_the_numbers():
    found = dict(albedo_kernels())
    for mode in MESH_FREE:
        found.update(guides_kernels(mode))
    table = design_table()
    assert sorted(table) == sorted(found), "DESIGN 4.16 has one row per mesh-free guides instantiation and per albedo kernel"
    for name, r in found.items():
        assert table[name] == (r["vgpr"] + r["agpr"], r["lds"], r["scratch"]), "DESIGN 4.16 records %r for %s, the object has %r" % (table[name], name, r)
