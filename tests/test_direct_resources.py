"""Resources of the direct-light pass's kernels (pt_direct_m<mode>.o), read from the code objects' metadata (no GPU needed), as tests/test_ao_resources.py reads the
ambient-occlusion pass's: every mode's object holds the pass's one kernel and nothing else, no instantiation of a mesh-free traversal mode spills a vector register
or uses scratch memory, and every one's registers are what DESIGN 4.20's table states."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_guides_resources import MESH_FREE, ROOT, kernels_of  # noqa: E402


def direct_kernels(mode):
    """`pt_direct_kernel<mode>` -> resources: the one instantiation of a mode's object, and nothing else in it."""
    found = {}
    for name, r in kernels_of("pt_direct_m%d.o" % mode).items():
        m = re.fullmatch(r"_Z16pt_direct_kernelILi(\d)EEv12PtDirectArgs", name)
        assert m and int(m.group(1)) == mode, "pt_direct_m%d.o holds another kernel: %s" % (mode, name)
        found["pt_direct_kernel<%d>" % mode] = r
    assert sorted(found) == ["pt_direct_kernel<%d>" % mode]
    return found


def design_table():
    """DESIGN 4.20's table: kernel -> (VGPRs + AGPRs, LDS bytes per block, scratch bytes per lane)."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.20 "):]
    sec = sec[:sec.index("\n## ")]
    rows = re.findall(r"^\|\s*`(pt_direct_kernel<\d>)`\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", sec, flags=re.M)
    return {name: (int(v), int(lds), int(scratch)) for name, v, lds, scratch in rows}


def test_every_mode_has_its_kernel_and_nothing_else():
    for mode in range(1, 10):
        for name, r in direct_kernels(mode).items():
            assert r["max_flat_workgroup_size"] == 256, (name, r)


def test_no_mesh_free_instantiation_spills_or_uses_scratch():
    for mode in MESH_FREE:
        for name, r in sorted(direct_kernels(mode).items()):
            print(name, r)
            assert r["spill"] == 0 and r["scratch"] == 0, (name, r)
            assert r["lds"] == 0, "the traversal stacks and the columns of terms and sums are dynamic LDS, sized at the launch"
            assert r["vgpr"] + r["agpr"] <= 128, "four waves per SIMD, as pt_segments_kernel's"


def test_the_design_states_the_numbers():
    found = {}
    for mode in range(1, 10):
        found.update(direct_kernels(mode))
    table = design_table()
    assert sorted(table) == sorted(found), "DESIGN 4.20 has one row per instantiation"
    for name, r in found.items():
        assert table[name] == (r["vgpr"] + r["agpr"], r["lds"], r["scratch"]), "DESIGN 4.20 records %r for %s, the object has %r" % (table[name], name, r)
