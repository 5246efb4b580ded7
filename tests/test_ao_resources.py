"""Resources of the ambient-occlusion pass's kernels (pt_ao_m<mode>.o), read from the code objects' metadata (no GPU needed), as tests/test_guides_resources.py reads
the guides pass's: every mode's object holds the pass's two work layouts and nothing else, no instantiation of a mesh-free traversal mode spills a vector register or
uses scratch memory, and every one's registers are what DESIGN 4.17's table states."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_guides_resources import MESH_FREE, ROOT, kernels_of  # noqa: E402

LAYOUT = {"0": "point", "1": "sample"}  # PT_AO_POINT_MAJOR, PT_AO_SAMPLE_MAJOR


def ao_kernels(mode):
    """`pt_ao_kernel<mode, layout>` -> resources: the two instantiations of one mode's object, and nothing else in it."""
    found = {}
    for name, r in kernels_of("pt_ao_m%d.o" % mode).items():
        m = re.fullmatch(r"_Z12pt_ao_kernelILi(\d)ELi([01])EEv8PtAoArgs", name)
        assert m and int(m.group(1)) == mode, "pt_ao_m%d.o holds another kernel: %s" % (mode, name)
        found["pt_ao_kernel<%d, %s>" % (mode, LAYOUT[m.group(2)])] = r
    assert sorted(found) == ["pt_ao_kernel<%d, point>" % mode, "pt_ao_kernel<%d, sample>" % mode]
    return found


def design_table():
    """DESIGN 4.17's table: kernel -> (VGPRs + AGPRs, LDS bytes per block, scratch bytes per lane)."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.17 "):]
    sec = sec[:sec.index("\n## ")]
    rows = re.findall(r"^\|\s*`(pt_ao_kernel<\d, (?:point|sample)>)`\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", sec, flags=re.M)
    return {name: (int(v), int(lds), int(scratch)) for name, v, lds, scratch in rows}


def test_every_mode_has_its_two_layouts_and_nothing_else():
    for mode in range(1, 10):
        for name, r in ao_kernels(mode).items():
            assert r["max_flat_workgroup_size"] == 256, (name, r)


def test_no_mesh_free_instantiation_spills_or_uses_scratch():
    for mode in MESH_FREE:
        for name, r in sorted(ao_kernels(mode).items()):
            print(name, r)
            assert r["spill"] == 0 and r["scratch"] == 0, (name, r)
            assert r["lds"] == 0, "the traversal stacks and the columns of directions are dynamic LDS, sized at the launch"
            assert r["vgpr"] + r["agpr"] <= 128, "four waves per SIMD, as pt_segments_kernel's"


def test_the_design_states_the_numbers():
    found = {}
    for mode in MESH_FREE:
        found.update(ao_kernels(mode))
    table = design_table()
    assert sorted(table) == sorted(found), "DESIGN 4.17 has one row per mesh-free instantiation"
    for name, r in found.items():
        assert table[name] == (r["vgpr"] + r["agpr"], r["lds"], r["scratch"]), "DESIGN 4.17 records %r for %s, the object has %r" % (table[name], name, r)
