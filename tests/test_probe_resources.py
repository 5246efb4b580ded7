"""Resources of the probe pass's kernels (pt_probe_m1..m9.o and pt_probe.o), read from the code objects' metadata (no GPU needed), as
tests/test_gather_resources.py reads the gather pass's. Every per-mode object holds the four <TEX, PARK> instantiations of its mode and nothing else;
pt_probe_waves (csrc/pt_probe_inst.h) compiles all of them for 3 waves per SIMD, the interpreter's occupancy: none may use more than the 168 registers that leaves
a lane, none may declare static LDS (the block's LDS is the frame's, sized at launch: the 27 sums live in frame slots that are dead once a lane is done), and each
one's registers, spilled registers and scratch bytes are what DESIGN 4.21's table states. The fold kernel spills nothing."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_guides_resources import ROOT, kernels_of  # noqa: E402

CSRC = os.path.join(ROOT, "portrayer_amd", "csrc")
BUDGET = 168  # registers per lane at 3 waves per SIMD (512 / 3, in allocation granules of 8)
INSTANTIATIONS = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (TEX, PARK)


def probe_kernels(mode):
    """(TEX, PARK) -> resources: the four instantiations of one mode's object, and nothing else in it."""
    found = {}
    assert os.path.exists(os.path.join(CSRC, "pt_probe_inst.hip")), "the pass's translation unit"
    for name, r in kernels_of("pt_probe_m%d.o" % mode).items():
        m = re.fullmatch(r"_Z15pt_probe_kernelILi(\d)ELb([01])ELi([01])EEv11PtProbeArgs", name)
        assert m and int(m.group(1)) == mode, "pt_probe_m%d.o holds another kernel: %s" % (mode, name)
        found[(int(m.group(2)), int(m.group(3)))] = r
    return found


def design_section():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.21 "):]
    return sec[:sec.index("\n## ")]


def design_table():
    """DESIGN 4.21's table: (mode, TEX, PARK) -> (VGPRs + AGPRs, spilled VGPRs, scratch bytes per lane)."""
    rows = re.findall(r"^\|\s*`pt_probe_kernel<(\d), ([01]), ([01])>`\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", design_section(), flags=re.M)
    return {(int(m), int(t), int(p)): (int(v), int(s), int(b)) for m, t, p, v, s, b in rows}


def function_body(text, signature):
    start = text.index(signature)
    return text[start:text.index("\n}\n", start)]


def test_the_wave_count_and_the_lds_are_the_interpreter_passes():
    src = open(os.path.join(CSRC, "pt_probe_inst.h")).read()
    assert re.search(r"constexpr int pt_probe_waves\(int /\*mode\*/\) \{ return 3; \}", src), "pt_probe_waves changed: update BUDGET here knowingly"
    kernel = open(os.path.join(CSRC, "pt_probe_inst.hip")).read()
    assert "__launch_bounds__(PT_BLOCK, pt_probe_waves(MODE))" in kernel
    # the launcher is the shading passes' (pt_shade_frame.h): the LDS of the PtRenderArgs the pass names, a.r
    frame = open(os.path.join(CSRC, "pt_shade_frame.h")).read()
    assert "const PtRenderArgs& r = PASS::render(a);" in frame and "pt_render_lds_bytes(r.stack_lds_cap, tex, park ? 1 : 0)" in frame
    assert "render(const PtProbeArgs& a0) { return a0.r; }" in kernel and "pt_shade_launch<PT_INST_MODE, PtProbePass>" in kernel
    assert "__shared__ uint32_t pt_lds[]" in kernel and kernel.count("__shared__") == 1, "no LDS beyond the frame's"
    api = open(os.path.join(CSRC, "pt_api.hip")).read()
    assert "pt_interp_sizing(c, a.r)" in function_body(api, "static int pt_probe_common("), "pt_probe_common sizes its LDS with pt_interp_sizing"


@pytest.mark.parametrize("mode", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_every_instantiation_is_present_fits_its_wave_count_and_is_what_the_design_states(mode):
    found = probe_kernels(mode)
    assert sorted(found) == INSTANTIATIONS, "pt_probe_m%d.o must hold exactly the <TEX, PARK> instantiations of its mode, found %r" % (mode, sorted(found))
    table = design_table()
    for (tex, park), r in sorted(found.items()):
        print("mode %d TEX %d PARK %d: %r" % (mode, tex, park, r))
        assert r["vgpr"] + r["agpr"] <= BUDGET, (mode, tex, park, r)
        assert r["lds"] == 0 and r["max_flat_workgroup_size"] == 256, (mode, tex, park, r)
        assert table.get((mode, tex, park)) == (r["vgpr"] + r["agpr"], r["spill"], r["scratch"]), "DESIGN 4.21 records %r for <%d, %d, %d>, the object has %r" % (table.get((mode, tex, park)), mode, tex, park, r)


def test_the_design_has_one_row_per_instantiation_and_the_folds():
    assert sorted(design_table()) == [(m, t, p) for m in range(1, 10) for t, p in INSTANTIATIONS]
    row = re.search(r"^\|\s*`pt_probe_fold_kernel`\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", design_section(), flags=re.M)
    assert row, "DESIGN 4.21 has a row for the fold kernel"
    fold = kernels_of("pt_probe.o")
    assert list(fold) == ["_Z20pt_probe_fold_kernelPKdPdmj"], "pt_probe.o holds the fold kernel and nothing else"
    r = fold["_Z20pt_probe_fold_kernelPKdPdmj"]
    assert tuple(int(v) for v in row.groups()) == (r["vgpr"] + r["agpr"], r["spill"], r["scratch"]) and r["spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0
