"""Resources of the lens film's kernels (pt_lens_m1..m9.o), read from the code objects' metadata (no GPU needed), as tests/test_probe_resources.py reads the
probe pass's. Every per-mode object holds the four <TEX, PARK> instantiations of its mode and nothing else; pt_lens_waves (csrc/pt_lens_inst.h) compiles all of
them for 3 waves per SIMD, the interpreter's occupancy: none may use more than the 168 registers that leaves a lane, none may declare static LDS (the block's LDS
is the frame's, sized at launch), and each one's registers, spilled registers and scratch bytes are what DESIGN 4.22's table states."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_guides_resources import ROOT, kernels_of  # noqa: E402

CSRC = os.path.join(ROOT, "portrayer_amd", "csrc")
BUDGET = 168  # registers per lane at 3 waves per SIMD (512 / 3, in allocation granules of 8)
INSTANTIATIONS = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (TEX, PARK)


def lens_kernels(mode):
    """(TEX, PARK) -> resources: the four instantiations of one mode's object, and nothing else in it."""
    found = {}
    assert os.path.exists(os.path.join(CSRC, "pt_lens_inst.hip")), "the kernel's translation unit"
    for name, r in kernels_of("pt_lens_m%d.o" % mode).items():
        m = re.fullmatch(r"_Z14pt_lens_kernelILi(\d)ELb([01])ELi([01])EEv10PtLensArgs", name)
        assert m and int(m.group(1)) == mode, "pt_lens_m%d.o holds another kernel: %s" % (mode, name)
        found[(int(m.group(2)), int(m.group(3)))] = r
    return found


def design_section():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.22 "):]
    return sec[:sec.index("\n## ")]


def design_table():
    """DESIGN 4.22's table: (mode, TEX, PARK) -> (VGPRs + AGPRs, spilled VGPRs, scratch bytes per lane)."""
    rows = re.findall(r"^\|\s*`pt_lens_kernel<(\d), ([01]), ([01])>`\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", design_section(), flags=re.M)
    return {(int(m), int(t), int(p)): (int(v), int(s), int(b)) for m, t, p, v, s, b in rows}


def function_body(text, signature):
    start = text.index(signature)
    return text[start:text.index("\n}\n", start)]


def test_the_wave_count_the_lds_and_the_frame_are_the_films():
    src = open(os.path.join(CSRC, "pt_lens_inst.h")).read()
    assert re.search(r"constexpr int pt_lens_waves\(int /\*mode\*/\) \{ return 3; \}", src), "pt_lens_waves changed: update BUDGET here knowingly"
    assert "PtFilmArgs f;" in src and "offsetof(PtLensArgs, f) == 0" in src
    kernel = open(os.path.join(CSRC, "pt_lens_inst.hip")).read()
    assert "__launch_bounds__(PT_BLOCK, pt_lens_waves(MODE))" in kernel and "pt_shade_frame<MODE, TEX, PARK, PtLensPass>(a0)" in kernel
    # the frame and the launcher are the shading passes' (pt_shade_frame.h): the LDS of the PtRenderArgs the pass names, a.f.r, and none beyond the frame's
    frame = open(os.path.join(CSRC, "pt_shade_frame.h")).read()
    assert "const PtRenderArgs& r = PASS::render(a);" in frame and "pt_render_lds_bytes(r.stack_lds_cap, tex, park ? 1 : 0)" in frame
    assert "render(const PtLensArgs& a0) { return a0.f.r; }" in kernel and "pt_shade_launch<PT_INST_MODE, PtLensPass>" in kernel
    assert "__shared__ uint32_t pt_lds[]" in frame and frame.count("__shared__") == 1 and "__shared__" not in kernel, "no LDS beyond the frame's"
    # the film's item-to-slot mapping (its begin and finish, on the PtFilmArgs at the start of the block), the lens' source
    film = open(os.path.join(CSRC, "pt_film.h")).read()
    assert "PtFilmPass::begin(a0.f, " in kernel and "PtFilmPass::finish(a0.f, " in kernel and film.count("pt_film_item_slot(") == 3
    assert "using Source = PtLensSource;" in kernel and "pt_source_advance<TEX, HIER, PARK, typename PASS::Source>" in frame
    # the lens is read through the kernarg segment where a sample starts: source() gets the block the frame has just seen again
    assert "src.lens = &aa.lens" in kernel and "const typename PASS::Args& aa = pt_args_again(a0);" in frame and "PASS::source(aa, src);" in frame
    api = open(os.path.join(CSRC, "pt_api.hip")).read()
    assert "k = pt_interp_sizing(c, a.r)" in function_body(api, "static int pt_film_pass_args("), "the lens add sizes its LDS as the film's add does: the same function"


@pytest.mark.parametrize("mode", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_every_instantiation_is_present_fits_its_wave_count_and_is_what_the_design_states(mode):
    found = lens_kernels(mode)
    assert sorted(found) == INSTANTIATIONS, "pt_lens_m%d.o must hold exactly the <TEX, PARK> instantiations of its mode, found %r" % (mode, sorted(found))
    table = design_table()
    for (tex, park), r in sorted(found.items()):
        print("mode %d TEX %d PARK %d: %r" % (mode, tex, park, r))
        assert r["vgpr"] + r["agpr"] <= BUDGET, (mode, tex, park, r)
        assert r["lds"] == 0 and r["max_flat_workgroup_size"] == 256, (mode, tex, park, r)
        assert table.get((mode, tex, park)) == (r["vgpr"] + r["agpr"], r["spill"], r["scratch"]), "DESIGN 4.22 records %r for <%d, %d, %d>, the object has %r" % (table.get((mode, tex, park)), mode, tex, park, r)


def test_the_design_has_one_row_per_instantiation():
    assert sorted(design_table()) == [(m, t, p) for m in range(1, 10) for t, p in INSTANTIATIONS]
