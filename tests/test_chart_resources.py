"""Resources of the chart pass's kernels (pt_chart.o), read from the code object's metadata (no GPU needed), as tests/test_gather_resources.py reads the gather
pass's: the object holds the seed, own and resolve kernels and nothing else; none uses scratch memory or LDS (no tree is walked, no stack is kept); and each
one's registers are what DESIGN 4.19's table states."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_guides_resources import ROOT, kernels_of  # noqa: E402

KERNELS = ("pt_chart_seed_kernel", "pt_chart_own_kernel", "pt_chart_resolve_kernel")


def chart_kernels():
    found = {}
    for name, r in kernels_of("pt_chart.o").items():
        short = [k for k in KERNELS if k in name]
        assert len(short) == 1, "pt_chart.o holds another kernel: %s" % name
        found[short[0]] = r
    return found


def design_table():
    """DESIGN 4.19's table: kernel -> (VGPRs + AGPRs, spilled VGPRs, scratch bytes per lane, LDS bytes)."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.19 "):]
    sec = sec[:sec.index("\n## ")]
    rows = re.findall(r"^\|\s*`(pt_chart_\w+_kernel)`\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", sec, flags=re.M)
    return {k: (int(v), int(s), int(b), int(l)) for k, v, s, b, l in rows}


def test_the_object_holds_the_three_kernels_and_nothing_else():
    assert sorted(chart_kernels()) == sorted(KERNELS)


def test_no_kernel_uses_scratch_or_lds_and_each_is_what_the_design_states():
    table = design_table()
    assert sorted(table) == sorted(KERNELS), "DESIGN 4.19's table names every kernel"
    for name, r in sorted(chart_kernels().items()):
        print(name, r)
        assert r["scratch"] == 0 and r["spill"] == 0, "%s spills: the pass is straight-line code over a handful of doubles" % name
        assert r["lds"] == 0, name
        assert r["max_flat_workgroup_size"] == 256, name
        assert r["vgpr"] + r["agpr"] <= 128, "%s: at most 128 registers keep four waves per SIMD" % name
        assert (r["vgpr"] + r["agpr"], r["spill"], r["scratch"], r["lds"]) == table[name], "%s: DESIGN 4.19 states %r" % (name, table[name])


def test_the_makefile_builds_the_unit_through_the_checked_assembly_path():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(OBJDIR)/pt_chart.o" in mk[mk.index("HIP_OBJS :="):mk.index("# Every HIP translation unit")]
    assert "$(OBJDIR)/%.o: $(CSRC)/%.hip $(HIP_HDRS) tools/check_exec_prologue.py\n\t$(call hip_four_steps,)" in mk
    tool = open(os.path.join(ROOT, "tools", "compare_render_objects.py")).read()
    assert '"pt_chart.o"' in tool
