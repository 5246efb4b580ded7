"""Register budgets of the adaptive film's sampling kernels (pt_film_map_m1..m9.o), read from the code objects' metadata (no GPU needed), as
tests/test_film_resources.py reads the film's. Every object holds the four <TEX, PARK> instantiations of pt_film_map_kernel of its mode and nothing else; they
are compiled for pt_film_waves = 3 waves per SIMD like the film's: none may use more than the 168 registers that leaves a lane, and none may declare static LDS
(the block's LDS is sized at launch). DESIGN 4.13 records the figures. pt_film_map.o holds the plan, fold, error and budget kernels, none of which spills."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "portrayer_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
BUDGET = 168        # registers per lane at 3 waves per SIMD (512 / 3, in allocation granules of 8)
INSTANTIATIONS = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (TEX, PARK)
SMALL = ["pt_film_budget_kernel", "pt_film_error_kernel", "pt_film_fold_map_kernel", "pt_film_plan_count_kernel", "pt_film_plan_reduce_kernel", "pt_film_plan_scan_kernel",
         "pt_film_plan_scatter_kernel"]


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


def kernels_of(mode):
    found, others = {}, []
    for blk in notes_of("pt_film_map_m%d.o" % mode).split("- .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        get = lambda key: re.search(r"\." + key + r":\s*(\S+)", blk).group(1)
        m = re.match(r"_Z18pt_film_map_kernelILi(\d+)ELb([01])ELi([01])EEv", get("name"))
        if not m:
            others.append(get("name"))
            continue
        assert int(m.group(1)) == mode, get("name")
        found[(int(m.group(2)), int(m.group(3)))] = {"vgpr": int(get("vgpr_count")), "agpr": int(get("agpr_count")), "sgpr": int(get("sgpr_count")), "spill": int(get("vgpr_spill_count")),
                                                     "scratch": int(get("private_segment_fixed_size")), "lds": int(get("group_segment_fixed_size")),
                                                     "max_flat_workgroup_size": int(get("max_flat_workgroup_size"))}
    assert not others, "pt_film_map_m%d.o holds other kernels: %r" % (mode, others)
    return found


def design_table():
    """DESIGN 4.13's table; its first column is written `map <MODE, TEX, PARK>`, so that 4.12's reader (every `| <d, d, d> |` row up to section 5) does not take
    these rows for the film's: (mode, TEX, PARK) -> (VGPRs + AGPRs, spilled VGPRs, scratch bytes per lane)."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.13 "):]
    sec = sec[:sec.index("\n## ")]
    rows = re.findall(r"^\|\s*map <(\d), ([01]), ([01])>\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", sec, flags=re.M)
    return {(int(m), int(t), int(p)): (int(v), int(s), int(b)) for m, t, p, v, s, b in rows}


def test_the_kernels_are_compiled_for_the_films_wave_count():
    src = open(os.path.join(CSRC, "pt_film_map.h")).read()
    assert re.search(r"__launch_bounds__\(PT_BLOCK, pt_film_waves\(MODE\)\) pt_film_map_kernel\(PtFilmMapArgs a0\)", src)
    assert len(design_table()) == 36, "DESIGN 4.13 has one row per instantiation"


def test_the_new_rows_are_not_read_as_the_films():
    """tests/test_film_resources.py::design_table reads `| <d, d, d> |` rows from 4.12 up to the next `## ` heading, which 4.13 lies inside: exactly the 36 of
    4.12 must match there."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.12 "):]
    sec = sec[:sec.index("\n## ")]
    assert "### 4.13 " in sec
    assert len(re.findall(r"^\|\s*<(\d), ([01]), ([01])>\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", sec, flags=re.M)) == 36


@pytest.mark.parametrize("mode", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_every_instantiation_is_present_and_fits_the_registers_of_its_wave_count(mode):
    found = kernels_of(mode)
    assert sorted(found) == INSTANTIATIONS, "pt_film_map_m%d.o must hold exactly the <TEX, PARK> instantiations of its mode, found %r" % (mode, sorted(found))
    table = design_table()
    for (tex, park), r in sorted(found.items()):
        print("mode %d TEX %d PARK %d: %r" % (mode, tex, park, r))
        assert r["vgpr"] + r["agpr"] <= BUDGET, (mode, tex, park, r)
        assert r["lds"] == 0 and r["max_flat_workgroup_size"] == 256, (mode, tex, park, r)
        assert table.get((mode, tex, park)) == (r["vgpr"] + r["agpr"], r["spill"], r["scratch"]), "DESIGN 4.13 records %r for <%d, %d, %d>, the object has %r" % (table.get((mode, tex, park)), mode, tex, park, r)


def test_the_small_kernels_object_holds_the_plan_fold_error_and_budget_kernels():
    notes = notes_of("pt_film_map.o")
    names = sorted(re.findall(r"\.name:\s*(\S+)", notes))
    assert len(names) == len(SMALL) and all(sum(want in got for got in names) == 1 for want in SMALL), names
    assert [int(v) for v in re.findall(r"\.vgpr_spill_count:\s*(\d+)", notes)] == [0] * len(SMALL)
    assert [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", notes)] == [0] * len(SMALL)
