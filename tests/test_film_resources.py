"""Register budgets of the film's sampling kernels (pt_film_m1..m9.o), read from the code objects' metadata (no GPU needed), as
tests/test_radiance_resources.py reads the radiance pass's. Every object holds the four <TEX, PARK> instantiations of its mode and nothing else;
pt_film_waves (csrc/pt_film_inst.h) compiles all of them for 3 waves per SIMD, the interpreter's occupancy: none may use more than the 168 registers that
leaves a lane, and none may declare static LDS (the block's LDS is sized at launch). DESIGN 4.12 records the figures. pt_film.o holds the fold and resolve
kernels and nothing else."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "portrayer_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
BUDGET = {3: 168}   # registers per lane at 3 waves per SIMD (512 / 3, in allocation granules of 8)
WAVES = 3           # pt_film_waves
INSTANTIATIONS = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (TEX, PARK)


def kernels_of(mode):
    obj = os.path.join(CSRC, "pt_film_m%d.o" % mode)
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no device object / llvm tools here: run __graft_entry__.build() first")
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(obj, os.path.join(tmp, "k.o"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "k.o"], cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)
        cos = [f for f in os.listdir(tmp) if "gfx950" in f]
        assert cos, "no gfx950 code object in %s" % obj
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, cos[0])], capture_output=True, text=True, check=True).stdout
    found, others = {}, []
    for blk in notes.split("- .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        get = lambda key: re.search(r"\." + key + r":\s*(\S+)", blk).group(1)
        m = re.match(r"_Z14pt_film_kernelILi(\d+)ELb([01])ELi([01])EEv", get("name"))
        if not m:
            others.append(get("name"))
            continue
        assert int(m.group(1)) == mode, get("name")
        found[(int(m.group(2)), int(m.group(3)))] = {"vgpr": int(get("vgpr_count")), "agpr": int(get("agpr_count")), "sgpr": int(get("sgpr_count")), "spill": int(get("vgpr_spill_count")),
                                                     "scratch": int(get("private_segment_fixed_size")), "lds": int(get("group_segment_fixed_size")),
                                                     "max_flat_workgroup_size": int(get("max_flat_workgroup_size"))}
    assert not others, "pt_film_m%d.o holds other kernels: %r" % (mode, others)
    return found


def design_table():
    """DESIGN 4.12's table (its first column is written <MODE, TEX, PARK>, so that no other section's reader takes its rows for its own): (mode, TEX, PARK) -> (VGPRs + AGPRs, spilled VGPRs, scratch bytes per lane)."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.12 "):]
    sec = sec[:sec.index("\n## ")]
    rows = re.findall(r"^\|\s*<(\d), ([01]), ([01])>\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", sec, flags=re.M)
    return {(int(m), int(t), int(p)): (int(v), int(s), int(b)) for m, t, p, v, s, b in rows}


def function_body(text, signature):
    """The function of pt_api.hip that starts with `signature`, up to its closing brace in column 0."""
    start = text.index(signature)
    return text[start:text.index("\n}\n", start)]


def test_the_wave_count_is_the_one_the_source_states():
    src = open(os.path.join(CSRC, "pt_film_inst.h")).read()
    assert re.search(r"constexpr int pt_film_waves\(int /\*mode\*/\) \{ return 3; \}", src), "pt_film_waves changed: update WAVES and BUDGET here knowingly"
    # the LDS budget stands once, in the sizing the interpreter passes share; the film's argument block calls it, and both of its queueing functions build that block
    api = open(os.path.join(CSRC, "pt_api.hip")).read()
    sizing = function_body(api, "static PtInterp pt_interp_sizing(")
    assert re.search(r"r\.stack_lds_cap = pt_stack_lds_cap\(r\.scene, pt_block_budget\(3\), frame_bytes\);", sizing), "the film sizes its LDS for three blocks per CU"
    budget = open(os.path.join(CSRC, "pt_context.h")).read()  # ... where pt_block_budget(3) is 52 KB: 3 x 52 KB of the CU's 160 KB
    assert re.search(r"static size_t pt_block_budget\(int waves\) \{ return \(size_t\)\(waves >= 6 \? 26 : \(waves == 5 \? 31 : \(waves == 4 \? 39 : 52\)\)\) \* 1024; \}", budget), "three blocks per CU: 52 KB each"
    assert "pt_kd_semantics(mode)" in function_body(api, "static int pt_stack_lds_cap(int mode, int stack_cap, size_t block_budget, size_t frame_bytes)")
    assert "k = pt_interp_sizing(c, a.r)" in function_body(api, "static int pt_film_pass_args(")
    for queue in ("static int pt_film_add_common(", "static int pt_film_add_map_common("):
        assert "pt_film_pass_args(c, f, cam, d_background, " in function_body(api, queue), queue


@pytest.mark.parametrize("mode", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_every_instantiation_is_present_and_fits_the_registers_of_its_wave_count(mode):
    found = kernels_of(mode)
    assert sorted(found) == INSTANTIATIONS, "pt_film_m%d.o must hold exactly the <TEX, PARK> instantiations of its mode, found %r" % (mode, sorted(found))
    table = design_table()
    for (tex, park), r in sorted(found.items()):
        print("mode %d TEX %d PARK %d: %r" % (mode, tex, park, r))
        assert r["vgpr"] + r["agpr"] <= BUDGET[WAVES], (mode, tex, park, r)
        assert r["lds"] == 0 and r["max_flat_workgroup_size"] == 256, (mode, tex, park, r)
        assert table.get((mode, tex, park)) == (r["vgpr"] + r["agpr"], r["spill"], r["scratch"]), "DESIGN 4.12 records %r for <%d, %d, %d>, the object has %r" % (table.get((mode, tex, park)), mode, tex, park, r)


def test_the_small_kernels_object_holds_the_fold_and_the_resolve_kernel():
    obj = os.path.join(CSRC, "pt_film.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no device object / llvm tools here: run __graft_entry__.build() first")
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(obj, os.path.join(tmp, "k.o"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "k.o"], cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)
        cos = [f for f in os.listdir(tmp) if "gfx950" in f]
        assert cos, "no gfx950 code object in %s" % obj
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, cos[0])], capture_output=True, text=True, check=True).stdout
    names = sorted(re.findall(r"\.name:\s*(\S+)", notes))
    assert len(names) == 2 and "pt_film_fold_kernel" in names[0] and "pt_film_resolve_kernel" in names[1], names
    assert [int(v) for v in re.findall(r"\.vgpr_spill_count:\s*(\d+)", notes)] == [0, 0]
