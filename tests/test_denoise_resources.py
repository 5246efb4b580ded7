"""Resources of the denoiser's kernels (pt_denoise.o), read from the code object's metadata (no GPU needed), as tests/test_film_map_resources.py reads the
adaptive film's: the object holds the seed, direct, tiled and finish kernels and nothing else, none spills or uses scratch, only the tiled kernel declares LDS,
and its size and every kernel's registers are what DESIGN 4.14's table states."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "portrayer_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ["pt_denoise_seed_kernel", "pt_denoise_direct_kernel", "pt_denoise_tiled_kernel", "pt_denoise_finish_kernel"]
TILE_LDS = 20 * 20 * (10 * 8 + 4 + 4)  # 20 x 20 cells: c, v, normal, position as f64 arrays of their own, node and valid as words


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


def kernels():
    found = {}
    for blk in notes_of("pt_denoise.o").split("- .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        get = lambda key: re.search(r"\." + key + r":\s*(\S+)", blk).group(1)
        short = [k for k in KERNELS if k in get("name")]
        assert len(short) == 1, "pt_denoise.o holds another kernel: %s" % get("name")
        found[short[0]] = {"vgpr": int(get("vgpr_count")), "agpr": int(get("agpr_count")), "sgpr": int(get("sgpr_count")), "spill": int(get("vgpr_spill_count")),
                           "sgpr_spill": int(get("sgpr_spill_count")), "scratch": int(get("private_segment_fixed_size")), "lds": int(get("group_segment_fixed_size")),
                           "max_flat_workgroup_size": int(get("max_flat_workgroup_size"))}
    return found


def design_table():
    """DESIGN 4.14's table: kernel -> (VGPRs + AGPRs, LDS bytes per block)."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.14 "):]
    sec = sec[:sec.index("\n## ")]
    rows = re.findall(r"^\|\s*`(pt_denoise_\w+_kernel)`\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", sec, flags=re.M)
    return {name: (int(v), int(lds)) for name, v, lds in rows}


def test_no_denoise_kernel_spills_or_uses_scratch():
    found = kernels()
    assert sorted(found) == sorted(KERNELS)
    for name, r in sorted(found.items()):
        print(name, r)
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["max_flat_workgroup_size"] == 256, (name, r)


def test_the_tiled_kernels_lds_is_what_the_design_states():
    found, table = kernels(), design_table()
    assert sorted(table) == sorted(KERNELS), "DESIGN 4.14 has one row per kernel"
    for name, r in found.items():
        assert table[name] == (r["vgpr"] + r["agpr"], r["lds"]), "DESIGN 4.14 records %r for %s, the object has %r" % (table[name], name, r)
        assert r["lds"] == (TILE_LDS if name == "pt_denoise_tiled_kernel" else 0), (name, r)
    assert TILE_LDS == 35200 and 4 * TILE_LDS <= 160 * 1024, "four blocks of the tiled kernel share a CU's 160 KiB"
    src = open(os.path.join(CSRC, "pt_denoise.h")).read()
    assert re.search(r"#define PT_DN_LDS_BYTES \(PT_DN_CELLS \* \(10 \* 8 \+ 4 \+ 4\)\)", src)
