"""tools/check_exec_prologue.py - the build's gate against the code-generation defect behind round 4's wrong counting render and round 3's hang
(profiles/r05/notes.md section 1): vector spill code placed in front of the s_or_b64 exec that re-converges a block's lanes. The fixture below is
the block as hipcc emitted it for pt_render_kernel<2, true, false, 0> (-DPT_ARGS_AGAIN_EVERYWHERE), registers and offsets as found."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "check_exec_prologue.py")
spec = importlib.util.spec_from_file_location("check_exec_prologue", TOOL)
chk = importlib.util.module_from_spec(spec)
spec.loader.exec_module(chk)

DEFECT = """\
_Z16pt_render_kernelILi2ELb1ELb0ELi0EEv12PtRenderArgs: ; @kernel
; %bb.190:
\ts_and_saveexec_b64 s[0:1], s[28:29]
\ts_cbranch_execz .LBB14_192
; %bb.191:                              ;   in Loop: Header=BB14_181 Depth=3
\ts_waitcnt vmcnt(0)
\tv_lshl_add_u64 v[136:137], v[48:49], 0, 1
\tv_mov_b64_e32 v[52:53], v[136:137]
.LBB14_192:                             ;   in Loop: Header=BB14_181 Depth=3
\ts_mov_b32 s2, s26
\tscratch_store_dwordx2 off, v[118:119], off offset:236 ; 8-byte Folded Spill
\tscratch_store_dword off, v114, off offset:232 ; 4-byte Folded Spill
\ts_or_b64 exec, exec, s[0:1]
\ts_load_dwordx2 s[74:75], s[24:25], 0x20
\tv_mov_b32_e32 v119, 0
"""
# ordinary code: a spill store inside the divergent region (after a real vector instruction), an exec restore in the middle of a block, a reload behind the restore
CLEAN = """\
kernel_b: ; @kernel_b
\ts_and_saveexec_b64 s[0:1], vcc
\ts_cbranch_execz .LBB0_2
\ts_and_saveexec_b64 s[6:7], vcc
\ts_cbranch_execz .LBB0_3
\ts_and_saveexec_b64 s[4:5], vcc
\ts_cbranch_execz .LBB0_1
.LBB0_1:
\tv_add_f64 v[0:1], v[2:3], v[4:5]
\tscratch_store_dwordx2 off, v[0:1], off offset:8 ; 8-byte Folded Spill
\ts_or_b64 exec, exec, s[4:5]
.LBB0_2:
\ts_mov_b32 s2, s26
\ts_or_b64 exec, exec, s[0:1]
\tscratch_load_dwordx2 v[0:1], off, off offset:8 ; 8-byte Folded Reload
\tv_writelane_b32 v167, s2, 3
.LBB0_3:
\tv_writelane_b32 v167, s2, 4
\ts_or_b64 exec, exec, s[6:7]
"""


def test_the_defect_is_found_and_repaired(tmp_path):
    src = tmp_path / "k.s"
    src.write_text(DEFECT)
    found = chk.scan(str(src))
    assert [d[4].split()[0] for d in found] == ["scratch_store_dwordx2", "scratch_store_dword"]
    assert all(d[1].startswith("_Z16pt_render_kernelILi2ELb1ELb0ELi0E") and d[2] == ".LBB14_192" for d in found)
    fixed, log = chk.repair(DEFECT.splitlines(keepends=True))
    assert len(log) == 1 and log[0][2].startswith("s_or_b64 exec, exec, s[0:1]") and len(log[0][3]) == 2
    text = "".join(fixed)
    # ONE instruction moved, nothing else touched: the exec restore now follows the scalar copy and precedes both stores
    block = text[text.index(".LBB14_192:"):].splitlines()[1:5]
    assert [b.split()[0] for b in block] == ["s_mov_b32", "s_or_b64", "scratch_store_dwordx2", "scratch_store_dword"]
    assert sorted(text.splitlines()) == sorted(DEFECT.splitlines())
    out = tmp_path / "k_fixed.s"
    out.write_text(text)
    assert chk.scan(str(out)) == []


# round 3's hang (profiles/r04/c20_hang_rocgdb.txt: the chunk-sum loop's trip count, v58 = v72, far above 8): the live-range-split copy that SAVES the count sits in
# front of the exec restore, so only the region's lanes save theirs. Block .LBB31_423 of pt_render_simple_kernel<6, false, false, 6, false> as round 3's tree compiles.
R03_HANG = """\
_Z23pt_render_simple_kernelILi6ELb0ELb0ELi6ELb0EEv12PtRenderArgs: ; @kernel
; %bb.367:
\tscratch_store_dwordx2 off, v[0:1], off offset:16 ; 8-byte Folded Spill
\ts_and_saveexec_b64 s[4:5], s[88:89]
\ts_cbranch_execz .LBB31_423
; %bb.368:
\tds_write2st64_b64 v78, v[6:7], v[4:5] offset0:8 offset1:12
.LBB31_423:                             ;   in Loop: Header=BB31_7 Depth=1
\tv_writelane_b32 v79, s96, 18
\tv_mov_b32_e32 v72, v58
\ts_nop 0
\tv_writelane_b32 v79, s97, 19
\ts_or_b64 exec, exec, s[4:5]
\ts_load_dword s33, s[78:79], 0x4
"""


def test_the_copy_form_of_round_3s_hang_and_the_region_body(tmp_path):
    src = tmp_path / "h.s"
    src.write_text(R03_HANG)
    found = chk.scan(str(src))
    assert len(found) == 1 and found[0][4] == "v_mov_b32_e32 v72, v58" and found[0][2] == ".LBB31_423"
    fixed, log = chk.repair(R03_HANG.splitlines(keepends=True))
    text = "".join(fixed)
    block = [b.split()[0] for b in text[text.index(".LBB31_423:"):].splitlines()[1:6]]
    assert block == ["v_writelane_b32", "s_or_b64", "v_mov_b32_e32", "s_nop", "v_writelane_b32"]
    out = tmp_path / "h_fixed.s"
    out.write_text(text)
    assert chk.scan(str(out)) == []
    # NOT the defect (pt_cast_kernel<2> of csrc/pt_api.hip as compiled in round 5; a first version of the checker "repaired" it and would have broken it): the label
    # is the region's BODY, entered with s_cbranch_execnz, laid out behind the join with the join's code duplicated at its end - the move in front of that copy of
    # the exec restore is the region's own code and must stay with the region's lanes
    ok = tmp_path / "ok.s"
    ok.write_text("k: ; @k\n.LBB9_327:\n\ts_or_b64 exec, exec, s[50:51]\n\ts_and_saveexec_b64 s[2:3], s[0:1]\n\ts_cbranch_execnz .LBB9_328\n.LBB9_190:\n"
                  "\ts_or_b64 exec, exec, s[2:3]\n\tv_mov_b32_e32 v0, 0\n\ts_branch .LBB9_332\n.LBB9_328:\n\tv_readlane_b32 s4, v146, 54\n\ts_or_b64 s[56:57], s[0:1], s[4:5]\n"
                  "\tv_mov_b32_e32 v56, v10\n\ts_or_b64 exec, exec, s[2:3]\n\tv_mov_b32_e32 v0, 0\n")
    assert chk.scan(str(ok)) == []
    same, log = chk.repair(ok.read_text().splitlines(keepends=True))
    assert log == [] and "".join(same) == ok.read_text()


def test_a_join_is_one_whatever_mask_its_restore_uses(tmp_path):
    # allocator code in a fall-through block is not the defect; but .LBB0_1, the execz target, is a join whatever register its restore
    # reads (the restore of an enclosing region brings back the lanes this branch skipped too): the copy in front of it is the defect
    src = tmp_path / "j.s"
    src.write_text("k: ; @k\n\ts_and_saveexec_b64 s[6:7], vcc\n\ts_cbranch_execz .LBB0_1\n; %bb.2:\n\tv_mov_b32_e32 v72, v58\n\ts_or_b64 exec, exec, s[4:5]\n.LBB0_1:\n\tv_mov_b32_e32 v1, v2\n\ts_or_b64 exec, exec, s[8:9]\n")
    assert [(d[2], d[4]) for d in chk.scan(str(src))] == [(".LBB0_1", "v_mov_b32_e32 v1, v2")]


def test_ordinary_code_is_left_alone(tmp_path):
    src = tmp_path / "c.s"
    src.write_text(CLEAN)
    assert chk.scan(str(src)) == []
    fixed, log = chk.repair(CLEAN.splitlines(keepends=True))
    assert log == [] and "".join(fixed) == CLEAN


def test_command_line(tmp_path):
    bad, good, out = tmp_path / "bad.s", tmp_path / "good.s", tmp_path / "out.s"
    bad.write_text(DEFECT)
    good.write_text(CLEAN)
    assert subprocess.run([sys.executable, TOOL, str(good)], capture_output=True).returncode == 0
    r = subprocess.run([sys.executable, TOOL, str(bad)], capture_output=True, text=True)
    assert r.returncode == 1 and "DEFECT" in r.stdout and "Folded Spill" in r.stdout
    r = subprocess.run([sys.executable, TOOL, "--fix", str(bad), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and "REPAIRED" in r.stdout and "1 block(s) repaired, 0 defect(s) left" in r.stdout
    assert subprocess.run([sys.executable, TOOL, str(out)], capture_output=True).returncode == 0


# The exec saved in the split form (s_mov_b64 sX, exec ... s_mov_b64 exec, sY): block .LBB13_796 of pt_render_simple_kernel<8, false, true, 4, true> as
# hipcc emits it at 7f68b95 - round 4's spill, down to the register pair, in front of the restore
SPLIT_SAVE = """\
_Z23pt_render_simple_kernelILi8ELb0ELb1ELi4ELb1EEv12PtRenderArgs: ; @kernel
.LBB13_792:                             ;   in Loop: Header=BB13_40 Depth=2
\tv_cmp_ne_u32_e32 vcc, -1, v88
\tv_cmp_eq_u32_e64 s[0:1], -1, v88
\tv_mov_b64_e32 v[72:73], 0
\tv_mov_b64_e32 v[74:75], 0
\tv_mov_b64_e32 v[116:117], 0
\ts_and_b64 s[2:3], s[86:87], s[0:1]
\ts_mov_b64 s[0:1], exec
\tv_writelane_b32 v127, s2, 34
\ts_nop 1
\tv_writelane_b32 v127, s3, 35
\ts_and_b64 s[2:3], s[0:1], s[2:3]
\ts_mov_b64 exec, s[2:3]
\ts_cbranch_execz .LBB13_796
; %bb.793:                              ;   in Loop: Header=BB13_40 Depth=2
\tscratch_load_dwordx2 v[2:3], off, off offset:52 ; 8-byte Folded Reload
\ts_load_dword s2, s[80:81], 0x218
\ts_waitcnt lgkmcnt(0)
\ts_cmp_lg_u32 s2, 0
\ts_cbranch_scc1 .LBB13_795
; %bb.794:                              ;   in Loop: Header=BB13_40 Depth=2
\ts_load_dword s2, s[80:81], 0x21c
\tscratch_load_dwordx2 v[2:3], off, off offset:60 ; 8-byte Folded Reload
\tscratch_load_dwordx2 v[6:7], off, off offset:52 ; 8-byte Folded Reload
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\tv_mad_u64_u32 v[2:3], s[2:3], s2, v6, v[2:3]
.LBB13_795:                             ;   in Loop: Header=BB13_40 Depth=2
\ts_load_dwordx2 s[2:3], s[80:81], 0x210
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\tv_mad_u64_u32 v[6:7], s[2:3], v2, 24, s[2:3]
\tv_mov_b32_e32 v2, v7
\tv_mad_u64_u32 v[2:3], s[2:3], v3, 24, v[2:3]
\tv_mov_b32_e32 v7, v2
\tglobal_load_dwordx2 v[116:117], v[6:7], off offset:16
\tglobal_load_dwordx4 v[72:75], v[6:7], off
.LBB13_796:                             ;   in Loop: Header=BB13_40 Depth=2
\tv_writelane_b32 v127, s94, 36
\tv_writelane_b32 v127, s91, 37
\ts_movk_i32 s12, 0x48
\tscratch_store_dwordx2 off, v[118:119], off offset:84 ; 8-byte Folded Spill
\ts_or_b64 exec, exec, s[0:1]
\ts_and_b64 s[94:95], s[86:87], vcc
"""


def test_the_split_saveexec_form_is_found_and_repaired(tmp_path):
    src = tmp_path / "m8.s"
    src.write_text(SPLIT_SAVE)
    found = chk.scan(str(src))
    assert [(d[2], d[4].split()[0], d[5]) for d in found] == [(".LBB13_796", "scratch_store_dwordx2", "s_or_b64 exec, exec, s[0:1]")]
    fixed, log = chk.repair(SPLIT_SAVE.splitlines(keepends=True))
    text = "".join(fixed)
    assert len(log) == 1 and log[0][1] == ".LBB13_796" and sorted(text.splitlines()) == sorted(SPLIT_SAVE.splitlines())
    block = [b.split()[0] for b in text[text.index(".LBB13_796:"):].splitlines()[1:6]]
    assert block == ["v_writelane_b32", "v_writelane_b32", "s_movk_i32", "s_or_b64", "scratch_store_dwordx2"]
    out = tmp_path / "m8_fixed.s"
    out.write_text(text)
    assert chk.scan(str(out)) == []


def join(*prologue, mask="s[0:1]"):
    """a function whose execz branch skips a region to .LBB0_2, whose prologue is `prologue` in front of `s_or_b64 exec, exec, mask`"""
    return ("k: ; @k\n\ts_and_saveexec_b64 s[0:1], vcc\n\ts_cbranch_execz .LBB0_2\n; %bb.1:\n\tv_add_f64 v[0:1], v[2:3], v[4:5]\n.LBB0_2:\n"
            + "".join(f"\t{p}\n" for p in prologue) + f"\ts_or_b64 exec, exec, {mask}\n\tv_mov_b32_e32 v0, 0\n")


SPILL_STORE = "scratch_store_dwordx2 off, v[0:1], off offset:8 ; 8-byte Folded Spill"


def test_an_unsafe_repair_is_refused(tmp_path):
    # ADVICE's readlane carrier: the mask pair is reloaded from lanes of v127 between the spill and the restore - hoisting the restore
    # over the readlanes would read s[0:1] before they define it; and a move over an instruction that reads exec changes what it reads
    for prologue in [(SPILL_STORE, "v_readlane_b32 s0, v127, 4", "v_readlane_b32 s1, v127, 5"), (SPILL_STORE, "s_mov_b64 s[4:5], exec")]:
        src, out = tmp_path / "u.s", tmp_path / "u_out.s"
        src.write_text(join(*prologue))
        assert [d[4] for d in chk.scan(str(src))] == [SPILL_STORE]
        r = subprocess.run([sys.executable, TOOL, "--fix", str(src), "-o", str(out)], capture_output=True, text=True)
        assert r.returncode == 1 and "DEFECT LEFT" in r.stdout and "REPAIRED" not in r.stdout
        assert out.read_text() == src.read_text()


def test_a_rematerialised_constant_in_front_of_the_restore_is_a_defect_that_is_not_repaired(tmp_path):
    src = tmp_path / "r.s"
    src.write_text(join("s_mov_b32 s2, s26", "v_mov_b32_e32 v5, 0x3ff00000", "s_nop 0"))
    assert [d[4] for d in chk.scan(str(src))] == ["v_mov_b32_e32 v5, 0x3ff00000"]
    fixed, log = chk.repair(src.read_text().splitlines(keepends=True))
    assert log == [] and "".join(fixed) == src.read_text()


def test_a_join_is_found_whatever_saved_its_mask_and_however_it_is_entered(tmp_path):
    # the mask copied (and saved in an earlier block than the branch): the restore uses the copy
    copied = ("k: ; @k\n\ts_and_saveexec_b64 s[0:1], vcc\n; %bb.1:\n\ts_mov_b64 s[6:7], s[0:1]\n\ts_cbranch_execz .LBB0_3\n; %bb.2:\n"
              f"\tv_add_f64 v[0:1], v[2:3], v[4:5]\n.LBB0_3:\n\t{SPILL_STORE}\n\ts_or_b64 exec, exec, s[6:7]\n")
    # a loop's exit: the lanes leave the loop one by one (s_andn2_b64 exec), the last ones fall through its execnz back-edge
    loop_exit = ("k: ; @k\n\ts_mov_b64 s[2:3], 0\n.LBB0_1:\n\tv_add_f64 v[0:1], v[0:1], v[4:5]\n\tv_cmp_gt_f64_e32 vcc, 0, v[0:1]\n"
                 "\ts_or_b64 s[2:3], vcc, s[2:3]\n\ts_andn2_b64 exec, exec, s[2:3]\n\ts_cbranch_execnz .LBB0_1\n; %bb.2:\n"
                 f"\t{SPILL_STORE}\n\ts_or_b64 exec, exec, s[2:3]\n")
    for text, label in [(copied, ".LBB0_3"), (loop_exit, "; %bb.2")]:
        src = tmp_path / "j.s"
        src.write_text(text)
        assert [(d[2], d[4]) for d in chk.scan(str(src))] == [(label, SPILL_STORE)]


def test_the_makefile_builds_every_hip_object_through_the_check():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "check_exec_prologue.py --fix" in mk and "--offload-device-only -S" in mk and "-fcuda-include-gpubinary" in mk
    # no rule left that compiles a .hip straight to an object
    for line in mk.splitlines():
        if line.startswith("\t$(HIPCC)") and " -c " in line:
            assert "--cuda-host-only" in line, line
