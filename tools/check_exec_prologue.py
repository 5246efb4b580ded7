#!/usr/bin/env python3
"""Build gate against ONE code-generation defect of the AMDGPU backend this library has met twice (round 3's hang of the 80-register
kernel, round 4's wrong counting render of pt_render_kernel<2, true, *, 0>; root-caused in round 5, profiles/r05/notes.md section 1):

    a basic block that re-converges a divergent region starts with   s_or_b64 exec, exec, s[N:M]        (SI_END_CF)
    the scalar register allocator, which runs first, may put a live-range-split copy (s_mov_b32 sA, sB) IN FRONT of it - harmless -
    the vector register allocator, which runs second, looks for "the first instruction after the block's prologue" to insert a
    spill store / reload or a split copy, does not take that copy for part of the prologue, and inserts the VECTOR code BEFORE the s_or_b64:

        .LBB14_192:
            s_mov_b32 s2, s26
            scratch_store_dwordx2 off, v[118:119], off offset:236 ; 8-byte Folded Spill     <- executed by the lanes of the region only
            s_or_b64 exec, exec, s[0:1]

    the lanes that sat out the divergent region never store their value; the reload (full exec) hands them whatever the slot held.

The rule. A JOIN is a block that lanes reach with their exec bits cleared: a target of `s_cbranch_execz`, however the mask was saved in front
of the branch, or the block an `s_cbranch_execnz` falls through to (a loop's exit). (The block an `s_cbranch_execz` falls through to and a target of
`s_cbranch_execnz` are region bodies: vector code in front of a restore there is the program's own.) A block's PROLOGUE is its instructions up to
its first exec-widening instruction, ending early at a branch. In a join, ANY exec-dependent vector instruction in the prologue in front of
`s_or_b64 exec, exec, <any register pair>` is a defect; scalar instructions (s_waitcnt and s_nop included) and v_readlane / v_writelane /
v_readfirstlane are not. The current build repairs four such blocks: .LBB21_51 of pt_render_simple_kernel<1,true,false,4,true>,
.LBB22_50 of <1,true,false,3,true>, .LBB5_51 of <8,true,true,4,true> and .LBB13_796 of <8,false,true,4,true>.

usage: check_exec_prologue.py file.s [file.s ...]              exit code 1 if any defect is found
       check_exec_prologue.py --fix in.s -o out.s             writes the assembly with every block of the one safe shape REPAIRED - the restore
                                                              moved in front of the offending code, which is where the allocator meant it to be
                                                              (profiles/r05/notes.md section 1: this one move per block turns the wrong render into
                                                              the right one) - and checks the result; exit code 1 if a defect is left. The safe
                                                              shape: the offending code is allocator code only (spill stores / reloads, register
                                                              moves), and nothing the restore moves over writes its mask pair, vcc or exec or reads
                                                              exec. The Makefile builds every HIP object through this (device assembly -> repair ->
                                                              assemble -> embed)."""
import re
import sys

VECTOR = re.compile(r"^(v_|scratch_|global_|flat_|buffer_|ds_|image_|tbuffer_)")
# lane-independent vector instructions (they ignore exec): scalar values kept in / fetched from lanes of a vector register
EXEC_FREE = re.compile(r"^(v_writelane_b32|v_readlane_b32|v_readfirstlane_b32)")
# what re-converges lanes at the START of a block: SI_END_CF (s_or_b64 exec, exec, saved) and SI_ELSE (s_or_saveexec_b64)
WIDEN = re.compile(r"^(s_or_b64\s+exec,\s*exec,|s_or_saveexec_b64)")
RESTORE = re.compile(r"^s_or_b64\s+exec,\s*exec,\s*(s\[\d+:\d+\]|vcc)")
BRANCH = re.compile(r"^(s_cbranch_\w+|s_branch|s_setpc_b64|s_swappc_b64|s_endpgm)\b\s*(\S*)")
BLOCK = re.compile(r"^(\.LBB\d+_\d+:|; %bb\.\d+:|[A-Za-z_$][\w$.]*:)")
FUNC = re.compile(r"^([A-Za-z_$][\w$.]*):\s*(;.*)?$")
SPILL = ("Folded Spill", "Folded Reload")
# register-to-register vector moves: what a live-range split by the register allocator looks like (round 3's hang: `v_mov_b32_e32 v72, v58` - the chunk's sample
# count saved across a region - in front of the s_or_b64 exec of block .LBB31_423 of pt_render_simple_kernel<6, false, false, 6, false>)
COPY = re.compile(r"^(v_mov_b32_e32\s+v\d+,\s*v\d+\s*(;.*)?$|v_mov_b64_e32\s+v\[\d+:\d+\],\s*v\[\d+:\d+\]\s*(;.*)?$|v_accvgpr_(read|write)_b32\s)")


class Block:
    """label, function, code [(line index, instruction)], entered: the branch mnemonics that target the block, plus ("fall", <the previous
    block's last branch or None>) when control can fall through into it"""

    def __init__(self, label, func):
        self.label, self.func, self.code, self.entered = label, func, [], set()

    def is_join(self):
        body = ("fall", "s_cbranch_execz") in self.entered or "s_cbranch_execnz" in self.entered
        return not body and ("s_cbranch_execz" in self.entered or ("fall", "s_cbranch_execnz") in self.entered)

    def prologue(self):
        """(the instructions in front of the first exec-widening one, that one) - or (.., None) if a branch or the block's end comes first"""
        for k, (i, s) in enumerate(self.code):
            if WIDEN.match(s):
                return self.code[:k], (i, s)
            if BRANCH.match(s):
                return self.code[:k], None
        return self.code, None

    def defects(self):
        """(the exec-dependent vector instructions in front of the join's exec restore, the restore)"""
        code, widen = self.prologue()
        if not (widen and RESTORE.match(widen[1]) and self.is_join()):
            return [], None
        return [(i, s) for (i, s) in code if VECTOR.match(s) and not EXEC_FREE.match(s)], widen


def blocks(lines):
    """the assembly as a list of Blocks, each with its code and how it is entered"""
    out, func = [], "?"
    for i, raw in enumerate(lines):
        line = raw.rstrip("\n")
        m = FUNC.match(line)
        if m and not line.startswith(".L"):
            func = m.group(1)
        s = line.strip()
        if BLOCK.match(line):
            out.append(Block(line.split(":")[0].strip(), func))
        elif out and s and not s.startswith((";", ".", "//")):
            out[-1].code.append((i, s))
    targets = {}
    for b in out:
        for (_, s) in b.code:
            m = BRANCH.match(s)
            if m and m.group(2):
                targets.setdefault(m.group(2), set()).add(m.group(1))
    last = None
    for b in out:
        b.entered = set(targets.get(b.label, ()))
        if last is None or last.startswith("s_cbranch"):
            b.entered.add(("fall", last))
        ends = [BRANCH.match(s).group(1) for (_, s) in b.code if BRANCH.match(s)]
        last = ends[-1] if ends else None
    return out


def allocator_code(s):
    """vector instructions only the register allocator puts at the start of a block: spill stores / reloads and live-range-split copies"""
    return any(t in s for t in SPILL) or COPY.match(s) is not None


def sregs(operand):
    """the scalar registers an operand names: s7 -> {7}, s[6:7] -> {6, 7}, vcc_lo -> {"vcc"}, exec -> {"exec"}"""
    m = re.fullmatch(r"s(\d+)|s\[(\d+):(\d+)\]|(vcc|exec)(_lo|_hi)?", operand.strip())
    if not m:
        return set()
    if m.group(4):
        return {m.group(4)}
    lo = int(m.group(1) or m.group(2))
    return set(range(lo, int(m.group(3) or lo) + 1))


def movable(b, bad, restore):
    """whether the restore may move in front of `bad`: allocator code only, and nothing it moves over writes (first operand) its mask pair,
    vcc or exec, or names exec at all"""
    if not all(allocator_code(s) for (_, s) in bad):
        return False
    keep = sregs(RESTORE.match(restore[1]).group(1)) | {"vcc", "exec"}
    for (i, s) in b.code:
        ins = s.split(";")[0]
        dest = (ins.split(None, 1) + [""])[1].split(",")[0]
        if bad[0][0] <= i < restore[0] and ("exec" in ins or sregs(dest) & keep):
            return False
    return True


def scan(path):
    """[(path, function, block, line number, offending instruction, restore)] for every defect in the file"""
    with open(path, errors="replace") as fh:
        lines = fh.readlines()
    return [(path, b.func, b.label, i + 1, s, restore[1]) for b in blocks(lines) for (bad, restore) in [b.defects()] for (i, s) in bad]


def repair(lines):
    """Moves, in every join block of the safe shape (movable()), the exec restore in front of the first offending instruction.
    Returns (new lines, [(function, block, moved instruction, the instructions it moved in front of)])."""
    out, log = list(lines), []
    for b in blocks(lines):
        bad, restore = b.defects()
        if bad and movable(b, bad, restore):
            out.insert(bad[0][0], out.pop(restore[0]))  # (only lines between the two move: the other blocks' indices hold)
            log.append((b.func, b.label, restore[1], [s for (_, s) in bad]))
    return out, log


def main(argv):
    if argv and argv[0] == "--fix":
        if len(argv) != 4 or argv[2] != "-o":
            print(__doc__)
            return 2
        with open(argv[1], errors="replace") as fh:
            lines = fh.readlines()
        fixed, log = repair(lines)
        with open(argv[3], "w") as fh:
            fh.writelines(fixed)
        for (func, label, moved, spills) in log:
            print(f"REPAIRED {argv[1]}: {func} block {label}: `{moved}` moved in front of {len(spills)} spill instruction(s): {'; '.join(spills)}")
        left = scan(argv[3])
        for (path, func, label, ln, text, restore) in left:
            print(f"DEFECT LEFT {path}:{ln}: {func} block {label}: vector code in front of `{restore}`: {text}")
        print(f"{argv[1]}: {len(log)} block(s) repaired, {len(left)} defect(s) left")
        return 1 if left else 0
    bad = 0
    for p in argv:
        d = scan(p)
        for (path, func, label, ln, text, restore) in d:
            print(f"DEFECT {path}:{ln}: {func} block {label}: vector code in front of `{restore}`: {text}")
        print(f"{p}: {len(d)} vector instruction(s) in front of a join's exec restore")
        bad += len(d)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
