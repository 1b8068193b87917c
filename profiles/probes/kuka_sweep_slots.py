#!/usr/bin/env python
"""Issue slots of the contact-free solver of a Kuka step (csrc/kuka_tree.hpp sweeps_free), counted on the BUILT object of the
configuration-specialised rollout kernel.  With one wavefront per SIMD every instruction the wavefront issues takes an issue slot of
~4 cycles, `s_nop N` takes N + 1 (profiles/NOTES.md section AB), so what is not a row instruction is overhead that can be read off
the code object without a GPU.  Three blocks are found by their shape:

  * the free-sweep loop: the backward branch whose body is nothing but solver rows
        v_add_f64 t, cs, acc clamp / v_fma_f64 acc, -e, acc, acc / <one slot> / v_fmac_f64_dpp acc, t, n [/ a second v_fmac_f64_dpp]
    s_nop and scalar instructions.  Per trip: row instructions, s_nop inside rows (the <one slot>), boundary slots (s_nop between
    rows: what the compiler puts around an asm statement), loop control (the scalar instructions), and the branch, which is
    listed but not counted: the count is of s_nop, SALU and VALU slots, as section AB's was.
  * the last sweep: from the loop's exit to the last row that follows it; its <one slot> may be the capture of u (a v_fma_f64).
  * the lane-mask block in front of the first sweep: v_cmp_eq_u32 / s_nop / v_cndmask_b32 and the moves between them.

    python profiles/probes/kuka_sweep_slots.py [object=robotics-rl-srl_amd/csrc/build/kuka_tree.hip.o] [kernel-regex]
used by tests/test_isa_sweep_slots.py."""
import importlib.util
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("mfma_asm_hazard_lint", os.path.join(HERE, "mfma_asm_hazard_lint.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)

SPEC_KERNEL = r"kuka_tree_rollout_k<1, false, false, 1, 0, 1, 0, 0>"       # bench.py's headline: one button, Philox, SPEC
ROWS = 12               # motor rows per sweep (the button's three ride on rows 0..2 as second v_fmac_f64_dpp)
ROW_SLOTS = 51          # 12 x (add, fma, <one slot>, fmac_dpp) + 3 button fmac_dpp
MASK_BLOCK = ("v_cmp_eq_u32", "v_cndmask_b32", "v_mov_b32", "v_mov_b64", "v_add_f64", "s_nop", "s_mov_b32", "s_movk_i32")


def _is(ins, name):
    return ins.mnem == name or ins.mnem.startswith(name + "_e")


def _salu(ins):
    return ins.mnem.startswith("s_") and ins.mnem != "s_nop" and ins.target is None and not ins.mnem.startswith("s_waitcnt")


def row_at(seq, k):
    """Number of instructions of the solver row that starts at seq[k] (0: none), and the row's middle instruction."""
    if k + 3 >= len(seq) or not (_is(seq[k], "v_add_f64") and "clamp" in seq[k].ops and _is(seq[k + 1], "v_fma_f64")):
        return 0, None
    mid = seq[k + 2]
    if not (mid.mnem == "s_nop" or _is(mid, "v_fma_f64")) or seq[k + 3].mnem != "v_fmac_f64_dpp":
        return 0, None
    return (5 if k + 4 < len(seq) and seq[k + 4].mnem == "v_fmac_f64_dpp" else 4), mid


def count(seq):
    """Slot counts of a run of instructions, by kind; None if it holds anything but rows, s_nop, scalar instructions and branches."""
    c = {"rows": 0, "row_instr": 0, "row_nop_slots": 0, "row_nop_max": -1, "captures_in_rows": 0, "boundary_slots": 0,
         "loop_control": 0, "other_valu": 0, "branches": 0, "foreign": 0}
    k = 0
    while k < len(seq):
        n, mid = row_at(seq, k)
        if n:
            c["rows"] += 1
            c["row_instr"] += n - 1
            if mid.mnem == "s_nop":
                c["row_nop_slots"] += mid.ws
                c["row_nop_max"] = max(c["row_nop_max"], mid.ws - 1)
            else:
                c["captures_in_rows"] += 1
            k += n
            continue
        ins = seq[k]
        if ins.mnem == "s_nop":
            c["boundary_slots"] += ins.ws
        elif ins.target is not None:
            c["branches"] += 1
        elif _salu(ins):
            c["loop_control"] += 1
        elif ins.mnem.startswith("v_"):
            c["other_valu"] += 1
        else:
            c["foreign"] += 1
        k += 1
    c["slots"] = c["row_instr"] + c["row_nop_slots"] + c["captures_in_rows"] + c["boundary_slots"] + c["loop_control"] + c["other_valu"]
    return c


def probe(obj, kernel=SPEC_KERNEL):
    """{"loop": counts per trip (+ "sweeps"), "last": counts of the last sweep, "masks": counts of the mask block}"""
    seqs = [s for name, s in H.kernels(H.disassemble(obj)).items() if re.search(re.escape(kernel) if kernel == SPEC_KERNEL else kernel, name)]
    assert len(seqs) == 1, "kernel %r: %d matches" % (kernel, len(seqs))
    seq = seqs[0]
    index = {i.addr: k for k, i in enumerate(seq)}
    loops = []
    for k, ins in enumerate(seq):
        if ins.target is not None and ins.target <= ins.addr and ins.target in index:
            c = count(seq[index[ins.target]:k + 1])
            if c["rows"] >= ROWS and c["rows"] % ROWS == 0 and not c["foreign"] and not c["other_valu"]:
                loops.append((index[ins.target], k, c))
    assert len(loops) == 1, "free-sweep loops found: %d" % len(loops)
    head, end, loop = loops[0]
    loop["sweeps"] = loop["rows"] // ROWS
    # the last sweep: the next ROWS rows after the loop's exit
    k, rows, stop = end + 1, 0, end + 1
    while rows < ROWS and k < len(seq):
        n, _ = row_at(seq, k)
        if n:
            rows += 1
            stop = k + n
            k += n
        else:
            k += 1
    last = count(seq[end + 1:stop])
    # the first sweep: the rows (and the loop's set-up) in front of the loop head; the mask block ends where it starts
    k = head
    while k > 0:
        back = [b for b in (5, 4) if k - b >= 0 and row_at(seq, k - b)[0] == b]
        if back:
            k -= back[0]
        elif seq[k - 1].mnem == "s_nop" or _salu(seq[k - 1]) or _is(seq[k - 1], "v_mov_b64"):
            k -= 1
        else:
            break
    first = k
    while k > 0 and any(_is(seq[k - 1], m) for m in MASK_BLOCK) and "clamp" not in seq[k - 1].ops:
        k -= 1
    blk = seq[k:first]
    masks = {"v_cmp": sum(_is(i, "v_cmp_eq_u32") for i in blk), "v_cndmask": sum(_is(i, "v_cndmask_b32") for i in blk),
             "nop_slots": sum(i.ws for i in blk if i.mnem == "s_nop"), "other": sum(not (_is(i, "v_cmp_eq_u32") or _is(i, "v_cndmask_b32") or i.mnem == "s_nop") for i in blk),
             "slots": sum(i.ws for i in blk)}
    return {"loop": loop, "last": last, "masks": masks}


def report(r):
    lp, la, mk = r["loop"], r["last"], r["masks"]
    out = ["free-sweep loop: %d sweeps per trip, %d slots per trip = %.2f per sweep (+ %d branch, not counted)" % (
               lp["sweeps"], lp["slots"], lp["slots"] / lp["sweeps"], lp["branches"]),
           "    row instructions %d | s_nop inside rows %d (longest: s_nop %d) | boundary slots %d | loop control %d" % (
               lp["row_instr"], lp["row_nop_slots"], lp["row_nop_max"], lp["boundary_slots"], lp["loop_control"]),
           "last sweep: %d slots" % la["slots"],
           "    row instructions %d | s_nop inside rows %d | captures inside rows %d | boundary slots %d | scalar %d | other VALU (captures between rows) %d" % (
               la["row_instr"], la["row_nop_slots"], la["captures_in_rows"], la["boundary_slots"], la["loop_control"], la["other_valu"]),
           "mask block in front of the first sweep: %d slots" % mk["slots"],
           "    v_cmp_eq_u32 %d | v_cndmask_b32 %d | s_nop slots %d | other (moves, the button lanes' adds) %d" % (
               mk["v_cmp"], mk["v_cndmask"], mk["nop_slots"], mk["other"])]
    return "\n".join(out)


if __name__ == "__main__":
    repo = os.path.dirname(os.path.dirname(HERE))
    obj = sys.argv[1] if len(sys.argv) > 1 else os.path.join(repo, "robotics-rl-srl_amd", "csrc", "build", "kuka_tree.hip.o")
    print(report(probe(obj, sys.argv[2] if len(sys.argv) > 2 else SPEC_KERNEL)))
