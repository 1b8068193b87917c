#!/usr/bin/env python
"""Issue slots of the one-button CONTACT sweeps of a Kuka step (csrc/kuka_tree.hpp cn_sweeps<NG>), counted on the BUILT object of the
configuration-specialised rollout kernel — the companion of kuka_sweep_slots.py (the contact-free sweeps), same rule: one wavefront
per SIMD pays an issue slot of ~4 cycles for every instruction, `s_nop N` pays N + 1, a taken branch ~6 slots (profiles/NOTES.md
sections AB, AH, AI).  No GPU.

The sweep loop of each NG instantiation is found by its shape: a backward branch whose body holds
  * 12 bank-A rows  v_add_f64 t, cs, accA clamp / v_fma_f64 accA, -e, accA, accA / ... / v_fmac_f64_dpp (same cs, same accA), whose
    v_fmac_f64_dpp write exactly two accumulators (accA, accB): 30 of them with the button's rows riding on rows 0..2,
  * NG normal rows     v_add_f64 t, csU, accB clamp / v_fma_f64 / <one slot> / two v_fmac_f64_dpp,
  * NG friction rows   v_fmac_f64_dpp hi, tN, mu (onto a zero) / v_add_f64 / v_max_f64 / v_min_f64 / v_cmp_lt_f64 / two v_cndmask_b32
    / v_fma_f64 / two v_fmac_f64_dpp,
and nothing else but moves, s_nop and scalar instructions.  Per trip (= per sweep) it reports
  row_instr      v_add_f64, v_fma_f64, v_fmac_f64_dpp: the instructions the asm statements of the rows hold, and the friction row's add
  row_nop_slots  s_nop inside rows: the `s_nop 0` between a row's restart v_fma_f64 and its v_fmac_f64_dpp, the `s_nop 1` a DPP statement opens with
  boundary_slots every other s_nop: what the compiler puts around an asm statement
  valu_moves / valu_minmax / valu_cmp / valu_cndmask   compiler-scheduled VALU between the statements
  salu           scalar instructions (the loop counter, its compare)
  branches       listed apart; `slots_priced` adds six slots for each (section AH: a taken branch costs a lone wavefront ~23 cycles)
  bank_a_instr   row_instr in front of the first bank-B row (54: csrc/kuka_tree.hpp cn_phaseA)

    python profiles/probes/kuka_contact_sweep_slots.py [object=robotics-rl-srl_amd/csrc/build/kuka_tree.hip.o] [kernel-regex]
used by tests/test_isa_contact_sweep_slots.py."""
import importlib.util
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("kuka_sweep_slots", os.path.join(HERE, "kuka_sweep_slots.py"))
F = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(F)
H, _is, _salu, SPEC_KERNEL = F.H, F._is, F._salu, F.SPEC_KERNEL

ROWS_A = 12             # bank-A rows per sweep
DPP_A = 30              # their v_fmac_f64_dpp: 12 rows x 2 accumulators + the button's 3 rows x 2
BANK_A_INSTR = 54       # cn_phaseA: 12 v_add_f64 + 12 restart v_fma_f64 + 30 v_fmac_f64_dpp
BRANCH_SLOTS = 6
# Floors per trip (profiles/NOTES.md section AI).  Bank A as cn_phaseA schedules it: 12 x (add, restart) + 30 fmac_dpp = 54 VALU and
# the one s_nop 0 of row 0 (nothing is deferred into the first row's wait state): 55.  A normal row: add, restart, one wait slot, two
# fmac_dpp = 5.  A friction row: zero, fmac_dpp hi, add, max, min, cmp, two cndmask, restart, two fmac_dpp = 12 (its two wait states
# between the last v_cndmask and the spreading DPP hold the restart and a neighbour's instruction).  Loop control: 2.
FLOOR_A, FLOOR_N, FLOOR_F, FLOOR_LOOP = 55, 5, 12, 2


def floor(ng):
    return FLOOR_A + ng * (FLOOR_N + FLOOR_F) + FLOOR_LOOP


def _ops(ins):
    return [o.strip() for o in ins.ops.split(",")]


def count(seq):
    """Slot counts of one trip by kind, and the sweep's shape (None where it is no contact sweep)."""
    c = {"row_instr": 0, "row_nop_slots": 0, "boundary_slots": 0, "valu_moves": 0, "valu_minmax": 0, "valu_cmp": 0, "valu_cndmask": 0,
         "salu": 0, "branches": 0, "foreign": 0, "dpp": 0}
    clamp_adds, plain_adds, dpp_dst_a = [], 0, set()
    first_b = None                   # index of the first bank-B row: the 13th clamped add, or the first add whose cs differs
    for k, ins in enumerate(seq):
        nxt = seq[k + 1] if k + 1 < len(seq) else None
        prv = seq[k - 1] if k else None
        if ins.mnem == "s_nop":
            own = nxt is not None and nxt.mnem == "v_fmac_f64_dpp" and (ins.ws == 2 or (prv is not None and _is(prv, "v_fma_f64")))
            c["row_nop_slots" if own else "boundary_slots"] += ins.ws
        elif ins.target is not None:
            c["branches"] += 1
        elif _salu(ins):
            c["salu"] += 1
        elif _is(ins, "v_add_f64") or _is(ins, "v_fma_f64") or ins.mnem == "v_fmac_f64_dpp":
            c["row_instr"] += 1
            if _is(ins, "v_add_f64"):
                if "clamp" in ins.ops:
                    o = _ops(ins)
                    clamp_adds.append((o[1], o[2].replace("clamp", "").strip()))
                    if first_b is None and (len(clamp_adds) > ROWS_A or clamp_adds[-1] != clamp_adds[0]):
                        first_b = k
                else:
                    plain_adds += 1
                    if first_b is None:
                        first_b = k
            if ins.mnem == "v_fmac_f64_dpp":
                c["dpp"] += 1
                if first_b is None:
                    dpp_dst_a.add(_ops(ins)[0])
        elif _is(ins, "v_mov_b64") or _is(ins, "v_mov_b32") or ins.mnem.startswith("v_accvgpr"):
            c["valu_moves"] += 1
        elif _is(ins, "v_max_f64") or _is(ins, "v_min_f64"):
            c["valu_minmax"] += 1
        elif ins.mnem.startswith("v_cmp_"):
            c["valu_cmp"] += 1
        elif _is(ins, "v_cndmask_b32"):
            c["valu_cndmask"] += 1
        else:
            c["foreign"] += 1
    ng = len(clamp_adds) - ROWS_A
    c["bank_a_instr"] = sum(1 for i in seq[:first_b if first_b is not None else len(seq)]
                            if _is(i, "v_add_f64") or _is(i, "v_fma_f64") or i.mnem == "v_fmac_f64_dpp")
    c["slots"] = (c["row_instr"] + c["row_nop_slots"] + c["boundary_slots"] + c["valu_moves"] + c["valu_minmax"] + c["valu_cmp"] + c["valu_cndmask"] + c["salu"])
    c["slots_priced"] = c["slots"] + BRANCH_SLOTS * c["branches"]
    shape = (not c["foreign"] and ng >= 0 and len(clamp_adds) >= ROWS_A and len(set(clamp_adds[:ROWS_A])) == 1
             and (ng == 0 or clamp_adds[ROWS_A] != clamp_adds[0]) and len(set(clamp_adds[ROWS_A:])) <= 1
             and plain_adds == ng and c["valu_minmax"] == 2 * ng and c["valu_cmp"] == ng and c["valu_cndmask"] == 2 * ng
             and c["dpp"] == DPP_A + 5 * ng and (len(dpp_dst_a) == 2 or ng == 0))
    c["ng"] = ng if shape else None
    return c


def probe(obj, kernel=SPEC_KERNEL):
    """{NG: counts per trip of the contact sweep loop of cn_sweeps<NG>} for every instantiation found in the kernel"""
    seqs = [s for name, s in H.kernels(H.disassemble(obj)).items() if re.search(re.escape(kernel) if kernel == SPEC_KERNEL else kernel, name)]
    assert len(seqs) == 1, "kernel %r: %d matches" % (kernel, len(seqs))
    seq = seqs[0]
    index = {i.addr: k for k, i in enumerate(seq)}
    out = {}
    for k, ins in enumerate(seq):
        if ins.target is not None and ins.target <= ins.addr and ins.target in index:
            body = seq[index[ins.target]:k + 1]
            if 40 <= len(body) <= 400:
                c = count(body)
                if c["ng"] is not None:
                    assert c["ng"] not in out, "two contact sweep loops with NG = %d" % c["ng"]
                    out[c["ng"]] = c
    return out


def report(r):
    out = ["contact sweep loops (cn_sweeps<NG>), issue slots per trip = per sweep; floor = %d + %d NG + %d" % (FLOOR_A, FLOOR_N + FLOOR_F, FLOOR_LOOP),
           "| NG | row instr (bank A) | s_nop in rows | boundary s_nop | moves | max/min | cmp | cndmask | SALU | slots | branches (x%d) | priced | floor | removable |" % BRANCH_SLOTS,
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for ng in sorted(r):
        c = r[ng]
        out.append("| %d | %d (%d) | %d | %d | %d | %d | %d | %d | %d | %d | %d | %d | %d | %d |" % (
            ng, c["row_instr"], c["bank_a_instr"], c["row_nop_slots"], c["boundary_slots"], c["valu_moves"], c["valu_minmax"], c["valu_cmp"],
            c["valu_cndmask"], c["salu"], c["slots"], c["branches"], c["slots_priced"], floor(ng), c["slots"] - floor(ng)))
    return "\n".join(out)


if __name__ == "__main__":
    repo = os.path.dirname(os.path.dirname(HERE))
    obj = sys.argv[1] if len(sys.argv) > 1 else os.path.join(repo, "robotics-rl-srl_amd", "csrc", "build", "kuka_tree.hip.o")
    print(report(probe(obj, sys.argv[2] if len(sys.argv) > 2 else SPEC_KERNEL)))
