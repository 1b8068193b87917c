#!/usr/bin/env python
"""Issue slots of the SETUP of a Kuka contact step (csrc/kuka_tree.hpp general_path, everything around the sweeps), counted on the
PROFILING build's code object (make -C robotics-rl-srl_amd/csrc prof) of the configuration-specialised rollout kernel — the companion
of kuka_isa_phases.py (the straight-line phases) and kuka_contact_sweep_slots.py (the contact sweeps).  Same rule: one wavefront per
SIMD pays an issue slot of ~4 cycles for every instruction, `s_nop N` pays N + 1, a branch is priced at 6 slots (profiles/NOTES.md
sections AB, AH, AI).  No GPU.

The code between two shader-clock stamps (s_memtime; the stamp's slot is read from the LDS write behind it, as kuka_isa_phases.py
does, relative to the running stamp's slot) is one segment: 8 -> 12 candidates -> row definitions, 12 -> 13 W J, 13 -> 14 the own bank-B row, 15 -> 16 the outputs.  Per
segment:
  static     every instruction of the segment once, by kind: VALU, SALU, LDS, s_nop (N + 1 slots), waitcnt, other, branches (x 6)
  loops      the backward branches inside the segment: body slots (priced) of each, in address order
  executed   an ESTIMATE for a step with one normal and one friction row (NG = 1, two used slots): straight-line code once, every
             loop body times the trip count the source gives it (TRIPS below, in address order of the loops; a loop the NG = 1 step
             does not enter has 0 trips).  Code behind a forward branch the step does not take is still counted once: an upper bound.
Limits of the estimate: trip counts are matched to loops by ADDRESS ORDER and are written down by hand per setup shape — "lanes"
(the one-button setup of section AJ, what the SPEC kernel compiles today) and "rolled" (the setup before it, which Kuka2Button /
KukaRandButton still compile; kept so that AJ's before-table can be reproduced from the commit before it).  A code-generation change
that adds, drops or reorders a loop makes the table wrong: with another loop COUNT the estimate is n/a, with the same count the
reader has to compare the printed loop bodies with the comments of TRIPS — the loop list is printed for that.  Block placement can
put a sweep loop of cn_sweeps<NG> between two setup stamps; a loop body above FOREIGN_LOOP_SLOTS is left out of the segment (and
reported in the `foreign` column), and whatever straight-line setup code the compiler placed behind it is then missing from the
segment: the static figures of two builds are comparable only where `foreign` is 0 in both.

    python profiles/probes/kuka_contact_setup_slots.py [object=robotics-rl-srl_amd/csrc/build/kuka_tree_prof.hip.o] [lanes|rolled]
"""
import importlib.util
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("kuka_sweep_slots", os.path.join(HERE, "kuka_sweep_slots.py"))
F = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(F)
H, _salu, SPEC_KERNEL = F.H, F._salu, F.SPEC_KERNEL

PROF_SLOTS = 22          # kProfSlots: the running stamp lives in slot 22
BRANCH_SLOTS = 6
FOREIGN_LOOP_SLOTS = 500    # a loop body this long is a solver sweep, not setup code
SEGMENTS = {12: "8 -> 12 candidates -> row definitions", 13: "12 -> 13 W J", 14: "13 -> 14 own bank-B row", 16: "15 -> 16 outputs"}
KINDS = ("valu", "salu", "lds", "nop", "waitcnt", "other")
# Trip counts of the loops of each segment for an NG = 1 contact step without a joint-limit row, in address order, read off
# general_path (SPEC instantiation: NB = 1, one friction direction).  None: not written down for this build — no estimate.
TRIPS = {
    # rolled: 8->12  put_limit's J fill (x2: lower / upper; not entered), put_contact's 12 Jacobian trips as 3 x `unroll 4` (cap and
    #                base copies: one of them runs), the wany loop over kNGen (6);  12->13 the 12 slots as 6 x `unroll 2`;
    #         13->14 diag / jv / offb 3 x `unroll 4`, NBA 3 x `unroll 5`, NBB 6 x `unroll 2`;  15->16 the 12 slots
    "rolled": {12: (0, 0, 3, 0), 13: (6, 6), 14: (3, 3, 6), 16: ()},
    # lanes:  8->12  put_limit's J fill (x2, not entered), the wany loop (6), the per-lane Jacobian loop (1 trip: one normal slot);
    #         12->13 two ranges (normal, friction) of one used slot each;  13->14 diag 3 x `unroll 4`, NBA 3 x `unroll 4`, NBB two
    #         ranges of one;  15->16 two ranges of one
    "lanes": {12: (0, 0, 6, 1), 13: (1, 1), 14: (3, 3, 1, 1), 16: (1, 1)},
}


def kind(ins):
    if ins.mnem == "s_nop":
        return "nop"
    if ins.mnem == "s_waitcnt":
        return "waitcnt"
    if ins.mnem.startswith("ds_"):
        return "lds"
    if ins.mnem.startswith("v_"):
        return "valu"
    if _salu(ins):
        return "salu"
    return "other"


def slots_of(seq):
    c = dict.fromkeys(KINDS, 0)
    c["branches"] = 0
    for ins in seq:
        if ins.target is not None:
            c["branches"] += 1
        else:
            c[kind(ins)] += ins.ws
    c["slots"] = sum(c[k] for k in KINDS)
    c["priced"] = c["slots"] + BRANCH_SLOTS * c["branches"]
    return c


def stamp_writes(seq, k):
    """(offset0, offset1) of the first ds_write2 behind the stamp at seq[k]: its phase slot and (usually) the running stamp's"""
    for ins in seq[k:k + 40]:
        if ins.mnem.startswith("ds_write2"):
            w0, w1 = re.search(r"offset0:(\d+)", ins.ops), re.search(r"offset1:(\d+)", ins.ops)
            return (int(w0.group(1)) if w0 else 0, int(w1.group(1)) if w1 else 0)
    return None


def probe(obj, kernel=SPEC_KERNEL):
    """{stamp slot: {"static": counts, "loops": [counts of each loop body], "straight": counts outside every loop}}"""
    seqs = [s for name, s in H.kernels(H.disassemble(obj)).items() if re.search(re.escape(kernel), name)]
    assert len(seqs) == 1, "kernel %r: %d matches" % (kernel, len(seqs))
    seq = seqs[0]
    stamps = [k for k, i in enumerate(seq) if i.mnem == "s_memtime"]
    assert stamps, "no stamps: not the profiling build"
    writes = {k: stamp_writes(seq, k) for k in stamps}
    firsts = [w[1] for w in writes.values() if w]
    running = max(set(firsts), key=firsts.count)          # the running stamp's LDS slot: what most stamps write second (stamp 8 shares its write with a counter)
    out, prev = {}, 0
    for k in stamps:
        slot, seg = (writes[k][0] - (running - PROF_SLOTS) if writes[k] else None), seq[prev:k]
        prev = k
        if slot not in SEGMENTS:
            continue
        assert slot not in out, "two segments end in stamp %d" % slot
        index = {i.addr: n for n, i in enumerate(seg)}
        loops, inside = [], set()
        for n, ins in enumerate(seg):
            if ins.target is not None and ins.target <= ins.addr and ins.target in index:
                loops.append((index[ins.target], n))
        outer = [l for l in loops if not any(o[0] <= l[0] and l[1] <= o[1] and o != l for o in loops)]      # nested loops count with their outer loop's body
        # block placement can put a sweep loop of cn_sweeps<NG> between two stamps of the setup: not this segment's code
        foreign = [l for l in outer if slots_of(seg[l[0]:l[1] + 1])["priced"] > FOREIGN_LOOP_SLOTS]
        skip = set()
        for a, b in foreign:
            skip.update(range(a, b + 1))
        outer = [l for l in outer if l not in foreign]
        for a, b in outer:
            inside.update(range(a, b + 1))
        out[slot] = {"static": slots_of([i for n, i in enumerate(seg) if n not in skip]), "loops": [slots_of(seg[a:b + 1]) for a, b in outer],
                     "nested": sum(1 for l in loops if l not in outer and not any(f[0] <= l[0] and l[1] <= f[1] for f in foreign)),
                     "foreign": len(foreign), "straight": slots_of([i for n, i in enumerate(seg) if n not in inside and n not in skip])}
    return out


def executed(r, trips):
    if trips is None or len(trips) != len(r["loops"]):
        return None
    return r["straight"]["priced"] + sum(t * l["priced"] for t, l in zip(trips, r["loops"]))


def report(res, build):
    out = ["| segment | VALU | SALU | LDS | s_nop | waitcnt | other | branches (x%d) | static priced | loops: body priced (nested inside) | foreign | executed, NG = 1 |" % BRANCH_SLOTS,
           "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    total = 0
    for slot in sorted(res):
        r, c = res[slot], res[slot]["static"]
        ex = executed(r, TRIPS[build][slot])
        total = None if ex is None or total is None else total + ex
        out.append("| %s | %d | %d | %d | %d | %d | %d | %d | %d | %s (%d) | %d | %s |" % (
            SEGMENTS[slot], c["valu"], c["salu"], c["lds"], c["nop"], c["waitcnt"], c["other"], c["branches"], c["priced"],
            " / ".join(str(l["priced"]) for l in r["loops"]) or "-", r["nested"], r["foreign"], "n/a" if ex is None else str(ex)))
    out.append("executed estimate of the four segments, NG = 1: %s slots" % ("n/a" if total is None else total))
    return "\n".join(out)


if __name__ == "__main__":
    repo = os.path.dirname(os.path.dirname(HERE))
    obj = sys.argv[1] if len(sys.argv) > 1 else os.path.join(repo, "robotics-rl-srl_amd", "csrc", "build", "kuka_tree_prof.hip.o")
    build = sys.argv[2] if len(sys.argv) > 2 else "lanes"
    print(report(probe(obj), build))
