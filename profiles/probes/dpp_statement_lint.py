#!/usr/bin/env python
"""ISA lint for the multi-instruction DPP statements of the Kuka kernels (csrc/kuka_tree.hpp: msum3, dot6_all12, dot6_arm,
transpose_low), on the BUILT object.  Such a statement writes accumulators before it has read all of its inputs; its outputs are
early-clobber so that no input shares a register with one.  The compiler cannot see inside the statement, so the result is checked
on the code it produced:

Rule S (aliasing): inside a run of consecutive v_fmac_f64_dpp instructions (`s_nop` between them allowed: the statements' own
hazard nops), no instruction reads as src0 / src1 a register that an earlier instruction of the same run wrote.  This is what an
input allocated onto an output register looks like (asm outputs without early-clobber: low[j] on M[j]).

The wait states of the DPP SOURCE (src0) are rule C of mfma_asm_hazard_lint.py, over every DPP instruction of the object.  The
accumulators are not checked: the compiler-scheduled one-instruction statements (fmac_bcast) re-read an accumulator fewer than 2 wait
states after its write throughout the kernels, code the GPU suite has always passed with — the DPP read hazard is the permuted
source's.  The statements above still re-read each accumulator no sooner than three instructions after its write.

    python profiles/probes/dpp_statement_lint.py [object=robotics-rl-srl_amd/csrc/build/kuka_tree.hip.o]
exit status 1 and one line per violation if any; used by tests/test_isa_lint_dpp_statements.py."""
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("mfma_asm_hazard_lint", os.path.join(HERE, "mfma_asm_hazard_lint.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)

FMAC = "v_fmac_f64_dpp"
MIN_RUN = 3        # runs this long or longer are multi-instruction statements (fmac_bcast is one instruction per statement)


def runs(seq):
    """Maximal runs of v_fmac_f64_dpp, s_nop allowed inside: lists of (index in seq, Ins)."""
    cur = []
    for k, ins in enumerate(seq):
        if ins.mnem == FMAC or (ins.mnem == "s_nop" and cur):
            cur.append((k, ins))
            continue
        if cur:
            yield cur
        cur = []
    if cur:
        yield cur


def operands(ins):
    ops = [o.strip() for o in ins.ops.split(",")]
    dst = H.regs_of(ops[0])
    src0 = H.regs_of(ops[1].split()[0]) if len(ops) > 1 else set()
    src1 = H.regs_of(ops[2].split()[0]) if len(ops) > 2 else set()
    return dst, src0, src1


def check(name, seq, found):
    """Rule S over one kernel's instructions; appends violations to `found`, returns (runs checked, instructions in them)."""
    n_runs = n_ins = 0
    for run in runs(seq):
        fm = [i for _, i in run if i.mnem == FMAC]
        if len(fm) < MIN_RUN:
            continue
        n_runs += 1
        n_ins += len(fm)
        written = {}
        for ins in fm:
            dst, src0, src1 = operands(ins)
            for what, regs in (("src0", src0), ("src1", src1)):
                hit = regs & set(written)
                if hit:
                    w = written[sorted(hit)[0]]
                    found.append("S %s: %s %s at 0x%x reads as %s a register written by %s at 0x%x in the same statement" % (
                        name[:70], ins.mnem, ins.ops.strip(), ins.addr, what, w.ops.strip(), w.addr))
            for r in dst:
                written[r] = ins
    return n_runs, n_ins


def lint(obj):
    """(violations, number of runs checked, number of instructions in them)"""
    found, n_runs, n_ins = [], 0, 0
    for name, seq in H.kernels(H.disassemble(obj)).items():
        r, i = check(name, seq, found)
        n_runs += r
        n_ins += i
    return found, n_runs, n_ins


if __name__ == "__main__":
    repo = os.path.dirname(os.path.dirname(HERE))
    obj = sys.argv[1] if len(sys.argv) > 1 else os.path.join(repo, "robotics-rl-srl_amd", "csrc", "build", "kuka_tree.hip.o")
    found, n_runs, n_ins = lint(obj)
    print("%d multi-instruction DPP runs, %d v_fmac_f64_dpp in them" % (n_runs, n_ins))
    for f in found[:50]:
        print("HAZARD " + f)
    print("%d violation(s)" % len(found))
    sys.exit(1 if found else 0)
