"""Issue slots of the contact-free solver in the BUILT configuration-specialised Kuka rollout kernel (the one bench.py times), read
off the code object by profiles/probes/kuka_sweep_slots.py.  One wavefront per SIMD: every s_nop, scalar and vector instruction is
an issue slot of ~4 cycles (profiles/NOTES.md sections AB, AH).  A sweep is 51 slots of rows (36 row VALU, 3 button fmac, 12 wait-state
slots); a loop trip of K sweeps may add ONE slot that is not a row's (the trip counter), i.e. 51 + 1/K per sweep.  The branch is no
s_nop, SALU or VALU slot and is not counted (the two-statement form counted the same way: 53 per sweep).  No GPU needed."""
import importlib.util
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_ROW_NOP = 0          # the wait-state nop of a row has always been `s_nop 0`


def _probe():
    spec = importlib.util.spec_from_file_location("kuka_sweep_slots", os.path.join(REPO, "profiles", "probes", "kuka_sweep_slots.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _built(obj):
    """the object of csrc/build, built on demand (hipcc cross-compiles gfx950 without a GPU): the test never skips"""
    csrc = os.path.join(REPO, "robotics-rl-srl_amd", "csrc")
    path = os.path.join(csrc, "build", obj)
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", csrc, "build/" + obj], env=dict(os.environ, HIPCC=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    return path


def test_the_probe_counts_a_planted_trip():
    P = _probe()
    row = ["\tv_add_f64 v[12:13], v[126:127], v[204:205] clamp // 000000001000: D280800C 0003997E",
           "\tv_fma_f64 v[204:205], -v[20:21], v[204:205], v[204:205] // 000000001008: D1CC00CC 27339914",
           "\ts_nop 0 // 000000001010: BF800000",
           "\tv_fmac_f64_dpp v[204:205], v[12:13], v[242:243] row_newbcast:0 row_mask:0xf bank_mask:0xf // 000000001014: 0999E4FA FF01500C"]
    button = "\tv_fmac_f64_dpp v[204:205], v[12:13], v[142:143] row_newbcast:12 row_mask:0xf bank_mask:0xf // 00000000101C: 09991CFA FF015C0C"
    sweep = (row + [button]) * 3 + row * 9
    pad, long_nop = "\ts_nop 0 // 000000001024: BF800000", "\ts_nop 1 // 000000001010: BF800001"
    ctl = ["\ts_sub_u32 vcc_lo, vcc_lo, 1 // 000000001028: 80EA816A", "\ts_cbranch_scc0 65330 // 00000000102C: BF84FF32"]
    c = P.count([P.H.Ins(x) for x in sweep * 2 + ctl])
    assert (c["rows"], c["row_instr"], c["row_nop_slots"], c["row_nop_max"], c["boundary_slots"], c["loop_control"], c["branches"], c["slots"]) == (24, 78, 24, 0, 0, 1, 1, 103)
    c = P.count([P.H.Ins(x) for x in sweep + [pad] + sweep[:2] + [long_nop] + sweep[3:] + ctl])
    assert (c["boundary_slots"], c["row_nop_max"], c["slots"]) == (1, 1, 105)


def test_free_sweep_loop_of_the_specialised_kernel_pays_one_slot_per_trip():
    P = _probe()
    r = P.probe(_built("kuka_tree.hip.o"))
    print(P.report(r))
    lp = r["loop"]
    k = lp["sweeps"]
    assert k >= 1 and lp["row_instr"] == 39 * k and lp["row_nop_slots"] == 12 * k, lp      # the rows themselves: unchanged
    assert lp["slots"] <= P.ROW_SLOTS * k + 1, lp                                              # 51 + 1/K per sweep
    assert lp["row_nop_max"] <= PARENT_ROW_NOP, lp


def test_last_sweep_captures_inside_its_rows():
    """Twelve rows whose wait-state slot is the capture of u: 51 slots, plus one slot at each of the two statement boundaries (the
    compiler's pad, or an instruction of its own standing in for it)."""
    P = _probe()
    la = P.probe(_built("kuka_tree.hip.o"))["last"]
    assert la["rows"] == 12 and la["captures_in_rows"] == 12 and la["row_nop_slots"] == 0, la
    assert la["slots"] <= P.ROW_SLOTS + 2, la
