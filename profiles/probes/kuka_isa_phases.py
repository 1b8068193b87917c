"""Static issue cost of the phases of a Kuka step, read from the PROFILING build's code object (make -C robotics-rl-srl_amd/csrc prof):
the instructions between two shader-clock stamps of tphysics_step, by kind.  With one wavefront per SIMD every instruction takes one
issue slot of ~4 cycles (VALU, SALU, LDS, waitcnt alike) and `s_nop N` takes N + 1 of them; float64 v_rcp / v_sqrt / v_rsq are
quarter rate (16 cycles).  Phase numbers are the stamp slots of profiles/probes/kuka_tree_phases.py.  Static counts: code behind a
branch a step does not take is counted too (the IK's four quaternion cases, the collision test's near path).  A row is labelled by
the slot of the LDS write that follows its stamp; the labels of phases 1-6 are checked by hand, later ones can be off by a phase.
usage (CPU): python profiles/probes/kuka_isa_phases.py [object=robotics-rl-srl_amd/csrc/build/kuka_tree_prof.hip.o] [kernel-regex]"""
import os
import re
import subprocess
import sys
import tempfile

OBJ = sys.argv[1] if len(sys.argv) > 1 else "robotics-rl-srl_amd/csrc/build/kuka_tree_prof.hip.o"
KERNEL = sys.argv[2] if len(sys.argv) > 2 else r"kuka_tree_rollout_kILi1ELb0ELb0ELi1ELi0ELi1ELi0EE"     # the SPEC instantiation, Philox
LLVM = "/opt/rocm/lib/llvm/bin"
SLOTS = 22      # kProfSlots: the running stamp lives in slot 22

with tempfile.TemporaryDirectory() as tmp:
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "co")
    subprocess.check_call([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, OBJ])
    tgt = [t for t in subprocess.check_output([LLVM + "/clang-offload-bundler", "--list", "--type=o", "--input=" + fat], text=True).split()
           if "gfx950" in t][0]
    subprocess.check_call([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat, "--targets=" + tgt, "--output=" + co])
    dis = subprocess.check_output([LLVM + "/llvm-objdump", "-d", "--mcpu=gfx950", co], text=True)

m = re.search(r"^[0-9a-f]+ <(\w*" + KERNEL + r"\w*)>:\n", dis, re.M)
body = dis[m.end():dis.find("\n\n", m.end())]
ins = [l.split("//")[0].strip() for l in body.split("\n") if l.startswith("\t")]
stamps = [i for i, s in enumerate(ins) if s.startswith("s_memtime")]
print("kernel", m.group(1)[:90], "|", len(ins), "instructions,", len(stamps), "stamps")
print("%5s %6s %6s %5s %5s %5s %5s %8s %11s" % ("phase", "instr", "valu", "dpp", "f64q", "nops", "slots", "issue_cy", "valu_cy"))
prev = 0
for i in stamps:
    seg = ins[prev:i]
    prev = i
    post = " ".join(s for s in ins[i:i + 40] if s.startswith("ds_write"))
    w = re.search(r"offset0:(\d+) offset1:(\d+)", post)
    if not w:
        continue
    slot = int(w.group(1)) - (int(w.group(2)) - SLOTS)
    nops = [s for s in seg if s.startswith("s_nop")]
    nop_slots = sum(int(s.split()[1], 0) + 1 for s in nops)
    valu = sum(s.startswith("v_") for s in seg)
    dpp = sum("_dpp" in s for s in seg)
    q = sum(bool(re.match(r"v_(rcp|sqrt|rsq)_f64", s)) for s in seg)
    slots = len(seg) - len(nops) + nop_slots
    print("%5d %6d %6d %5d %5d %5d %5d %8d %11d" % (slot, len(seg), valu, dpp, q, nop_slots, slots, 4 * slots + 12 * q, 4 * valu + 12 * q))
