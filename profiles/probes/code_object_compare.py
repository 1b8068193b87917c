"""Compare the kernels of two builds of libsrlhip.so symbol by symbol: VGPR / AGPR / SGPR counts, VGPR / SGPR spills, LDS and
scratch (the code objects' metadata notes) and text size (their symbol tables), read from the gfx950 code objects inside .hip_fatbin.

    python profiles/probes/code_object_compare.py OLD/libsrlhip.so NEW/libsrlhip.so

Kernels are matched by demangled name; a template that gained a trailing defaulted parameter matches its old name with `, 0` appended.
Prints how many kernels each build has, which common kernels differ, which are gone, and the figures of the new ones."""
import glob
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
          "private_segment_fixed_size")


def extract_code_objects(lib, out_dir):
    """every gfx950 entry of every offload bundle in the library's .hip_fatbin section -> files in out_dir"""
    section = os.path.join(out_dir, "fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, section])
    with open(section, "rb") as f:
        data = f.read()
    pos, count = 0, 0
    while True:
        pos = data.find(BUNDLE_MAGIC, pos)
        if pos < 0:
            return
        entries, = struct.unpack_from("<Q", data, pos + len(BUNDLE_MAGIC))
        p = pos + len(BUNDLE_MAGIC) + 8
        for _ in range(entries):
            offset, size, id_len = struct.unpack_from("<QQQ", data, p)
            p += 24
            target = data[p:p + id_len].decode()
            p += id_len
            if "gfx950" in target and size:
                with open(os.path.join(out_dir, "co_%d.elf" % count), "wb") as f:
                    f.write(data[pos + offset:pos + offset + size])
                count += 1
        pos += len(BUNDLE_MAGIC)


def note_field(block, key):
    m = re.search(r"\.%s:\s+(\S+)" % key, block)
    return m.group(1) if m else None


def kernels_of(lib):
    """{mangled kernel name: (the FIELDS figures..., text bytes)}"""
    out_dir = tempfile.mkdtemp()
    try:
        extract_code_objects(lib, out_dir)
        out = {}
        for co in sorted(glob.glob(os.path.join(out_dir, "co_*.elf"))):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
            for block in notes.split("- .agpr_count:")[1:]:
                block = ".agpr_count:" + block
                out[note_field(block, "name")] = tuple(int(note_field(block, k) or -1) for k in FIELDS)
            symbols = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", co], capture_output=True, text=True, check=True).stdout
            for line in symbols.splitlines():
                cols = line.split()
                if len(cols) >= 8 and cols[3] == "FUNC" and cols[7] in out:
                    out[cols[7]] = out[cols[7]] + (int(cols[2]),)
        return out
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def demangled(kernels):
    names = subprocess.run(["c++filt"], input="\n".join(kernels), capture_output=True, text=True, check=True).stdout.splitlines()
    short = (n.replace("(anonymous namespace)::", "").replace("void ", "") for n in names)
    return {re.sub(r"\(.*", "", n): v for n, v in zip(short, kernels.values())}


def main():
    old, new = demangled(kernels_of(sys.argv[1])), demangled(kernels_of(sys.argv[2]))
    for name in list(old):
        if name not in new and name.endswith(">") and name[:-1] + ", 0>" in new:
            old[name[:-1] + ", 0>"] = old.pop(name)
    print("kernels:", len(old), "->", len(new))
    print("changed:", [(k, old[k], new[k]) for k in old if k in new and old[k] != new[k]])
    print("missing:", [k for k in old if k not in new])
    print("new kernels (vgpr, agpr, sgpr, vgpr_spill, sgpr_spill, lds, scratch, text):")
    for name in new:
        if name not in old:
            print("  ", name, new[name])


if __name__ == "__main__":
    main()
