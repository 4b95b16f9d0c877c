#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of vectorwave_amd/csrc: tools/codeobj_compare.py DIR_A DIR_B

For every object (*.o) of each directory the offload bundle's gfx950 code object is extracted (llvm-objdump
--offloading).  Over the union of all objects of a build the two sets of kernel symbols must be equal, and per
kernel the code bytes (the symbol's range of .text), the metadata note entry (registers, scratch, LDS, kernarg and
wavefront size, ...) and the 64-byte .kd descriptor outside its entry offset.  Prints one line per difference and
a count; exit status 1 when anything differs.  LLVM_BIN names the directory of llvm-objdump / llvm-readelf."""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
NOTE_KEYS = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
             "kernarg_segment_size", "kernarg_segment_align", "wavefront_size", "max_flat_workgroup_size",
             "sgpr_spill_count", "vgpr_spill_count", "uses_dynamic_stack")


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def notes_of(co):
    """{kernel name: {key: value}} from the amdhsa.kernels list of the code object's metadata note."""
    out, cur, dash = {}, None, None
    for line in run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).splitlines():
        m = re.match(r"^(\s*)(- )?\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        indent, item, key, val = len(m.group(1)), m.group(2), m.group(3), m.group(4).strip().strip("'\"")
        if item and (dash is None or indent <= dash):  # a new entry of the outermost list: a kernel
            dash, cur = indent, {}
        if cur is not None and indent + (2 if item else 0) == dash + 2:
            cur[key] = val
            if key == "name":
                out[val] = cur
    return {k: {n: v.get(n) for n in NOTE_KEYS} for k, v in out.items()}


def kernels_of(build_dir, tmp):
    """{kernel: (object, code bytes, notes, descriptor bytes)} over every object of the directory."""
    found = {}
    for obj in sorted(glob.glob(os.path.join(build_dir, "*.o"))):
        base = os.path.basename(obj)
        link = os.path.join(tmp, base)
        os.symlink(os.path.abspath(obj), link)
        run(os.path.join(LLVM, "llvm-objdump"), "--offloading", base, cwd=tmp)
        cos = glob.glob(link + ".*gfx950*")
        os.unlink(link)
        for co in cos:
            data = open(co, "rb").read()
            secs = {}  # index -> (name, address, file offset)
            for line in run(os.path.join(LLVM, "llvm-readelf"), "-S", "-W", co).splitlines():
                m = re.match(r"^\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
                if m:
                    secs[m.group(1)] = (m.group(2), int(m.group(3), 16), int(m.group(4), 16))
            notes = notes_of(co)
            syms = {}
            for line in run(os.path.join(LLVM, "llvm-readelf"), "-s", "-W", co).splitlines():
                f = line.split()
                if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6] in secs:
                    name, addr, off = secs[f[6]]
                    a = int(f[1], 16)
                    syms[f[7]] = (f[3], name, data[a - addr + off: a - addr + off + int(f[2])])
            for name, (kind, sec, code) in syms.items():
                if kind != "FUNC":
                    continue
                kd = syms.get(name + ".kd", (None, None, None))[2]  # None: a device function, not a kernel
                if name in found:
                    print(f"DIFF {build_dir}: {name} defined in {found[name][0]} and {base}")
                found[name] = (base, sec, code, notes.get(name), kd)
            os.unlink(co)
    return found


def main():
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        A, B = kernels_of(a_dir, ta), kernels_of(b_dir, tb)
    diffs = 0
    for name in sorted(set(A) ^ set(B)):
        diffs += 1
        print(f"DIFF symbol only in {a_dir if name in A else b_dir}: {name} ({(A.get(name) or B.get(name))[0]})")
    moved = 0
    for name in sorted(set(A) & set(B)):
        (oa, sa, ca, na, ka), (ob, sb, cb, nb, kb) = A[name], B[name]
        if oa != ob:
            moved += 1
            print(f"MOVED {name}: {oa} -> {ob}")
        if sa != ".text" or sb != ".text" or ca != cb:
            diffs += 1
            print(f"DIFF code {name}: {sa} {len(ca)} bytes vs {sb} {len(cb)} bytes")
        if ka is None and kb is None:
            continue
        if na is None or na != nb:
            diffs += 1
            print(f"DIFF notes {name}: {na} vs {nb}")
        if not ka or not kb or len(ka) != 64 or ka[:16] + ka[24:] != kb[:16] + kb[24:]:  # bytes 16..23: entry offset
            diffs += 1
            print(f"DIFF descriptor {name}")
    print(f"{a_dir}: {len(A)} device functions; {b_dir}: {len(B)}; compared {len(set(A) & set(B))} "
          f"(code bytes, metadata notes, descriptors); moved between objects: {moved}; differences: {diffs}")
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
