#!/usr/bin/env python3
"""Compare the gfx950 ISA of two builds of the library kernel by kernel (symbol by symbol), without running anything.

    python tools/compare_isa.py OLD/libpasst_amd.so NEW/libpasst_amd.so

A kernel's instruction stream is its disassembly with the addresses and encodings stripped (branch operands are relative offsets), so
a kernel that merely moved inside its code object compares equal.  Prints one line per kernel
that differs, the kernels only one side has, and per new kernel its resources (VGPRs, scratch bytes) from the code object's metadata.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from so_isa import LLVM, code_objects, kernel_bodies  # noqa: E402


def streams(so):
    out = {}
    for _, text in code_objects(so):
        for name, body in kernel_bodies(text).items():
            lines = []
            for ln in body.splitlines():
                m = re.match(r"\s+(\S.*?)\s+//\s+[0-9A-Fa-f]+:", ln)
                if m:           # a branch prints its target's label in <...>; its operand itself is a relative offset
                    lines.append(re.sub(r"<[^>]*>", "", m.group(1)).strip())
            out[name] = lines
    return out


def resources(so):
    """{kernel: (vgprs, agprs, scratch bytes)} from the notes of every gfx950 code object"""
    import struct
    res = {}
    with tempfile.TemporaryDirectory() as d:
        fb = os.path.join(d, "fatbin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, so, os.path.join(d, "copy.so")],
                       check=True, capture_output=True)
        blob = open(fb, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        k = 0
        for m in re.finditer(re.escape(magic), blob):
            p = m.start()
            q = p + len(magic)
            n, = struct.unpack_from("<Q", blob, q)
            q += 8
            for _ in range(n):
                off, size, tl = struct.unpack_from("<QQQ", blob, q)
                q += 24
                triple = blob[q:q + tl].decode()
                q += tl
                if "gfx950" in triple and size:
                    co = os.path.join(d, f"co{k}.co")
                    k += 1
                    open(co, "wb").write(blob[p + off:p + off + size])
                    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True).stdout
                    for blk in notes.split(".agpr_count")[1:]:
                        name = re.search(r"\.name:\s+(\S+)", blk)
                        z = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                        v = re.search(r"\.vgpr_count:\s+(\d+)", blk)
                        a = re.match(r":\s+(\d+)", blk)
                        if name and z and v:
                            res[name.group(1)] = (int(v.group(1)), int(a.group(1)) if a else -1, int(z.group(1)))
    return res


def main(old, new):
    a, b = streams(old), streams(new)
    same = [k for k in a if k in b and a[k] == b[k]]
    diff = [k for k in a if k in b and a[k] != b[k]]
    print(f"kernels: {len(a)} old, {len(b)} new; {len(same)} identical instruction streams, {len(diff)} differ, "
          f"{len(set(a) - set(b))} only old, {len(set(b) - set(a))} only new")
    for k in diff:
        print(f"DIFFERS  {k}: {len(a[k])} -> {len(b[k])} instructions")
    for k in sorted(set(a) - set(b)):
        print(f"ONLY OLD {k}")
    res = resources(new)
    for k in sorted(set(b) - set(a)):
        v = res.get(k, (-1, -1, -1))
        print(f"ONLY NEW {k}: {len(b[k])} instructions, {v[0]} VGPRs, scratch {v[2]} B")
    return 1 if diff or set(a) - set(b) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
