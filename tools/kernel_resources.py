#!/usr/bin/env python3
"""Compare the resource metadata of every GPU kernel in two builds of libnnop_hip.so -- no GPU needed.

A change that adds kernel variants must leave the kernels that existed before as they were.  For every kernel symbol of the
PARENT library this reads the code objects' AMDGPU metadata notes (what the loader itself goes by) in both libraries and compares
VGPRs, AGPRs, SGPRs, spills, scratch bytes per lane, static LDS bytes and the wavefront size, and a hash of the kernel's machine-code
bytes (the function symbol's range in the code object: register figures alone do not show that no instruction moved).  Exit status 1
when a parent kernel is missing from the new library or a figure differs; kernels that only the new library has are listed with
their figures (a host-only change must report new: 0 as well).

    python tools/kernel_resources.py --parent /path/to/parent/libnnop_hip.so [--this nnop.jl_amd/lib/libnnop_hip.so]
                                     [--out profiles/r05/kernel_resources.txt] [--new-only-filter cap]

The code objects are found inside the host library's fat binary by their ELF headers (uncompressed bundles, which is what the
Makefile builds); the notes are read with llvm-readelf from $ROCM_PATH/llvm/bin (default /opt/rocm).
"""
import argparse
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

FIELDS = [("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("vspill", ".vgpr_spill_count"),
          ("sspill", ".sgpr_spill_count"), ("scratch", ".private_segment_fixed_size"), ("lds", ".group_segment_fixed_size"),
          ("wave", ".wavefront_size"), ("maxwg", ".max_flat_workgroup_size")]
EM_AMDGPU = 224


def code_objects(path):
    """every AMDGPU ELF image embedded in the file, as bytes"""
    data = open(path, "rb").read()
    out = []
    pos = 0
    while True:
        pos = data.find(b"\x7fELF", pos)
        if pos < 0:
            break
        hdr = data[pos:pos + 64]
        if len(hdr) == 64 and hdr[4] == 2 and hdr[5] == 1 and struct.unpack_from("<H", hdr, 18)[0] == EM_AMDGPU:
            shoff, = struct.unpack_from("<Q", hdr, 40)
            shentsize, shnum = struct.unpack_from("<HH", hdr, 58)
            size = shoff + shentsize * shnum                  # the section header table closes an image written by lld
            out.append(data[pos:pos + size])
            pos += max(size, 4)
        else:
            pos += 4
    return out


def code_hashes(img):
    """{function symbol: first 16 hex digits of the SHA-256 of its machine-code bytes} from one code object's symbol table"""
    shoff, = struct.unpack_from("<Q", img, 40)
    shentsize, shnum = struct.unpack_from("<HH", img, 58)
    # section header: name, type, flags, addr, offset, size, link, info, addralign, entsize
    secs = [struct.unpack_from("<IIQQQQIIQQ", img, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for _, typ, _, _, off, size, link, _, _, entsize in secs:
        if typ != 2:                                          # SHT_SYMTAB
            continue
        str_off = secs[link][4]
        for i in range(size // entsize):
            name, info, _, shndx, value, sz = struct.unpack_from("<IBBHQQ", img, off + i * entsize)
            if (info & 15) != 2 or sz == 0 or shndx == 0 or shndx >= shnum:      # STT_FUNC, defined
                continue
            end = img.index(b"\0", str_off + name)
            start = secs[shndx][4] + value - secs[shndx][3]
            out[img[str_off + name:end].decode()] = hashlib.sha256(img[start:start + sz]).hexdigest()[:16]
    return out


def readelf():
    return os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")


def kernels(path):
    """{demangled-free symbol name: {field: int, "code": hash}} over all code objects of the library"""
    res = {}
    for img in code_objects(path):
        hashes = code_hashes(img)
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(img)
            f.flush()
            txt = subprocess.run([readelf(), "--notes", f.name], check=True, capture_output=True, text=True).stdout
        # the metadata is YAML; its kernel entries start at "  - .agpr_count:" (keys sorted) -- split on list items of amdhsa.kernels
        m = re.search(r"amdhsa\.kernels:\n(.*?)\n\s*amdhsa\.", txt, re.S)
        if not m:
            continue
        for block in re.split(r"\n  - (?=\.)", "\n" + m.group(1)):
            name = re.search(r"\.name:\s+(\S+)", block)
            if not name:
                continue
            rec = {}
            for key, tag in FIELDS:
                v = re.search(r"\n?\s" + re.escape(tag) + r":\s+(\d+)", block)
                rec[key] = int(v.group(1)) if v else 0
            rec["code"] = hashes.get(name.group(1), "none")
            res[name.group(1)] = rec
    return res


def fmt(rec):
    return " ".join(f"{k}={rec[k]}" for k, _ in FIELDS) + f" code={rec['code']}"


def main():
    ap = argparse.ArgumentParser()
    here = os.path.dirname(os.path.abspath(__file__))
    ap.add_argument("--parent", required=True, help="libnnop_hip.so built from the parent commit")
    ap.add_argument("--this", default=os.path.join(here, "..", "nnop.jl_amd", "lib", "libnnop_hip.so"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--new-only-filter", default="", help="list only the new kernels whose name contains this")
    a = ap.parse_args()
    old, new = kernels(a.parent), kernels(a.this)
    lines = []
    missing = sorted(n for n in old if n not in new)
    differ = sorted(n for n in old if n in new and old[n] != new[n])
    added = sorted(n for n in new if n not in old)
    lines.append(f"parent kernels: {len(old)}   this build: {len(new)}   missing: {len(missing)}   differing: {len(differ)}   "
                 f"identical: {len(old) - len(missing) - len(differ)}   new: {len(added)}")
    lines.append("fields: " + ", ".join(k for k, _ in FIELDS) + ", code (hash of the machine-code bytes)")
    for n in missing:
        lines.append(f"MISSING {n}")
    for n in differ:
        lines.append(f"DIFFERS {n}\n    parent {fmt(old[n])}\n    this   {fmt(new[n])}")
    lines.append("")
    lines.append("new kernels:")
    for n in added:
        if a.new_only_filter in n:
            lines.append(f"  {n}\n      {fmt(new[n])}")
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.stdout.write(text if not a.out else "\n".join(lines[:2 + len(missing) + 3 * len(differ)]) + "\n")
    return 1 if (missing or differ or not old) else 0


if __name__ == "__main__":
    sys.exit(main())
