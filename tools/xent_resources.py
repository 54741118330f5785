"""Register table of the cross-entropy kernels: compiles csrc/xent.hip for gfx950 with the compiler's kernel resource report and
prints one markdown row per instantiation (VGPRs / SGPRs / scratch bytes per lane / waves per SIMD / LDS bytes).  Exits 1 if any
kernel has scratch.  Needs hipcc, no GPU.  (The approach of tools/norm_resources.py.)

usage: python tools/xent_resources.py"""
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nnop.jl_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c"]
TY = {"f": "f32", "DF16_": "f16", "DF16b": "bf16"}
NAME = re.compile(r"_ZN4nnop\d+(xent_(?:fwd|bwd)_kernel)I(f|DF16_|DF16b)Li(\d+)ELi(\d+)E((?:Lb[01]E)+)")
FIELD = re.compile(r"remark:\s+(VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run(["hipcc", *FLAGS, "xent.hip", "-o", os.path.join(tmp, "xent.o")], cwd=CSRC, capture_output=True, text=True)
    if out.returncode:
        sys.exit(out.stderr[-2000:])
    rows, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        m = FIELD.search(line)
        if m and cur is not None:
            cur[m.group(1).split()[0]] = int(m.group(2))
    print("| kernel | T | VEC | G | CAP[, SMOOTH] | VGPRs | SGPRs | scratch | waves/SIMD | LDS |\n|---|---|---|---|---|---|---|---|---|---|")
    bad, table = 0, []
    for name, r in rows.items():
        m = NAME.match(name)
        if not m:
            if "xent_" in name and "_kernel" in name:
                sys.exit(f"cannot parse the kernel name {name}: extend NAME before trusting the table")
            continue
        flags = ", ".join(re.findall(r"Lb([01])E", m.group(5)))
        table.append((m.group(1), TY[m.group(2)], int(m.group(3)), int(m.group(4)), flags, r))
        bad += r["ScratchSize"] != 0
    for k, t, vec, g, flags, r in sorted(table, key=lambda e: e[:5]):
        print(f"| `{k}` | {t} | {vec} | {g} | {flags} | {r['VGPRs']} | {r['TotalSGPRs']} | {r['ScratchSize']} | {r['Occupancy']} | {r['LDS']} |")
    if not table:
        sys.exit("no xent kernel in the compiler's report")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
