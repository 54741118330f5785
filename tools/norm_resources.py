"""Register table of the norm kernels, fused (residual add) next to plain: compiles csrc/rms_norm.hip and csrc/layer_norm.hip for
gfx950 with the compiler's kernel resource report and prints one markdown row per kernel shape (VGPRs / scratch bytes per lane /
waves per SIMD).  Exits 1 if a fused instantiation has scratch where its plain twin has none.  Needs hipcc, no GPU.

usage: python tools/norm_resources.py [--all]        (default: T/W = f32/f32, bf16/bf16, bf16/f32; --all: every dtype pair)"""
import collections
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nnop.jl_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c"]
TY = {"f": "f32", "DF16_": "f16", "DF16b": "bf16"}
NAME = re.compile(r"_ZN4nnop\d+(norm_[a-z_]+_kernel)I((?:f|DF16_|DF16b)+)((?:Li\d+E)*)((?:Lb[01]E)+)")
FIELD = re.compile(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)")


def report(unit, tmp):
    out = subprocess.run(["hipcc", *FLAGS, unit + ".hip", "-o", os.path.join(tmp, unit + ".o")], cwd=CSRC, capture_output=True, text=True)
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
    return rows


def main():
    with tempfile.TemporaryDirectory() as tmp:
        rows = {**report("rms_norm", tmp), **report("layer_norm", tmp)}
    table = collections.defaultdict(dict)                       # (kernel, T/W, shape) -> {(ln, fused): resources}
    for name, r in rows.items():
        m = NAME.match(name)
        if not m:
            if "norm_" in name and "_kernel" in name:     # (the fold, row_common.hpp fold_partial_rows_kernel, has no "norm_" in its name)
                sys.exit(f"cannot parse the kernel name {name}: extend NAME before trusting the table")
            continue
        tys = "/".join(TY[t] for t in re.findall(r"f|DF16_|DF16b", m.group(2)))
        shape = "×".join(re.findall(r"Li(\d+)E", m.group(3))) or "any"
        flags = re.findall(r"Lb([01])E", m.group(4))             # LN, ADD (absent on older builds), ...
        table[(m.group(1), tys, shape)][(flags[0] == "1", len(flags) > 1 and flags[1] == "1")] = r
    keep = None if "--all" in sys.argv else {"f32/f32", "bf16/bf16", "bf16/f32"}
    fmt = lambda r: "–" if r is None else f"{r['VGPRs']} / {r['ScratchSize']} / {r['Occupancy']}"
    print("| kernel | T/W | G×C | RMS plain | RMS fused | LN plain | LN fused |\n|---|---|---|---|---|---|---|")
    bad = 0
    order = lambda k: (k[0], k[1], [int(v) for v in k[2].split("×")] if k[2] != "any" else [0])
    for key in sorted(table, key=order):
        c = table[key]
        for ln in (False, True):
            p, f = c.get((ln, False)), c.get((ln, True))
            if p and f and p["ScratchSize"] == 0 and f["ScratchSize"] != 0:
                bad += 1
                print(f"<!-- scratch only in the fused variant: {key} LN={ln} -->")
        if keep is None or key[1] in keep:
            print(f"| `{key[0]}` | {key[1]} | {key[2]} | " + " | ".join(fmt(c.get(k)) for k in ((False, False), (False, True), (True, False), (True, True))) + " |")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
