"""Worst error / gate ratios of the expert linear layers' GPU tests -> profiles/moe_linear/parity.json.
usage: NNOP_TEST_ERRLOG=log.jsonl python -m pytest tests/test_zzzzzzz_moe_linear_gpu.py -m gpu; python tools/moe_linear_parity.py log.jsonl [out.json]
Every comparison of tests/test_zzzzzzz_moe_linear_gpu.py logs |got - ref| / tolerance (util.record_error, kind "moe_linear"); this keeps,
per case (grid, across-layouts, micro-batches-..., clamped, gpt-oss...), output (ys-<layout>-<bias>, dxs-<layout>, dw-<layout>-<grad type>[-acc],
db-<grad type>[-acc], and the layer's stages) and dtype, the worst one, and whether dw of the [E, K, N] layout was the transpose of the
other layout's bit for bit.  The exact-data, isolation and reproducibility tests compare bit for bit and log nothing."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("ys", "dxs", "dw", "db")


def main(log, out):
    worst, bitwise, n = {}, [], 0
    for line in open(log):
        r = json.loads(line)
        if r.get("kind") != "moe_linear":
            continue
        if "bitwise" in r:
            bitwise.append(bool(r["bitwise"]))
            continue
        n += 1
        key = (r["case"], r["name"], r["dt"])
        if key not in worst or r["worst_ratio"] > worst[key]:
            worst[key] = round(r["worst_ratio"], 5)
    res = dict(comparisons=n, dw_kn_is_dw_nk_transposed_bitwise=f"{sum(bitwise)} of {len(bitwise)}",
               worst={f"{case}/{g}/{dt}": v for (case, g, dt), v in sorted(worst.items())})
    for g in OUTPUTS:
        res[f"worst_{g}"] = max(v for (_, name, _), v in worst.items() if name.split("-")[0] == g)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for k, v in res["worst"].items():
        print(f"{k}: {v}")
    print(json.dumps({k: v for k, v in res.items() if k != "worst"}))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "moe_linear", "parity.json"))
