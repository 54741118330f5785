"""Worst error / gate ratios of the grouped expert GEMM's GPU tests -> profiles/moe_gemm/parity.json.
usage: NNOP_TEST_ERRLOG=log.jsonl python -m pytest tests/test_zzzzz_moe_gemm_gpu.py -m gpu; python tools/moe_gemm_parity.py log.jsonl [out.json]
Every comparison of tests/test_zzzzz_moe_gemm_gpu.py logs |got - ref| / tolerance (util.record_error, kind "moe_gemm"); this keeps, per
case (grid, plan, clamped, layer-...), output (ys, dxs, dw, and the layer's stages) and dtype, the worst one.  The exact-data, isolation and
reproducibility tests compare bit for bit and log nothing."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("ys", "dxs", "dw")


def main(log, out):
    worst, n = {}, 0
    for line in open(log):
        r = json.loads(line)
        if r.get("kind") != "moe_gemm":
            continue
        n += 1
        key = (r["case"], r["name"], r["dt"])
        if key not in worst or r["worst_ratio"] > worst[key]:
            worst[key] = round(r["worst_ratio"], 5)
    res = dict(comparisons=n, worst={f"{case}/{g}/{dt}": v for (case, g, dt), v in sorted(worst.items())})
    for g in OUTPUTS:
        res[f"worst_{g}"] = max(v for (_, name, _), v in worst.items() if name == g)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for k, v in res["worst"].items():
        print(f"{k}: {v}")
    print(json.dumps({k: v for k, v in res.items() if k != "worst"}))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "moe_gemm", "parity.json"))
