"""Worst error / gate ratios of the MoE permute / combine GPU tests -> profiles/moe_data/parity.json.
usage: NNOP_TEST_ERRLOG=log.jsonl python -m pytest tests/test_zzzz_moe_data_gpu.py -m gpu; python tools/moe_data_parity.py log.jsonl [out.json]
Every comparison of tests/test_zzzz_moe_data_gpu.py logs |got - ref| / tolerance (util.record_error, kind "moe_data"); this keeps, per
output (xs, y, dx, dys, dw) and dtype of the rows, the worst one and the case it came from.  xs is compared exactly: its ratio is 0 or inf."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("xs", "y", "dx", "dys", "dw")


def main(log, out):
    worst, n = {}, 0
    for line in open(log):
        r = json.loads(line)
        if r.get("kind") != "moe_data":
            continue
        n += 1
        key = (r["name"], r["dt"])
        if key not in worst or r["worst_ratio"] > worst[key]["ratio"]:
            worst[key] = dict(ratio=round(r["worst_ratio"], 5), case=r["case"])
    res = dict(comparisons=n, worst={f"{g}/{dt}": v for (g, dt), v in sorted(worst.items())})
    for g in OUTPUTS:
        res[f"worst_{g}"] = max(v["ratio"] for (name, _), v in worst.items() if name == g)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "moe_data", "parity.json"))
