"""Worst error / gate ratios of the mixture-of-experts GPU tests -> profiles/moe/parity.json.
usage: NNOP_TEST_ERRLOG=log.jsonl python -m pytest tests/test_zzz_moe_gpu.py -m gpu; python tools/moe_parity.py log.jsonl [out.json]
Every comparison of tests/test_zzz_moe_gpu.py logs |got - ref| / tolerance (util.record_error); this keeps, per tensor (w, lse, dlogits)
and dtype of the logits, the worst one and the case it came from.  idx and the plan are compared exactly and have no ratio."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(log, out):
    worst, n = {}, 0
    for line in open(log):
        r = json.loads(line)
        if r.get("kind") != "moe":
            continue
        n += 1
        key = (r["name"], r["dt"])
        if key not in worst or r["worst_ratio"] > worst[key]["ratio"]:
            worst[key] = dict(ratio=round(r["worst_ratio"], 5), case=r["case"])
    res = dict(comparisons=n, worst={f"{g}/{dt}": v for (g, dt), v in sorted(worst.items())})
    for g in ("w", "lse", "dlogits"):
        res[f"worst_{g}"] = max(v["ratio"] for (name, _), v in worst.items() if name == g)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "moe", "parity.json"))
