"""Worst error / gate ratios of the fused QK-norm + RoPE GPU tests -> profiles/qknr/parity.json.
usage: NNOP_TEST_ERRLOG=log.jsonl python -m pytest tests/test_zz_qknr_gpu.py -m gpu; python tools/qknr_parity.py log.jsonl [out.json]
Every comparison of tests/test_zz_qknr_gpu.py logs |got - ref| / tolerance (util.record_error); this keeps, per gate and dtype, the
worst one and the case it came from.  Gates: "out" = q_out, k_out, dq, dk (TOL of tests/test_rope_gpu.py); "dw" = dwq, dwk."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(log, out):
    worst, n = {}, 0
    for line in open(log):
        r = json.loads(line)
        if r.get("kind") != "qknr":
            continue
        n += 1
        key = ("dw" if r["name"] in ("dwq", "dwk") else "out", r["dt"])
        if key not in worst or r["worst_ratio"] > worst[key]["ratio"]:
            worst[key] = dict(ratio=round(r["worst_ratio"], 5), case=r["case"], tensor=r["name"])
    res = dict(comparisons=n, worst={f"{g}/{dt}": v for (g, dt), v in sorted(worst.items())},
               worst_out=max(v["ratio"] for (g, _), v in worst.items() if g == "out"),
               worst_dw=max(v["ratio"] for (g, _), v in worst.items() if g == "dw"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "qknr", "parity.json"))
