"""Logit soft-capping at a realistic cap (c = 30 on scores of std 8), capped AND uncapped, per dtype, against the fp64 reference.

    python tools/measure_softcap_realistic.py > profiles/r05/softcap_realistic.txt

The inputs are those of tests/test_softcap_gpu.test_realistic_cap_on_sharp_scores (tests/softcap_cases.realistic_inputs) in fp32, bf16
and fp16; the gates are those of tests/util.assert_close with the scales tests/attn_ref.check_parity uses.  Per tensor: the worst
error / tolerance (> 1 misses the gate) and the number of elements outside.  This is the evidence for keeping that test to fp32:
in bf16 the `ls` gate is missed by the uncapped call as by the capped one."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge
from attn_ref import attention_fwd, attention_grads, inputs
from util import ATOL_FRAC, RTOL, ABS_FLOOR, GRAD_SCALE

pkg = ge.load_package()
dev = torch.device("cuda:0")
np64 = lambda t: t.detach().double().cpu().numpy()


def ratio(g, ref, dt, scale, kind="fwd"):
    if kind == "grad" and scale == 1.0:
        scale = GRAD_SCALE[dt]
    g = np64(g)
    mag = np.abs(ref).max()
    tol = scale * (ATOL_FRAC[dt] * mag + RTOL[dt] * np.abs(ref)) + ABS_FLOOR[dt]
    err = np.abs(g - ref)
    return float((err / tol).max()), int((err > tol).sum()), err.size, float(err.max()), float(mag)


cases = [(dt, E, 130, 517, 30.0) for dt in ("f32", "bf16") for E in (64, 128)] + [("f16", 64, 130, 517, 30.0)]
for case in cases:
    dt, E, QL, KL, cap = case
    d = inputs(("real",) + tuple(case), 1, 2, 1, QL, KL, E, dt, dev, qscale=8.0)
    q, k, v, do = d["q"], d["k"], d["v"], d["do"]
    for c in (cap, None):
        o, ms, ls = pkg._flash_attention(q, k, v, causal=False, softcap=c)
        dq, dk, dv = pkg.grad_flash_attention(do, o, ms, ls, q, k, v, causal=False, softcap=c)[:3]
        torch.cuda.synchronize()
        a = (np64(q), np64(k), np64(v))
        fr = attention_fwd(*a, causal=False, softcap=c)
        gr = attention_grads(*a, np64(do), causal=False, softcap=c)
        sc = 1.0 if dt == "f32" else 2.0
        rows = [("o", o, fr[0], 1.0, "fwd"), ("ms", ms, fr[1], 1.0, "fwd"), ("ls", ls, fr[2], 2.0, "fwd"),
                ("dq", dq, gr[0], sc, "grad"), ("dk", dk, gr[1], sc, "grad"), ("dv", dv, gr[2], sc, "grad")]
        for name, g, r, s, kind in rows:
            wr, nbad, n, emax, mag = ratio(g, r, dt, s, kind)
            print(f"{dt} E{E} cap={c} {name}: worst err/tol {wr:.3f}  bad {nbad}/{n}  max err {emax:.3e}  max|ref| {mag:.3e}", flush=True)
        # the (ms, ls) pair together: log-sum-exp = ms + log(ls), which is what the backward reads
        lse, lse_ref = np64(ms) + np.log(np64(ls)), fr[1] + np.log(fr[2])
        print(f"{dt} E{E} cap={c} ms+log(ls): max err {np.abs(lse - lse_ref).max():.3e}; max |ms - ms_ref| {np.abs(np64(ms) - fr[1]).max():.3e}; "
              f"max |ls/ls_ref - 1| {np.abs(np64(ls) / fr[2] - 1).max():.3e}", flush=True)
