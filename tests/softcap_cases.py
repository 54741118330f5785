"""The inputs and case lists of tests/test_softcap_gpu.py (test infrastructure, not a test file).  They live apart from the test so
that the CPU tests (tests/test_softcap_host.py) can check on the very same inputs that the cap changes the result by much more than
the parity tolerance, and so that tools/measure_softcap_realistic.py measures what the test runs."""
from attn_ref import inputs

DTYPES = ["f32", "bf16", "f16"]
EMBS = [16, 32, 64, 128, 256, 8]                 # 8: the plain-HIP kernels
CAPS = [0.5, 1.0, 2.0]
LENS = [(63, 65), (65, 63), (517, 517), (1, 63), (300, 1100)]


def parity_grid():
    """every E meets every dtype and both causal settings; caps and lengths cycle over the grid (as test_window_gpu._grid prunes).
    Cases: (dt, E, causal, QL, KL, cap)."""
    out = []
    i = 0
    for E in EMBS:
        for dt in DTYPES:
            for causal in (False, True):
                QL, KL = LENS[(i + EMBS.index(E)) % len(LENS)]
                if E >= 128 and QL * KL > 600 * 600:
                    QL, KL = (QL // 2 + 1, KL // 2 + 1)          # the window grid's rule (none of LENS is that large today)
                out.append((dt, E, causal, QL, KL, CAPS[i % len(CAPS)]))
                i += 1
    return out


def grid_inputs(case, dev):
    dt, E, causal, QL, KL, cap = case
    return inputs(case, 1, 2, 1, QL, KL, E, dt, dev)


# realistic cap: scores of std 8 (q x 8) under c = 30.  fp32 only: at row maxima of 25 .. 40 a bf16 ms is rounded by up to 0.0625
# (0.125 past 32) and ls is stored relative to the ROUNDED ms, so ls alone is up to 6.6 % (13 %) off the exact row's while
# ms + log(ls) is right to 6e-3.  Measured on an MI355X on these very inputs, the unchanged ls gate is missed by the capped call
# (err / tol 1.37 at E = 64, 1.35 at E = 128) and equally by the uncapped one (1.21, 1.29); o, ms, dq, dk, dv are inside their
# gates (err / tol <= 0.24) either way (tools/measure_softcap_realistic.py, profiles/r05/softcap_realistic.txt).  It is the
# residual format, not the cap: DESIGN.md section 4.4d.
REALISTIC = [("f32", E, 130, 517, 30.0) for E in (64, 128)]


def realistic_inputs(case, dev):
    dt, E, QL, KL, cap = case
    return inputs(("real",) + case, 1, 2, 1, QL, KL, E, dt, dev, qscale=8.0)
