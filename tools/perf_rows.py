"""Bandwidth of the row-wise operators (online_softmax; later the norms) vs the HBM roofline.  Dev tool: one JSON line
per shape.  usage: python tools/perf_rows.py [softmax] [norms] [add_norms [--shape=emb,n,dtype ...]] [glu [--shape=rows,n,dtype,layout ...]] [xent [--shape=rows,n,ld,dtype ...] [--crossover]] [qknr [--shape=B,L,QH,KH,D,dtype ...]] [--cpu]
add_norms: the residual add fused into the norms against the two-call sequence it replaces, one JSON line per operator,
direction and shape (profiles/add_norm/perf.jsonl is this mode's output).
glu: the gated MLP activations against the torch sequence they replace (profiles/glu/perf.jsonl).
xent: the cross-entropy loss against F.cross_entropy and its autograd backward (profiles/xent/perf.jsonl).
qknr: the fused QK-norm + RoPE against the three-call sequence it replaces (profiles/qknr/perf.jsonl)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
HBM_PEAK = 8000.0   # GB/s, MI355X_MICROARCH.md
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
DEV = "cuda:0"


def timeit(fn, iters=30):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def line(op, shape, dt, us, nbytes, **kw):
    d = dict(op=op, shape=shape, dtype=dt, us=round(us, 2), bytes=nbytes, gbps=round(nbytes / us / 1e3, 1),
             frac_hbm=round(nbytes / us / 1e3 / HBM_PEAK, 3))
    d.update(kw)
    print(json.dumps(d), flush=True)


def softmax():
    softmax_bytes = pkg.workmodel.softmax_bytes
    for N, batch, dt in [(1024, 1024, "f32"), (4096, 16384, "f32"), (4096, 16384, "bf16"), (512, 262144, "bf16"),
                         (16384, 8192, "bf16"), (32768, 4096, "bf16"), (131072, 1024, "f32"), (4100, 16384, "f32")]:
        x = torch.randn(batch, N, device=DEV).to(DT[dt])
        y = torch.empty_like(x)
        us = timeit(lambda: pkg.online_softmax_into(y, x))
        us_t = timeit(lambda: torch.softmax(x, -1))
        line("online_softmax", f"N{N} batch{batch}", dt, us, softmax_bytes(N, batch, x.element_size()), us_torch=round(us_t, 2))
        dy = torch.randn_like(y)
        us = timeit(lambda: pkg.grad_online_softmax(dy, y))
        line("grad_online_softmax", f"N{N} batch{batch}", dt, us, softmax_bytes(N, batch, x.element_size(), bwd=True))
    if "--cpu" in sys.argv:
        from oracle.naive_softmax import naive_softmax
        xs = np.random.default_rng(0).standard_normal((4096, 4096)).astype(np.float32)
        t = []
        for _ in range(5):
            t0 = time.perf_counter(); naive_softmax(xs, dtype=np.float32); t.append(time.perf_counter() - t0)
        print(json.dumps(dict(op="online_softmax", cpu_baseline_gbps=round(softmax_bytes(4096, 4096, 4) / np.median(t) / 1e9, 2),
                              kind="port", cores=1, sample="N4096 batch4096 f32, median of 5")), flush=True)


NORM_SHAPES = [(1024, 1024, "f32"), (4096, 16384, "bf16"), (4096, 16384, "f32"), (8192, 8192, "bf16"),
               (768, 65536, "bf16"), (16384, 4096, "bf16"), (5120, 16384, "bf16")]


def norms():
    norm_bytes = pkg.workmodel.norm_bytes
    for emb, n, dt in NORM_SHAPES:
        x = torch.randn(n, emb, device=DEV).to(DT[dt])
        dy = torch.randn(n, emb, device=DEV).to(DT[dt])
        w = torch.randn(emb, device=DEV); b = torch.randn(emb, device=DEV)
        shape = f"emb{emb} n{n}"
        nb_f, nb_b = norm_bytes(emb, n, x.element_size()), norm_bytes(emb, n, x.element_size(), bwd=True)
        us = timeit(lambda: pkg._rms_norm(x, w))
        us_t = timeit(lambda: torch.nn.functional.rms_norm(x, (emb,), w.to(x.dtype)))
        line("rms_norm", shape, dt, us, nb_f, us_torch=round(us_t, 2))
        y, rms = pkg._rms_norm(x, w)
        line("grad_rms_norm", shape, dt, timeit(lambda: pkg.grad_rms_norm(dy, rms, x, w)), nb_b)
        us = timeit(lambda: pkg._layer_norm(x, w, b))
        us_t = timeit(lambda: torch.nn.functional.layer_norm(x, (emb,), w.to(x.dtype), b.to(x.dtype)))
        line("layer_norm", shape, dt, us, nb_f, us_torch=round(us_t, 2))
        y, mu, sg = pkg._layer_norm(x, w, b)
        line("grad_layer_norm", shape, dt, timeit(lambda: pkg.grad_layer_norm(dy, mu, sg, x, w, b)), nb_b)
    if "--cpu" in sys.argv:
        from oracle.naive_norms import naive_layer_norm, naive_rms_norm
        xs = np.random.default_rng(0).standard_normal((4096, 4096)).astype(np.float32)
        ws = np.ones(4096, np.float32)
        for name, fn in (("rms_norm", lambda: naive_rms_norm(xs, ws, dtype=np.float32)),
                         ("layer_norm", lambda: naive_layer_norm(xs, ws, ws, dtype=np.float32))):
            t = []
            for _ in range(5):
                t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
            print(json.dumps(dict(op=name, cpu_baseline_gbps=round(norm_bytes(4096, 4096, 4) / np.median(t) / 1e9, 2),
                                  kind="port", cores=1, sample="emb4096 n4096 f32, median of 5")), flush=True)


def _register_rows(emb, itemsize, bwd):
    """does a row of emb elements take the register kernels (csrc/row_common.hpp: dispatch_row_shape / _narrow)?"""
    if emb * itemsize % 16:
        return False
    chunks = emb * itemsize // 16
    return chunks <= (1024 * (4 if itemsize == 4 else 2) if bwd else 1024 * 16)


def add_norms():
    """Per operator and direction: the fused call, the two-call sequence it replaces (forward: torch.add into a preallocated h, then
    the plain norm; backward: the plain pullback, then torch.add of dh into dx) and the plain operator alone, each the median of 5
    repeats of timeit() with the min-max spread.  gate: fused median below the sequence's median by more than the sequence's own
    spread -- judged where the rows take the register kernels and x is at least 64 MiB, null elsewhere.  A missed gate ends the
    run with a non-zero status after every line is printed."""
    norm_bytes, add_norm_bytes = pkg.workmodel.norm_bytes, pkg.workmodel.add_norm_bytes

    def med(fn):
        t = sorted(timeit(fn) for _ in range(5))
        return t[2], t[0], t[-1]

    # --shape emb,n,dtype (repeatable): measure these shapes instead of the list
    extra = [a.split("=", 1)[1].split(",") for a in sys.argv[1:] if a.startswith("--shape=")]
    shapes = [(int(e), int(n), dt) for e, n, dt in extra] or NORM_SHAPES
    failed = []
    for emb, n, dt in shapes:
        x = torch.randn(n, emb, device=DEV).to(DT[dt])
        r, dy, dh = (torch.randn(n, emb, device=DEV).to(DT[dt]) for _ in range(3))
        w = torch.randn(emb, device=DEV); b = torch.randn(emb, device=DEV)
        h = torch.empty_like(x)
        isz = x.element_size()
        big = x.numel() * isz >= 64 * 2 ** 20
        _, _, rms = pkg._add_rms_norm(x, r, w, h_out=h)
        _, _, mu, sg = pkg._add_layer_norm(x, r, w, b, h_out=h)

        def seq_rms_fwd():
            torch.add(x, r, out=h)
            return pkg._rms_norm(h, w)

        def seq_ln_fwd():
            torch.add(x, r, out=h)
            return pkg._layer_norm(h, w, b)

        def seq_rms_bwd():
            dx, dw = pkg.grad_rms_norm(dy, rms, h, w)
            return torch.add(dx, dh, out=dx), dw

        def seq_ln_bwd():
            dx, dw, db = pkg.grad_layer_norm(dy, mu, sg, h, w, b)
            return torch.add(dx, dh, out=dx), dw, db

        cases = [("add_rms_norm", False, lambda: pkg._add_rms_norm(x, r, w, h_out=h), seq_rms_fwd, lambda: pkg._rms_norm(h, w)),
                 ("grad_add_rms_norm", True, lambda: pkg.grad_add_rms_norm(dy, dh, rms, h, w), seq_rms_bwd,
                  lambda: pkg.grad_rms_norm(dy, rms, h, w)),
                 ("add_layer_norm", False, lambda: pkg._add_layer_norm(x, r, w, b, h_out=h), seq_ln_fwd,
                  lambda: pkg._layer_norm(h, w, b)),
                 ("grad_add_layer_norm", True, lambda: pkg.grad_add_layer_norm(dy, dh, mu, sg, h, w, b), seq_ln_bwd,
                  lambda: pkg.grad_layer_norm(dy, mu, sg, h, w, b))]
        for op, bwd, fused, seq, plain in cases:
            f, s, p = med(fused), med(seq), med(plain)
            nb, nbp = add_norm_bytes(emb, n, isz, bwd=bwd), norm_bytes(emb, n, isz, bwd=bwd)
            judged = big and _register_rows(emb, isz, bwd)
            line(op, f"emb{emb} n{n}", dt, f[0], nb, us_min=round(f[1], 2), us_max=round(f[2], 2),
                 seq_us=round(s[0], 2), seq_min=round(s[1], 2), seq_max=round(s[2], 2), ratio=round(f[0] / s[0], 3),
                 plain_us=round(p[0], 2), plain_gbps=round(nbp / p[0] / 1e3, 1),
                 gate=(bool(f[0] < s[0] - (s[2] - s[1])) if judged else None))
            if judged and not f[0] < s[0] - (s[2] - s[1]):
                failed.append(f"{op} emb{emb} n{n} {dt}")
    if failed:
        sys.exit("gate missed: " + "; ".join(failed))


GLU_SHAPES = [(8192, 14336, "bf16", "split"), (4096, 28672, "bf16", "split"), (32768, 2880, "bf16", "interleaved"),
              (8192, 14336, "f32", "split"), (1024, 1024, "bf16", "split"), (8192, 14336, "bf16", "halves")]


def _glu_torch(g, u, act, alpha=1.702, limit=7.0):
    """the torch sequence a model runs without the fused call"""
    F = torch.nn.functional
    if act == "silu":
        return F.silu(g) * u
    if act == "gelu_tanh":
        return F.gelu(g, approximate="tanh") * u
    if act == "gelu_erf":
        return F.gelu(g, approximate="none") * u
    g = g.clamp(min=None, max=limit)                 # gpt-oss
    u = u.clamp(min=-limit, max=limit)
    glu = g * torch.sigmoid(g * alpha)
    return (u + 1) * glu


def glu():
    """Gated activations against the torch sequence they replace: per shape, activation and direction the fused call and the
    sequence (forward: the formula; backward: autograd of it, graph kept, backward alone timed), alternating in one process,
    5 repeats of timeit() each: median with the min-max spread, algorithmic GB/s from workmodel.glu_bytes, ratio of the medians.
    Interleaved shapes: the sequence reads gu[:, 0::2] and gu[:, 1::2]; "halves": both sides read gu.chunk(2, -1) (ld = 2n).  --out=FILE (default profiles/glu/perf.jsonl) also gets
    the lines; --tag=NAME labels them (a library variant under NNOP_LIB_PATH).  A large shape (>= 64 MiB per array) where the
    fused call is slower than the sequence ends the run with a non-zero status after every line is printed."""
    glu_bytes = pkg.workmodel.glu_bytes
    out = ([a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")] or [os.path.join(ROOT, "profiles", "glu", "perf.jsonl")])[0]
    tag = ([a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--tag=")] or [None])[0]
    extra = [a.split("=", 1)[1].split(",") for a in sys.argv[1:] if a.startswith("--shape=")]
    shapes = [(int(r), int(n), dt, lay) for r, n, dt, lay in extra] or GLU_SHAPES
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    failed, lines = [], []
    for rows, n, dt, layout in shapes:
        il = layout == "interleaved"
        isz = torch.empty(0, dtype=DT[dt]).element_size()
        big = rows * n * isz >= 64 * 2 ** 20
        if il:
            gu = (3 * torch.randn(rows, 2 * n, device=DEV)).to(DT[dt])
            g, u = gu[:, 0::2], gu[:, 1::2]
        elif layout == "halves":                         # split addressing with ld = 2n: the chunk views of one projection
            gu = (3 * torch.randn(rows, 2 * n, device=DEV)).to(DT[dt])
            g, u = gu.chunk(2, -1)
        else:
            g, u = ((3 * torch.randn(rows, n, device=DEV)).to(DT[dt]) for _ in range(2))
        dy = torch.randn(rows, n, device=DEV).to(DT[dt])
        y = torch.empty_like(dy)
        for act in ("silu", "gelu_tanh", "gelu_erf", "swiglu_oai"):
            if il:
                dgu = torch.empty_like(gu)
                fused_f = lambda: pkg.glu_packed(gu, act=act, layout="interleaved")
                fused_b = lambda: pkg.grad_glu_packed(dy, gu, act=act, layout="interleaved", dgu_out=dgu)
                leaf = gu.clone().requires_grad_(True)
                yt = _glu_torch(leaf[:, 0::2], leaf[:, 1::2], act)
                seq_b = lambda: torch.autograd.grad(yt, (leaf,), dy, retain_graph=True)
            else:
                if layout == "halves":
                    dg, du = torch.empty_like(gu).chunk(2, -1)
                    leaf = gu.clone().requires_grad_(True)
                    yt = _glu_torch(*leaf.chunk(2, -1), act)
                    seq_b = lambda: torch.autograd.grad(yt, (leaf,), dy, retain_graph=True)
                else:
                    dg, du = torch.empty_like(g), torch.empty_like(u)
                    lg, lu = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
                    yt = _glu_torch(lg, lu, act)
                    seq_b = lambda: torch.autograd.grad(yt, (lg, lu), dy, retain_graph=True)
                fused_f = lambda: pkg.glu_into(y, g, u, act=act)
                fused_b = lambda: pkg.grad_glu_into(dg, du, dy, g, u, act=act)
            seq_f = lambda: _glu_torch(g, u, act)
            for op, bwd, fused, seq in ((f"glu[{act}]", False, fused_f, seq_f), (f"grad_glu[{act}]", True, fused_b, seq_b)):
                tf, ts = [], []
                for _ in range(5):                       # alternate: fused, sequence, fused, ...
                    tf.append(timeit(fused))
                    ts.append(timeit(seq))
                tf.sort(); ts.sort()
                nb = glu_bytes(n, rows, isz, bwd=bwd)
                d = dict(op=op, shape=f"rows{rows} n{n}", layout=layout, dtype=dt, us=round(tf[2], 2), us_min=round(tf[0], 2),
                         us_max=round(tf[4], 2), bytes=nb, tbps=round(nb / tf[2] / 1e6, 3), seq_us=round(ts[2], 2),
                         seq_min=round(ts[0], 2), seq_max=round(ts[4], 2), ratio=round(tf[2] / ts[2], 3),
                         gate=(bool(tf[2] <= ts[2]) if big else None))
                if tag:
                    d["tag"] = tag
                print(json.dumps(d), flush=True)
                lines.append(json.dumps(d))
                if big and not tf[2] <= ts[2]:
                    failed.append(f"{op} rows{rows} n{n} {dt}")
            del yt
        with open(out, "w") as f:                        # rewritten after every shape: a run that is cut short keeps what it has
            f.write("\n".join(lines) + "\n")
    if failed:
        sys.exit("fused slower than the torch sequence: " + "; ".join(failed))


XENT_SHAPES = [(8192, 32000, None), (8192, 50257, 50304), (8192, 128256, None), (4096, 201088, None), (4096, 262144, None)]
XENT_OPTS = {"plain": {}, "cap+z+smooth": dict(label_smoothing=0.1, z_loss=1e-4, softcap=30.0)}


def _xent_torch(x, t, label_smoothing=0.0, z_loss=0.0, softcap=0.0):
    """the loss as a trainer writes it, in the dtype of the logits: what the fused call replaces"""
    z = softcap * torch.tanh(x / softcap) if softcap else x
    loss = torch.nn.functional.cross_entropy(z, t, label_smoothing=label_smoothing)
    if z_loss:
        loss = loss + z_loss * (torch.logsumexp(z, -1) ** 2).mean()
    return loss


def xent():
    """Cross-entropy against the torch calls it replaces, in the same process and dtype: per shape, option set and direction the fused
    call (forward: cross_entropy with the mean reduction; backward: grad_cross_entropy into a preallocated gradient) and torch
    (forward: F.cross_entropy, behind c tanh(x / c) where capped and with the z-loss term where asked; backward: autograd of it, graph
    kept, backward alone timed), alternating, 5 repeats of timeit() each: median with the min-max spread, algorithmic TB/s from
    workmodel.xent_bytes, ratio of the medians.  --out=FILE (default profiles/xent/perf.jsonl), --tag=NAME, --shape=rows,n,ld,dtype.
    A shape of 64 MiB or more where the fused call is not faster than torch with the spreads apart ends the run with a non-zero status
    after every line is printed.
    --crossover: instead, the fused calls alone over row lengths around the launch rule's crossover (bf16 and fp32, 256 MiB of logits
    each), for a library variant under NNOP_LIB_PATH that forces one form; default output profiles/xent/perf_crossover.jsonl."""
    xent_bytes = pkg.workmodel.xent_bytes
    sweep = "--crossover" in sys.argv
    default = os.path.join(ROOT, "profiles", "xent", "perf_crossover.jsonl" if sweep else "perf.jsonl")
    out = ([a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")] or [default])[0]
    tag = ([a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--tag=")] or [None])[0]
    extra = [a.split("=", 1)[1].split(",") for a in sys.argv[1:] if a.startswith("--shape=")]
    if extra:
        shapes = [(int(r), int(n), int(ld), dt) for r, n, ld, dt in extra]
    elif sweep:
        shapes = [(2 ** 27 // n, n, n, dt) for dt in ("bf16", "f32") for n in (256, 512, 1024, 2048, 4096, 8192, 16384, 32768)]
    else:
        shapes = [(r, n, ld or n, dt) for dt in ("bf16", "f32") for r, n, ld in XENT_SHAPES] + [(1048576, 1000, 1000, "bf16")]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    failed, lines = [], ([l for l in open(out).read().splitlines() if l] if sweep and os.path.exists(out) else [])
    for rows, n, ld, dt in shapes:
        isz = torch.empty(0, dtype=DT[dt]).element_size()
        big = rows * n * isz >= 64 * 2 ** 20
        buf = torch.empty(rows, ld, device=DEV, dtype=DT[dt])
        for r0 in range(0, rows, 65536):                     # filled in slabs: no fp32 copy of the whole matrix
            buf[r0:r0 + 65536] = (4 * torch.randn(min(65536, rows - r0), ld, device=DEV)).to(DT[dt])
        x = buf[:, :n]
        t = torch.randint(0, n, (rows,), device=DEV)
        gr = torch.full((rows,), 1.0 / rows, device=DEV)
        dx = torch.empty(rows, n, device=DEV, dtype=DT[dt])
        for name, opts in XENT_OPTS.items():
            _, lse = pkg._cross_entropy(x, t, **opts)
            fused_f = lambda: pkg.cross_entropy(x, t, **opts)
            fused_b = lambda: pkg.grad_cross_entropy(gr, lse, x, t, out=dx, **opts)
            if not sweep:
                leaf = x.detach().clone().requires_grad_(True)
                lt = _xent_torch(leaf, t, **opts)
                seq_f = lambda: _xent_torch(x, t, **opts)
                seq_b = lambda: torch.autograd.grad(lt, (leaf,), retain_graph=True)
            for op, bwd, fused, seq in (("cross_entropy", False, fused_f, None if sweep else seq_f),
                                        ("grad_cross_entropy", True, fused_b, None if sweep else seq_b)):
                tf, ts = [], []
                for _ in range(5):                           # alternate: fused, torch, fused, ...
                    tf.append(timeit(fused, iters=10))
                    ts.append(timeit(seq, iters=10) if seq else 0.0)
                tf.sort(); ts.sort()
                nb = xent_bytes(n, rows, isz, index_bytes=8, bwd=bwd)
                d = dict(op=op, opts=name, shape=f"rows{rows} n{n} ld{ld}", dtype=dt, us=round(tf[2], 2), us_min=round(tf[0], 2),
                         us_max=round(tf[4], 2), bytes=nb, tbps=round(nb / tf[2] / 1e6, 3))
                if not sweep:
                    ok = bool(tf[4] < ts[0])                 # faster, and the spreads do not overlap
                    d.update(torch_us=round(ts[2], 2), torch_min=round(ts[0], 2), torch_max=round(ts[4], 2), ratio=round(tf[2] / ts[2], 3),
                             gate=(ok if big else None))
                    if big and not ok:
                        failed.append(f"{op}[{name}] rows{rows} n{n} {dt}")
                if tag:
                    d["tag"] = tag
                print(json.dumps(d), flush=True)
                lines.append(json.dumps(d))
            if not sweep:
                del lt, leaf
        with open(out, "w") as f:                            # rewritten after every shape: a run that is cut short keeps what it has
            f.write("\n".join(lines) + "\n")
        del buf, x, dx
    if failed:
        sys.exit("fused not faster than torch: " + "; ".join(failed))


QKNR_SHAPES = [(4, 4096, 32, 8, 128, "bf16"), (1, 32768, 32, 8, 128, "bf16"), (4, 4096, 8, 4, 256, "bf16")]
QKNR_BAR = 0.75     # fused <= 0.75 x the sequence: midway between the byte ratio (0.5 forward, 0.6 pullback) and parity


def qknr():
    """Fused QK-norm + RoPE against the three calls it replaces, in the same process: forward _qk_norm_rope against _rms_norm on q,
    _rms_norm on k and _llama_rope; pullback grad_qk_norm_rope against grad_llama_rope, grad_rms_norm on q and grad_rms_norm on k (with
    the rms the sequence's forward saved).  Alternating, 5 repeats of timeit() each: median with the min-max spread, algorithmic TB/s
    from workmodel.qknr_bytes, ratio of the medians, gate = ratio <= QKNR_BAR.  --out=FILE (default profiles/qknr/perf.jsonl),
    --shape=B,L,QH,KH,D,dtype.  A missed gate ends the run with a non-zero status after every line is printed."""
    import ctypes as C
    qknr_bytes = pkg.workmodel.qknr_bytes
    out = ([a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")] or [os.path.join(ROOT, "profiles", "qknr", "perf.jsonl")])[0]
    extra = [a.split("=", 1)[1].split(",") for a in sys.argv[1:] if a.startswith("--shape=")]
    shapes = [(int(b), int(l), int(qh), int(kh), int(d), dt) for b, l, qh, kh, d, dt in extra] or QKNR_SHAPES
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    failed, lines = [], []
    for B, L, QH, KH, D, dt in shapes:
        q, dq2 = (torch.randn(B, QH, L, D, device=DEV).to(DT[dt]) for _ in range(2))
        k, dk2 = (torch.randn(B, KH, L, D, device=DEV).to(DT[dt]) for _ in range(2))
        wq, wk = torch.randn(D, device=DEV), torch.randn(D, device=DEV)
        cos, sin = pkg.LlamaRotaryEmbedding(D, device=DEV)(torch.arange(L, device=DEV, dtype=torch.float32).expand(B, L))
        isz = q.element_size()
        _, rms_q = pkg._rms_norm(q.view(-1, D), wq)
        _, rms_k = pkg._rms_norm(k.view(-1, D), wk)
        n_parts = pkg._lib_ext.load().nnop_qk_norm_rope_bwd_workspace_bytes(C.byref(pkg.qknorm._desc(q, k, wq, cos, 1e-6, 0.0))) // (8 * D)

        def seq_f():
            nq, _ = pkg._rms_norm(q.view(-1, D), wq)
            nk, _ = pkg._rms_norm(k.view(-1, D), wk)
            return pkg._llama_rope(nq.view_as(q), nk.view_as(k), cos, sin, bwd=False)

        def seq_b():
            dnq, dnk = pkg.grad_llama_rope((dq2, dk2), cos, sin)
            return pkg.grad_rms_norm(dnq.view(-1, D), rms_q, q.view(-1, D), wq) + pkg.grad_rms_norm(dnk.view(-1, D), rms_k, k.view(-1, D), wk)

        fused_f = lambda: pkg._qk_norm_rope(q, k, wq, wk, cos, sin)
        fused_b = lambda: pkg.grad_qk_norm_rope((dq2, dk2), q, k, wq, wk, cos, sin)
        for op, bwd, fused, seq in (("qk_norm_rope", False, fused_f, seq_f), ("grad_qk_norm_rope", True, fused_b, seq_b)):
            tf, ts = [], []
            for _ in range(5):                               # alternate: fused, sequence, fused, ...
                tf.append(timeit(fused))
                ts.append(timeit(seq))
            tf.sort(); ts.sort()
            nb = qknr_bytes(D, L, QH, KH, B, isz, bwd=bwd, n_parts=n_parts if bwd else 0)
            ratio = tf[2] / ts[2]
            d = dict(op=op, shape=f"B{B} L{L} QH{QH} KH{KH} D{D}", dtype=dt, us=round(tf[2], 2), us_min=round(tf[0], 2), us_max=round(tf[4], 2),
                     bytes=nb, tbps=round(nb / tf[2] / 1e6, 3), seq_us=round(ts[2], 2), seq_min=round(ts[0], 2), seq_max=round(ts[4], 2),
                     ratio=round(ratio, 3), gate=bool(ratio <= QKNR_BAR))
            print(json.dumps(d), flush=True)
            lines.append(json.dumps(d))
            if not ratio <= QKNR_BAR:
                failed.append(f"{op} {d['shape']} {dt}: {ratio:.3f}")
        with open(out, "w") as f:                            # rewritten after every shape: a run that is cut short keeps what it has
            f.write("\n".join(lines) + "\n")
        del q, k, dq2, dk2
    if failed:
        sys.exit(f"fused above {QKNR_BAR} x the three-call sequence: " + "; ".join(failed))


if __name__ == "__main__":
    which =[a for a in sys.argv[1:] if not a.startswith("--")] or ["softmax"]
    for w in which:
        globals()[w]()
