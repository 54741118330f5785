"""CPU tests of the cross-entropy loss (include/nnop_hip.h, nnop_cross_entropy / nnop_cross_entropy_bwd): the two entry points are
declared, bound and exported; they validate descriptor, pointers and alignment in that order and return before any launch; the Python
wrappers raise before any device work and hand views over by stride; the reference the GPU tests are judged against (tests/xent_ref.py)
agrees with autograd of torch's own cross_entropy, with finite differences and with its closed-form gradient; and the gates tell a
result rounded once from one that is 4 ulp off.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import itertools
import math
import re

import pytest
import torch

import xent_ref as ref
from abi_util import HEADER, SHIM, strip_c_comments

NEW = ("nnop_cross_entropy", "nnop_cross_entropy_bwd")
OK = C.c_void_p(0x7f0000001000)              # never dereferenced: every call in this file returns before a launch
NULL = C.c_void_p(0)
INF, NAN = float("inf"), float("nan")


def test_exports(pkg):
    header = strip_c_comments(open(HEADER).read())
    declared = set(re.findall(r"\b(nnop_[a-z_]+)\s*\(", header))
    lib = pkg._lib.load()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/nnop_hip.h"
        assert name in pkg._lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert len(lib.nnop_cross_entropy.argtypes) == 6 and len(lib.nnop_cross_entropy_bwd.argtypes) == 7
    assert lib.nnop_abi_version() == 7 and pkg._lib.ABI_VERSION == 7
    assert C.sizeof(pkg._lib.XentDesc) == 72
    assert len(pkg._lib.EXPORTED_SYMBOLS) == 30
    for name in ("cross_entropy", "_cross_entropy", "grad_cross_entropy"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))


def _desc(pkg, **kw):
    base = dict(dtype=2, index_bytes=8, rows=64, n=1000, ld=1024, ld_grad=1024, ignore_index=-100, index_base=0, reserved=0,
                label_smoothing=0.0, z_loss=0.0, softcap=0.0, reserved_f=0.0)
    base.update(kw)
    return pkg._lib.XentDesc(**base)


def _both(lib, d, p=OK):
    return [lib.nnop_cross_entropy(C.byref(d), p, p, p, p, None), lib.nnop_cross_entropy_bwd(C.byref(d), p, p, p, p, p, None)]


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=9), "NNOP_ERR_DTYPE"),
    (dict(dtype=-1), "NNOP_ERR_DTYPE"),
    (dict(index_bytes=2), "NNOP_ERR_OPTS"),
    (dict(index_bytes=0), "NNOP_ERR_OPTS"),
    (dict(index_base=2), "NNOP_ERR_OPTS"),
    (dict(index_base=-1), "NNOP_ERR_OPTS"),
    (dict(reserved=1), "NNOP_ERR_OPTS"),
    (dict(reserved_f=1.0), "NNOP_ERR_OPTS"),
    (dict(reserved_f=NAN), "NNOP_ERR_OPTS"),
    (dict(label_smoothing=-0.1), "NNOP_ERR_OPTS"),
    (dict(label_smoothing=1.5), "NNOP_ERR_OPTS"),
    (dict(label_smoothing=NAN), "NNOP_ERR_OPTS"),
    (dict(z_loss=-1e-4), "NNOP_ERR_OPTS"),
    (dict(z_loss=INF), "NNOP_ERR_OPTS"),
    (dict(z_loss=NAN), "NNOP_ERR_OPTS"),
    (dict(softcap=-30.0), "NNOP_ERR_OPTS"),
    (dict(softcap=INF), "NNOP_ERR_OPTS"),
    (dict(softcap=NAN), "NNOP_ERR_OPTS"),
    (dict(rows=0), "NNOP_ERR_SHAPE"),
    (dict(rows=-3), "NNOP_ERR_SHAPE"),
    (dict(n=0), "NNOP_ERR_SHAPE"),
    (dict(ld=999), "NNOP_ERR_SHAPE"),
    (dict(n=2 ** 31, ld=2 ** 31, ld_grad=2 ** 31), "NNOP_ERR_SHAPE"),
    (dict(rows=2 ** 31), "NNOP_ERR_SHAPE"),
    # the order: dtype before options before shape, all before the pointers
    (dict(dtype=9, index_bytes=3, rows=0), "NNOP_ERR_DTYPE"),
    (dict(index_bytes=3, rows=0), "NNOP_ERR_OPTS"),
    (dict(softcap=NAN, n=0), "NNOP_ERR_OPTS"),
])
def test_descriptor_validation(pkg, kw, status):
    d = _desc(pkg, **kw)
    want = getattr(pkg._lib, status)
    lib = pkg._lib.load()
    assert _both(lib, d) == [want] * 2
    assert _both(lib, d, NULL) == [want] * 2             # the descriptor is judged before the pointers


def test_ld_grad_is_read_by_the_pullback_only(pkg):
    lib, L = pkg._lib.load(), pkg._lib
    d = _desc(pkg, ld_grad=999)
    assert _both(lib, d, NULL) == [L.NNOP_ERR_NULL, L.NNOP_ERR_SHAPE]
    for ok in (dict(label_smoothing=0.0), dict(label_smoothing=1.0), dict(z_loss=1e-4, softcap=30.0, index_base=1, index_bytes=4),
               dict(rows=2 ** 31 - 1), dict(n=2 ** 31 - 1, ld=2 ** 31 - 1, ld_grad=2 ** 31 - 1), dict(ignore_index=5)):
        assert _both(lib, _desc(pkg, **ok), NULL) == [L.NNOP_ERR_NULL] * 2, ok     # the descriptor passed
    assert lib.nnop_cross_entropy(None, OK, OK, OK, OK, None) == L.NNOP_ERR_NULL
    assert lib.nnop_cross_entropy_bwd(None, OK, OK, OK, OK, OK, None) == L.NNOP_ERR_NULL


def test_null_and_alignment_checks_come_before_any_launch(pkg):
    lib, L = pkg._lib.load(), pkg._lib
    at = lambda off: C.c_void_p(0x7f0000001000 + off)
    # (entry point, number of pointers, {position: alignment}) -- fwd: loss, lse, logits, targets; bwd: dlogits, dloss, lse, logits, targets
    for dtype, es in ((2, 2), (1, 2), (0, 4)):
        for ib in (4, 8):
            d = _desc(pkg, dtype=dtype, index_bytes=ib)
            for fn, aligns in ((lib.nnop_cross_entropy, [4, 4, es, ib]), (lib.nnop_cross_entropy_bwd, [es, 4, 4, es, ib])):
                args = [OK] * len(aligns)
                for pos, a in enumerate(aligns):
                    b = list(args)
                    b[pos] = NULL
                    assert fn(C.byref(d), *b, None) == L.NNOP_ERR_NULL, (fn.__name__, pos)
                    c = [at(1)] * len(aligns)                    # NULL is judged before alignment
                    c[pos] = NULL
                    assert fn(C.byref(d), *c, None) == L.NNOP_ERR_NULL
                    c = list(args)
                    c[pos] = at(a // 2)                          # aligned to half of what is needed
                    assert fn(C.byref(d), *c, None) == L.NNOP_ERR_ALIGN, (fn.__name__, pos, a)
    for st in (L.NNOP_ERR_OPTS, L.NNOP_ERR_ALIGN):
        assert "cross_entropy" in L.strerror(st)


class OnGpu(torch.Tensor):
    """a CPU tensor that claims to be on the GPU reaches the host checks, which run in front of any device work"""
    is_cuda = True


def test_python_checks_raise_before_device_work(pkg):
    x, t = torch.ones(4, 32), torch.zeros(4, dtype=torch.int64)
    f32 = torch.ones(4)
    for call in (lambda: pkg.cross_entropy(x, t), lambda: pkg._cross_entropy(x, t), lambda: pkg.grad_cross_entropy(f32, f32, x, t),
                 lambda: pkg.cross_entropy(x.clone().requires_grad_(True), t)):
        with pytest.raises(pkg.NNopError, match="GPU-only"):
            call()
    mk = lambda *s, dt=torch.float32: torch.ones(*s, dtype=dt).as_subclass(OnGpu)
    xg, tg = mk(4, 32), mk(4, dt=torch.int64)
    for bad_x, bad_t in ((mk(4, 32, dt=torch.float64), tg), (torch.ones(()).as_subclass(OnGpu), tg), ([1.0], tg), (xg, mk(4)),
                         (xg, mk(4, dt=torch.int16)), (xg, mk(5, dt=torch.int64)), (xg, mk(4, 1, dt=torch.int64)), (xg, [0, 1, 2, 3])):
        for call in (lambda: pkg.cross_entropy(bad_x, bad_t), lambda: pkg._cross_entropy(bad_x, bad_t),
                     lambda: pkg.grad_cross_entropy(mk(4), mk(4), bad_x, bad_t)):
            with pytest.raises(TypeError):
                call()
    with pytest.raises(pkg.NNopError, match="reduction"):
        pkg.cross_entropy(xg, tg, reduction="batchmean")
    with pytest.raises(pkg.NNopError, match="non-empty"):
        pkg.cross_entropy(mk(0, 32), mk(0, dt=torch.int64))
    with pytest.raises(TypeError, match="dloss_rows"):
        pkg.grad_cross_entropy(mk(5), mk(4), xg, tg)
    with pytest.raises(TypeError, match="lse"):
        pkg.grad_cross_entropy(mk(4), mk(4, dt=torch.float16), xg, tg)
    with pytest.raises(TypeError, match="out"):
        pkg.grad_cross_entropy(mk(4), mk(4), xg, tg, out=mk(4, 31))
    with pytest.raises(TypeError, match="out"):
        pkg.grad_cross_entropy(mk(4), mk(4), xg, tg, out=mk(32, 4).t())


def test_views_map_to_rows_and_stride_without_a_copy(pkg):
    rows = pkg.losses._as_rows
    x = torch.zeros(3, 7, 50)
    assert rows(x)[1:] == (21, 50, 50) and rows(x)[0] is x
    padded = torch.zeros(21, 64)
    v = padded[:, :50]
    assert rows(v)[1:] == (21, 50, 64) and rows(v)[0] is v
    v3 = padded.view(3, 7, 64)[..., :50]
    assert rows(v3)[1:] == (21, 50, 64) and rows(v3)[0] is v3
    one = padded[2, :50]
    assert rows(one)[1:] == (1, 50, 50) and rows(one)[0] is one
    tr = torch.zeros(50, 21).t()                             # no row stride expresses it: copied
    got = rows(tr)
    assert got[1:] == (21, 50, 50) and got[0] is not tr and got[0].is_contiguous()
    part = torch.zeros(3, 7, 64)[:, :5, :50]
    assert rows(part)[1:] == (15, 50, 50) and rows(part)[0].is_contiguous()
    d = pkg.losses._desc(torch.zeros(2, dtype=torch.bfloat16), 21, 50, 64, 50, torch.zeros(2, dtype=torch.int32), -100, 0.1, 1e-4, 30.0)
    assert (d.dtype, d.index_bytes, d.rows, d.n, d.ld, d.ld_grad, d.ignore_index, d.index_base) == (2, 4, 21, 50, 64, 50, -100, 0)
    assert (d.reserved, d.reserved_f) == (0, 0.0) and abs(d.label_smoothing - 0.1) < 1e-8 and d.softcap == 30.0


def test_workmodel_bytes(pkg):
    wb = pkg.workmodel.xent_bytes
    assert wb(128256, 8192, 2) == 8192 * 128256 * 2 + 8 * 8192 + 8 * 8192
    assert wb(128256, 8192, 2, bwd=True) == 2 * 8192 * 128256 * 2 + 8 * 8192 + 8 * 8192
    assert wb(1000, 1048576, 2, index_bytes=4) == 1048576 * (2000 + 8 + 4)
    assert wb(1, 1, 4, index_bytes=4, bwd=True) == 8 + 8 + 4


# ---- the reference ----------------------------------------------------------------------------------------------------
OPTS = [dict(eps=e, zeta=z, cap=c) for e, z, c in itertools.product((0.0, 0.1), (0.0, 1e-4), (0.0, 30.0))] + [dict(eps=1.0, zeta=0.01, cap=2.0)]


def _inputs(rows, n, seed, scale=4.0):
    gen = torch.Generator().manual_seed(seed)
    x = scale * torch.randn(rows, n, generator=gen, dtype=torch.float64)
    t = torch.randint(0, n, (rows,), generator=gen)
    g = torch.randn(rows, generator=gen, dtype=torch.float64)
    return x, t, g


@pytest.mark.parametrize("opts", OPTS, ids=lambda o: "eps%g-zeta%g-cap%g" % (o["eps"], o["zeta"], o["cap"]))
@pytest.mark.parametrize("ignore", [None, -100, 3])
def test_reference_matches_autograd_of_torch_cross_entropy(opts, ignore):
    x, t, g = _inputs(9, 23, 0, scale=12.0 if opts["cap"] else 4.0)
    ii = -100 if ignore is None else ignore
    if ignore is not None:
        t[1] = t[4] = ii
    if ignore == 3:
        t[t == 3] = 3                                            # every row whose target is class 3 is ignored
    xd = x.clone().requires_grad_(True)
    loss = ref.textbook(xd, t, ignore_index=ii, **opts)
    loss.backward(g)
    r = ref.xent_ref(x, t, ignore_index=ii, **opts)
    torch.testing.assert_close(r["loss"], loss.detach(), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(ref.xent_grad_ref(g, x, t, ignore_index=ii, **opts), xd.grad, rtol=1e-12, atol=1e-14)
    if ignore is not None:
        assert (r["loss"][[1, 4]] == 0).all() and (xd.grad[[1, 4]] == 0).all()
    # index_base = 1: the same rows with every stored target one higher (and the same stored ignore_index)
    t1 = torch.where(t == ii, t, t + 1)
    if ignore != 3:                                              # (with ignore_index 3, a stored 3 that means class 2 would be ignored)
        r1 = ref.xent_ref(x, t1, ignore_index=ii, index_base=1, **opts)
        assert torch.equal(r1["loss"], r["loss"])
        assert torch.equal(ref.xent_grad_ref(g, x, t1, ignore_index=ii, index_base=1, **opts), ref.xent_grad_ref(g, x, t, ignore_index=ii, **opts))


@pytest.mark.parametrize("opts", OPTS, ids=lambda o: "eps%g-zeta%g-cap%g" % (o["eps"], o["zeta"], o["cap"]))
def test_reference_gradient_matches_finite_differences(opts):
    x, t, g = _inputs(4, 9, 1, scale=6.0 if opts["cap"] else 2.0)
    t[2] = -100
    dx = ref.xent_grad_ref(g, x, t, **opts)
    h = 1e-6
    fd = torch.zeros_like(x)
    for j in range(x.shape[1]):
        e = torch.zeros_like(x)
        e[:, j] = h
        fd[:, j] = (ref.xent_ref(x + e, t, **opts)["loss"] - ref.xent_ref(x - e, t, **opts)["loss"]) / (2 * h) * g
    assert (fd - dx).abs().max() < 1e-8 * max(1.0, float(dx.abs().max()))
    assert (dx[2] == 0).all()


def test_reference_special_rows():
    x, t, g = _inputs(6, 11, 2)
    t[1], t[3] = 11, -5                                          # invalid: neither ignore_index nor a class
    t[4] = -100
    x[5, :] = -INF
    x[0, 2] = -INF
    t[0] = 2
    r = ref.xent_ref(x, t)
    dx = ref.xent_grad_ref(g, x, t)
    assert torch.isnan(r["loss"][[1, 3, 5]]).all() and r["loss"][4] == 0 and r["loss"][0] == INF
    assert torch.isnan(dx[[1, 3, 5]]).all() and (dx[4] == 0).all() and torch.isfinite(dx[[0, 2]]).all()
    assert dx[0, 2] == -g[0]                                     # p = 0 at a -inf logit; the target's -g stays
    assert torch.isfinite(r["lse"][:5]).all()


# ---- the gates ----------------------------------------------------------------------------------------------------------
def _off_by_ulps(v, k):
    """v (a 16-bit tensor) moved k units in the last place, away from zero"""
    bits = v.view(torch.int16).to(torch.int32)
    return (bits + k).to(torch.int16).view(v.dtype)


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_gates_tell_one_rounding_from_four_ulp(dt):
    x, t, g = _inputs(37, 1000, 3)
    x = x.to(ref.DT[dt])
    opts = dict(eps=0.1, zeta=1e-4, cap=30.0)
    r = ref.xent_ref(x, t, **opts)
    dx = ref.xent_grad_ref(g, x, t, **opts)
    once = dx.to(ref.DT[dt])
    assert ref.grad_ratio(once, dx, g, r["lse"], opts["zeta"], dt) <= 1.0
    if dt == "f32":
        # r = 1e-5 is 84 ulp of fp32 (the project's softmax-pullback rtol): 4 ulp stays inside it; twice r does not
        assert ref.grad_ratio(once * (1 + 4 * 2.0 ** -23), dx, g, r["lse"], opts["zeta"], dt) <= 1.0
        assert ref.grad_ratio(once.double() * (1 + 2e-5) + 1e-5, dx, g, r["lse"], opts["zeta"], dt) > 1.0
    else:
        assert ref.grad_ratio(_off_by_ulps(once, 4), dx, g, r["lse"], opts["zeta"], dt) > 1.0
    # loss and lse are fp32 whatever T is: rounded once passes, 4e-6 of the magnitude twice over fails
    for key in ("loss", "lse"):
        assert ref.loss_ratio(r[key].float(), r[key], r["lse"], r["z"]) <= 1.0
        assert ref.loss_ratio(r[key] + 8.1e-6 * 30, r[key], r["lse"], r["z"]) > 1.0
    # a NaN or an infinity in the wrong place fails whatever the magnitudes
    bad = r["loss"].clone()
    bad[3] = math.nan
    assert ref.loss_ratio(bad, r["loss"], r["lse"], r["z"]) == math.inf
    bad = once.clone()
    bad[3, 5] = math.inf
    assert ref.grad_ratio(bad, dx, g, r["lse"], opts["zeta"], dt) == math.inf


# ---- the Julia shim ---------------------------------------------------------------------------------------------------
def test_shim_source_names_the_symbols():
    src = open(SHIM).read()
    for name in NEW:
        assert re.search(r"ccall\(\(:%s\b" % name, src), f"the Julia shim does not ccall {name}"
    assert re.search(r"rrule\(::typeof\(cross_entropy\)", src), "no rrule for cross_entropy in the shim"
    assert re.search(r"export [^\n]*\bcross_entropy\b", src)
    m = re.search(r"struct XentDesc\n(.*?)\nend", src, re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == (
        "dtype::Int32; index_bytes::Int32 rows::Int64; n::Int64 ld::Int64; ld_grad::Int64 ignore_index::Int64 "
        "index_base::Int32; reserved::Int32 label_smoothing::Float32; z_loss::Float32; softcap::Float32; reserved_f::Float32")
