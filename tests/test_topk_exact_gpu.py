"""Bit-exact tests of the top-k select, decode / code-gradient and sparse weight-gradient kernels
(``ops/csrc/topk.hip``) against the fp64 / integer-key references of ``topk_exact_cases.py``.

Every comparison is ``torch.equal``.  Outputs are prefilled with NaN / -1 (zeros where the contract
asks for zero-initialised buffers), so an unwritten or misplaced element cannot pass.  One select
test id is one row length, i.e. one kernel instantiation or one of its edges.
"""

import pytest
import torch

import topk_exact_cases as X

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_coding__amd.ops import _lib as L

    L.lib()  # must load: no silent fallback on a GPU box
    yield


def _T():
    from sparse_coding__amd.ops import topk

    return topk


def _same(out, ref, what):
    """``out`` holds exactly the reference, rounded once to the output type."""
    want = (ref.float() if ref.dtype == torch.float64 else ref).to(out.dtype).to(out.device)
    if not torch.equal(out, want):
        bad = out != want
        if out.is_floating_point():
            bad |= out.isnan()
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} values differ, first at {i}: "
                             f"{out[tuple(i)].item()} vs {want[tuple(i)].item()}")


def _k(ks):
    return torch.tensor(list(ks), device=DEV, dtype=torch.int32)


def _dev(t):
    return {k: v.to(DEV) if isinstance(v, torch.Tensor) else v for k, v in t.items()}


# ------------------------------------------------------------------ select
def _select(c, absolute=False, relu=True, x=None, D=None):
    G, B, _ = c["scores"].shape
    idx = torch.full((G, B, c["kmax"]), -1, device=DEV, dtype=torch.int32)
    val = torch.full((G, B, c["kmax"]), NAN, device=DEV)
    _T().topk_select(c["scores"].to(DEV), _k(c["ks"]), c["kmax"], absolute=absolute, relu=relu, out=(idx, val),
                     x=None if x is None else x.to(DEV), D=None if D is None else D.to(DEV))
    return idx, val


def _check_launches(c, what, x=None, D=None):
    """The contract on one case: plain, repeated (bit-identical), and by |score| without ReLU."""
    idx, val = _select(c, x=x, D=D)
    tags = X.check_select(c["scores"], c["ks"], c["kmax"], idx, val, x=x, D=D, what=what)
    idx2, val2 = _select(c, x=x, D=D)
    assert torch.equal(idx2, idx) and torch.equal(val2, val), what + ": a second call differs"
    ia, va = _select(c, absolute=True, relu=False, x=x, D=D)
    X.check_select(c["scores"], c["ks"], c["kmax"], ia, va, absolute=True, relu=False, x=x, D=D, what=what + " absolute")
    return tags


@pytest.mark.parametrize("n", X.F32_N)
def test_select_fp32(n):
    kind, P = X.dispatch(False, n)
    _check_launches(X.select_case(n, False), f"{kind}<{P}>")


@pytest.mark.parametrize("n", X.BF16_N)
def test_select_bf16(n):
    kind, P = X.dispatch(True, n)
    c = X.select_case(n, True)
    x, D = X.select_operands(n, 4, per_model=X.BF16_N.index(n) % 2 == 1)
    _check_launches(c, f"{kind}<{P}> with x, D", x, D)
    idx, val = _select(c)  # without the operands: every tie by its path's documented order
    X.check_select(c["scores"], c["ks"], c["kmax"], idx, val, what=f"{kind}<{P}>")


@pytest.mark.parametrize("n,d", X.RESOLVE_EXTRA)
def test_select_bf16_exact_resolve(n, d):
    c = X.select_case(n, True)
    for per_model in (False, True):
        x, D = X.select_operands(n, d, per_model)
        tags = _check_launches(c, f"bf16 n={n} d={d} per-model x={per_model}", x, D)
        assert {"resolve"} in tags


def test_select_refusals():
    from sparse_coding__amd.ops._lib import KernelError

    for bf, ns in X.REFUSED_N.items():
        for n in ns:
            scores = torch.zeros(1, 2, n, device=DEV, dtype=BF if bf else F32)
            with pytest.raises(KernelError):
                _T().topk_select(scores, _k([1]), 4)


@pytest.mark.parametrize("n,bf", X.OVER_KMAX_N)
def test_select_clamps_k_to_kmax(n, bf):
    """k[g] > kmax on the last model: its rows hold a top-kmax, the other rows and the elements behind
    the last row are intact (the buffers are carved from larger ones, so even an unclamped write
    stays inside the allocation)."""
    c = X.over_kmax_case(n, bf)
    G, B, _ = c["scores"].shape
    rows = G * B * c["kmax"]
    big_i = torch.full((rows + n + 64,), -7, device=DEV, dtype=torch.int32)
    big_v = torch.full((rows + n + 64,), -7.0, device=DEV)
    idx, val = big_i[:rows].view(G, B, -1), big_v[:rows].view(G, B, -1)
    _T().topk_select(c["scores"].to(DEV), _k(c["ks"]), c["kmax"], out=(idx, val))
    assert max(c["ks"]) == c["kmax"] + 5
    X.check_select(c["scores"], c["ks"], c["kmax"], idx, val, what=f"k > kmax, {X.dispatch(bf, n)}")
    assert bool((big_i[rows:] == -7).all()) and bool((big_v[rows:] == -7.0).all()), "written past the last row"


def test_select_bf16_many_ties_order():
    """n = 4096 (a thread owns columns of two chunks), 200 equal keys over the chunk boundary just
    below 100 larger ones, k = 150, no operands: the 50 ties taken are the lowest columns."""
    c = X.tie_order_case(True)
    idx, val = _select(c)
    lo, hi = c["ties"]
    pick = idx.cpu().long().sort(-1).values
    for g in range(X.SEL_G):
        for b in range(X.SEL_B):
            tied = pick[g, b][(pick[g, b] >= lo) & (pick[g, b] < hi)]
            want = torch.arange(lo, lo + 50) if X.BF16_BRACKET_TIES == "column" else torch.arange(2048, 2098)
            assert torch.equal(tied, want), f"row ({g}, {b}): ties taken {tied.tolist()}"
    X.check_select(c["scores"], c["ks"], c["kmax"], idx, val, what="bf16 tie order")


def test_select_block_bracket_ties_are_thread_major():
    """The fp32 block kernel's bracket documents thread-major ties: n = 8192, ties in 1000..1199."""
    c = X.tie_order_case(False)
    idx, val = _select(c)
    pick = idx.cpu().long().sort(-1).values
    for g in range(X.SEL_G):
        for b in range(X.SEL_B):
            tied = pick[g, b][(pick[g, b] >= 1000) & (pick[g, b] < 1200)]
            assert torch.equal(tied, torch.arange(1024, 1074)), f"row ({g}, {b}): ties taken {tied.tolist()}"
    X.check_select(c["scores"], c["ks"], c["kmax"], idx, val, what="block tie order")


# ------------------------------------------------------------------ decode and code gradient
def _decode(t, codebuf, dscbuf, dscv, prev_idx=None, dense_from=0):
    G, B, _ = t["idx"].shape
    d = t["D"].shape[2]
    r = torch.full((G, B, d), NAN, device=DEV, dtype=BF)
    se = torch.full((G, B), NAN, device=DEV)
    _T().decode_grad(t["idx"], t["val"], _k(t["ks"]), t["D"], t["x"], r, se, codebuf, dscbuf, dscv=dscv, prev_idx=prev_idx,
                     dense_from=dense_from)
    return r, se


def _dense_buffers(t):
    G, B, _ = t["idx"].shape
    n = t["D"].shape[1]
    return torch.zeros(G, B, n, device=DEV, dtype=BF), torch.zeros(G, B, n, device=DEV, dtype=BF)


@pytest.mark.parametrize("case", X.DECODE_CASES, ids=lambda c: f"d{c[0]}")
def test_decode_grad(case):
    d, ks, kmax, per_model, dense_from = case
    cpu = X.decode_inputs(3, X.DEC_B, X.DEC_N, d, ks, kmax, per_model)
    ref = X.decode_ref(cpu, dense_from)
    X.check_decode(cpu, ref, f"d={d}")
    t = _dev(cpu)
    what = f"d={d} NV={X.decode_nv(d)} k={ks} kmax={kmax} per-model x={per_model} dense_from={dense_from}"
    cb, db = _dense_buffers(t)
    dscv = torch.where(ref["live"], NAN, 0.0).float().to(DEV)  # (slots >= k are never written)
    r, se = _decode(t, cb, db, dscv, dense_from=dense_from)
    _same(r, ref["R"], what + " R")
    _same(se, ref["row_se"], what + " row_se")
    _same(dscv, ref["dscv"], what + " dscv")
    _same(cb, ref["code"], what + " codebuf")
    _same(db, ref["dsc"], what + " dscbuf")
    # forward only: without the code buffer nothing but R and row_se is written
    db2, dscv2 = torch.full_like(db, 7.0), torch.full_like(dscv, 7.0)
    r, se = _decode(t, None, db2, dscv2)
    _same(r, ref["R"], what + " forward-only R")
    _same(se, ref["row_se"], what + " forward-only row_se")
    assert bool((db2 == 7.0).all()) and bool((dscv2 == 7.0).all()), what + ": forward-only wrote a gradient buffer"


def test_decode_grad_refusals():
    from sparse_coding__amd.ops._lib import KernelError

    for d in X.DECODE_REFUSED_D:
        t = _dev(X.decode_inputs(1, 2, 8, d, (2,), 2, False))
        with pytest.raises(KernelError):
            _decode(t, None, None, None)


def test_decode_grad_clears_previous_picks():
    """Step B with ``prev_idx`` = step A's picks on the same dense buffers leaves a fresh scatter of B
    alone: overlapping columns, column 0 both a real pick and the index of the padded slots."""
    d, ks, kmax, per_model, _ = X.DECODE_CASES[3]
    a = X.decode_inputs(3, X.DEC_B, X.DEC_N, d, ks, kmax, per_model, seed=1)
    b = X.decode_inputs(3, X.DEC_B, X.DEC_N, d, ks, kmax, per_model, seed=2)
    ra, rb = X.decode_ref(a), X.decode_ref(b)
    ta, tb = _dev(a), _dev(b)
    cb, db = _dense_buffers(ta)
    _decode(ta, cb, db, None)
    _same(cb, ra["code"], "step A codebuf")
    _same(db, ra["dsc"], "step A dscbuf")
    r, se = _decode(tb, cb, db, None, prev_idx=ta["idx"])
    _same(r, rb["R"], "step B R")
    _same(cb, rb["code"], "step B codebuf")
    _same(db, rb["dsc"], "step B dscbuf")


# ------------------------------------------------------------------ sparse weight gradient
@pytest.mark.parametrize("d", X.WGRAD_D)
def test_sparse_wgrad(d):
    from sparse_coding__amd.ops import gemm as GM

    T = _T()
    for twin in (False, True):
        cpu = X.wgrad_inputs(d, dense_twin=twin)
        t = _dev(cpu)
        lists = T.SlotLists(X.WG_G, X.WG_B, X.WG_N, X.WG_KS, X.WG_KMAX, DEV)
        T.slot_lists(t["idx"], _k(X.WG_KS), lists)
        for alpha in X.WGRAD_ALPHAS:
            ref = X.wgrad_ref(cpu, alpha)
            what = f"d={d} alpha={alpha} dense twin={twin}"
            outs = {}
            for dtype in (F32, BF):
                outs[dtype] = torch.full((X.WG_G, X.WG_N, d), NAN, device=DEV, dtype=dtype)
                T.sparse_wgrad(lists, t["val"], t["dscv"], t["R"], t["x"], outs[dtype], alpha)
                _same(outs[dtype], ref, f"{what} {dtype}")
            if twin:  # the dense GEMM over the scattered buffers computes the same sums
                dense = torch.full((X.WG_G, X.WG_N, d), NAN, device=DEV)
                GM.weight_grads([[(t["code"], t["R"]), (t["dsc"], t["x"])]], [dense], alpha)
                _same(dense, ref, what + " dense weight_grads")
                assert torch.equal(dense, outs[F32])


def test_sparse_wgrad_refusals():
    from sparse_coding__amd.ops._lib import KernelError

    T = _T()
    G, B, n, kmax = 1, 4, 8, 2
    idx = torch.zeros(G, B, kmax, device=DEV, dtype=torch.int32)
    lists = T.SlotLists(G, B, n, (0,), kmax, DEV)
    T.slot_lists(idx, _k([0]), lists)
    for d in X.WGRAD_REFUSED_D:
        z = lambda *s, dt=F32: torch.zeros(*s, device=DEV, dtype=dt)
        with pytest.raises(KernelError):
            T.sparse_wgrad(lists, z(G, B, kmax), z(G, B, kmax), z(G, B, d, dt=BF), z(B, d, dt=BF), z(G, n, d), 1.0)
