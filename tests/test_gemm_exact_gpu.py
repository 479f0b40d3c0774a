"""Bit-exact tests of every K-loop instantiation and fused epilogue of the grouped MFMA GEMM.

Inputs are small integers in bf16 and scalars are dyadic (``exact_gemm_cases.py``), so the fp64
result of plain torch ops is the only right answer: every comparison is ``torch.equal``.  Outputs
are prefilled with NaN (zeros where the contract asks for zero-initialised buffers), so an
unwritten or doubly mapped tile cannot pass.  One test id is one instantiation (``cfg``).
"""

import pytest
import torch

import exact_gemm_cases as X

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32
NAN = float("nan")
ALPHAS = {F32: (1.0, 0.5, 2.0), BF: (1.0, 2.0)}  # (bf16 outputs stay integers)
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_coding__amd.ops import _lib as L

    L.lib()  # must load: no silent fallback on a GPU box
    yield
    _CACHE.clear()


def _gemm():
    from sparse_coding__amd.ops import gemm

    return gemm


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _same(out, ref, what):
    """``out`` holds exactly the fp64 reference rounded once to the output type."""
    want = ref.float() if out.dtype == F32 else ref.float().to(out.dtype)
    if not torch.equal(out, want):
        bad = (out != want) | out.isnan()
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} values differ, first at {idx}: "
                             f"{out[tuple(idx)].item()} vs {want[tuple(idx)].item()}")


def _sum_same(part, ref, what):
    """Partial sums (any grid of partials along dim 1) add up to the reference."""
    assert torch.equal(part.double().sum(1), ref), f"{what}: {part.double().sum(1).tolist()} vs {ref.tolist()}"


def _full(shape, dtype, fill=NAN):
    return torch.full(shape, fill, device=DEV, dtype=dtype)


def _i32(v):
    return torch.tensor(list(v), device=DEV, dtype=torch.int32)


# ------------------------------------------------------------------ A. plain epilogues
def _pool(kind):
    return _cached(("pool", kind), lambda: tuple(t.to(DEV, BF) for t in X.plain_pool(kind)))


def _pref(kind, k0, k1):
    """fp64 A B^T over pool columns [k0, k1) at the full pool size (the cases slice it), with the
    input conditions asserted at the largest alpha."""
    def make():
        a, b = _pool(kind)
        return X.check_plain(a[..., k0:k1], b[..., k0:k1], 2.0, F32 if kind == "int" else BF, f"pool {kind} [{k0},{k1})") / 2.0
    return _cached(("pref", kind, k0, k1), make)


def _ops(kind, G, M, N, k0, k1):
    a, b = _pool(kind)
    return a[:G, :M, k0:k1], b[:G, :N, k0:k1]


def _stored(t, kmajor):
    return t.contiguous() if kmajor else t.transpose(-1, -2).contiguous()


def _launch_plain(cfg, layout, dtype, probs, G, M, N, ksplit=1, nact_k=None):
    """One direct launch of the plain epilogue: probs = [(A segments, B segments, alpha)] of logical
    operands [G, rows, K] (or [rows, K], shared by every model)."""
    gemm = _gemm()
    a_ops, b_ops, keep = [], [], []
    for seg_a, seg_b, _ in probs:
        for segs, kmajor, ops in ((seg_a, layout & 1, a_ops), (seg_b, layout & 2, b_ops)):
            st = [_stored(s, kmajor) for s in segs]
            keep += st
            o = [gemm._op(s, s.shape[-1], 0 if s.dim() == 2 else s.shape[-2] * s.shape[-1]) for s in st]
            ops += o if len(o) == 2 else o * 2
    k1 = probs[0][0][0].shape[-1]
    k2 = probs[0][0][1].shape[-1] if len(probs[0][0]) == 2 else 0
    outs = [_full(((ksplit,) if ksplit > 1 else ()) + (G, M, N), dtype) for _ in probs]
    gemm._launch(gemm.EPI_F32 if dtype == F32 else gemm.EPI_BF16, layout, M, N, k1, k2, G, a_ops, b_ops, outs,
                 [p[2] for p in probs], N, M * N, cfg=cfg, ksplit=ksplit, split_stride=G * M * N, nact_k=nact_k)
    return outs


def _front_end(cfg, layout, dtype, a, b, alpha, variant=0):
    """The same product through the public front ends (layout 2 has none)."""
    gemm = _gemm()
    G, M, N = b.shape[0], a.shape[-2], b.shape[-2]
    if layout == 2:
        return _launch_plain(cfg, 2, dtype, [([a], [b], alpha)], G, M, N)[0]
    out = _full((G, M, N), dtype)
    if layout == 0 and variant % 2 == 0:
        gemm.weight_grads([[(_stored(a, False), _stored(b, False))]], [out], alpha, cfg=cfg)
        return out
    with gemm.force_shape(cfg):
        if layout == 3:
            gemm.matmul_nt(a.contiguous(), b.contiguous(), out, alpha)
        elif layout == 1:
            gemm.matmul_nn(a.contiguous(), _stored(b, False), out, alpha)
        else:
            gemm.matmul_tn(_stored(a, False), _stored(b, False), out, alpha)
    return out


def _grid(cfg):
    """The asymmetric 2 x 3 tile grid of three models: 18 blocks (not a multiple of the 8 XCDs)."""
    bm, bn = X.block(cfg)
    return 3, 2 * bm, 3 * bn


@pytest.mark.parametrize("cfg", X.ALL_CFGS)
def test_plain_whole_k(cfg):
    G, M, N = _grid(cfg)
    for i, K in enumerate(X.whole_k_values(cfg)):
        for dtype, layout in X.plain_combos(cfg):
            kind, alpha = X.pool_kind(dtype), ALPHAS[dtype][(i + layout) % len(ALPHAS[dtype])]
            a, b = _ops(kind, G, M, N, 0, K)
            out = _front_end(cfg, layout, dtype, a, b, alpha, variant=i)
            _same(out, alpha * _pref(kind, 0, K)[:G, :M, :N], f"cfg {cfg} K={K} layout {layout} {dtype} alpha {alpha}")


@pytest.mark.parametrize("cfg", X.ALL_CFGS)
def test_plain_single_block(cfg):
    bm, bn = X.block(cfg)
    for i, K in enumerate((64, 64 * (X.ring(cfg)[1] + 1))):
        for dtype, layout in X.plain_combos(cfg):
            kind, alpha = X.pool_kind(dtype), ALPHAS[dtype][i]
            a, b = _ops(kind, 1, bm, bn, 0, K)
            out = _front_end(cfg, layout, dtype, a, b, alpha, variant=i + 1)
            _same(out, alpha * _pref(kind, 0, K)[:1, :bm, :bn], f"cfg {cfg} one block K={K} layout {layout} {dtype}")


def _check_slabs(cfg, slabs, kind, ranges, k_lo, alpha, G, M, N, what):
    """Every slab equals the product over its documented K-tile range, the slabs sum to the whole
    product and none of them is the whole product."""
    bk = X.ring(cfg)[0]
    total = alpha * _pref(kind, k_lo + ranges[0][0] * bk, k_lo + ranges[-1][1] * bk)[:G, :M, :N]
    for ksi, (t0, t1) in enumerate(ranges):
        _same(slabs[ksi], alpha * _pref(kind, k_lo + t0 * bk, k_lo + t1 * bk)[:G, :M, :N], f"{what} slab {ksi} tiles [{t0},{t1})")
        assert not torch.equal(slabs[ksi].double(), total), f"{what}: slab {ksi} holds the whole product"
    assert torch.equal(slabs.double().sum(0), total), f"{what}: the slabs do not sum to the product"


@pytest.mark.parametrize("cfg", X.ALL_CFGS)
def test_plain_split_k(cfg):
    G, M, N = _grid(cfg)
    bk = X.ring(cfg)[0]
    for i, (K, ks) in enumerate(X.SPLITS):
        for dtype, layout in X.plain_combos(cfg):
            kind, alpha = X.pool_kind(dtype), ALPHAS[dtype][i % len(ALPHAS[dtype])]
            a, b = _ops(kind, G, M, N, 0, K)
            slabs = _launch_plain(cfg, layout, dtype, [([a], [b], alpha)], G, M, N, ksplit=ks)[0]
            _check_slabs(cfg, slabs, kind, X.split_ranges(K, bk, ks), 0, alpha, G, M, N,
                         f"cfg {cfg} K={K} ksplit={ks} layout {layout} {dtype}")


@pytest.mark.parametrize("cfg", X.ALL_CFGS)
def test_plain_live_k_ranges(cfg):
    """Per-model live K ranges on the plain epilogue: one, three and seven K-tiles on a BK32 ring."""
    G, M, N = _grid(cfg)
    K, live = X.NACT_K
    for dtype, layout in X.plain_combos(cfg):
        kind = X.pool_kind(dtype)
        a, b = _ops(kind, G, M, N, 0, K)
        a = a.clone()
        for g, s in enumerate(live):
            a[g, :, s:] = 0
        out = _launch_plain(cfg, layout, dtype, [([a], [b], 1.0)], G, M, N, nact_k=_i32(live))[0]
        ref = torch.stack([_pref(kind, 0, s)[g, :M, :N] for g, s in enumerate(live)])
        _same(out, ref, f"cfg {cfg} live K {live} layout {layout} {dtype}")


@pytest.mark.parametrize("cfg", X.ALL_CFGS)
def test_plain_two_segments(cfg):
    G, M, N = _grid(cfg)
    bk = X.ring(cfg)[0]
    gemm = _gemm()
    for i, (K1, K2) in enumerate(X.SEGMENTS):
        for dtype, layout in X.plain_combos(cfg):
            kind, alpha = X.pool_kind(dtype), ALPHAS[dtype][i % len(ALPHAS[dtype])]
            a1, b1 = _ops(kind, G, M, N, 0, K1)
            a2, b2 = _ops(kind, G, M, N, K1, K1 + K2)
            what = f"cfg {cfg} K={K1}+{K2} layout {layout} {dtype}"
            ref = alpha * _pref(kind, 0, K1 + K2)[:G, :M, :N]
            out = _launch_plain(cfg, layout, dtype, [([a1, a2], [b1, b2], alpha)], G, M, N)[0]
            _same(out, ref, what)
            if layout == 0:  # the weight-gradient front end (dense top-k step: two segments)
                out = _full((G, M, N), dtype)
                gemm.weight_grads([[(_stored(a1, False), _stored(b1, False)), (_stored(a2, False), _stored(b2, False))]],
                                  [out], alpha, cfg=cfg)
                _same(out, ref, what + " weight_grads")
            ks = X.straddling_split(K1, K2, bk) or 2
            slabs = _launch_plain(cfg, layout, dtype, [([a1, a2], [b1, b2], alpha)], G, M, N, ksplit=ks)[0]
            _check_slabs(cfg, slabs, kind, X.split_ranges(K1 + K2, bk, ks), 0, alpha, G, M, N, what + f" ksplit={ks}")


@pytest.mark.parametrize("cfg", X.ALL_CFGS)
def test_plain_two_problems(cfg):
    G, M, N = _grid(cfg)
    K = 192
    gemm = _gemm()
    for dtype, layout in X.plain_combos(cfg):
        kind = X.pool_kind(dtype)
        al = (0.5, 2.0) if dtype == F32 else (1.0, 2.0)
        (a0, b0), (a1, b1) = _ops(kind, G, M, N, 0, K), _ops(kind, G, M, N, K, 2 * K)
        refs = [_pref(kind, 0, K)[:G, :M, :N], _pref(kind, K, 2 * K)[:G, :M, :N]]
        outs = _launch_plain(cfg, layout, dtype, [([a0], [b0], al[0]), ([a1], [b1], al[1])], G, M, N)
        for i in range(2):
            _same(outs[i], al[i] * refs[i], f"cfg {cfg} problem {i} layout {layout} {dtype}")
        if layout == 0:
            outs = [_full((G, M, N), dtype) for _ in range(2)]
            gemm.weight_grads([[(_stored(a0, False), _stored(b0, False))], [(_stored(a1, False), _stored(b1, False))]],
                              outs, 2.0, cfg=cfg)
            for i in range(2):
                _same(outs[i], 2.0 * refs[i], f"cfg {cfg} weight_grads problem {i} {dtype}")


@pytest.mark.parametrize("cfg", X.ALL_CFGS)
def test_plain_shared_operand(cfg):
    G, M, N = _grid(cfg)
    K = 192
    gemm = _gemm()
    for dtype, layout in X.plain_combos(cfg):
        if layout not in (0, 3):
            continue
        kind = X.pool_kind(dtype)
        a, b = _ops(kind, G, M, N, 0, K)
        ref = _pref(kind, 0, K)
        # the first model's A with every model's B, every model's A with the first model's B
        ref_a = _cached(("shared_a", kind), lambda: X.check_plain(_pool(kind)[0][:1, :, :K], _pool(kind)[1][..., :K], 1.0, dtype, "shared A"))
        ref_b = _cached(("shared_b", kind), lambda: X.check_plain(_pool(kind)[0][..., :K], _pool(kind)[1][:1, :, :K], 1.0, dtype, "shared B"))
        assert torch.equal(ref_a[0], ref[0]) and not torch.equal(ref_a[1], ref[1])
        what = f"cfg {cfg} layout {layout} {dtype}"
        if layout == 3:
            out = _full((G, M, N), dtype)
            with gemm.force_shape(cfg):
                gemm.matmul_nt(a[0].contiguous(), b.contiguous(), out, 2.0)
            _same(out, 2.0 * ref_a[:G, :M, :N], what + " shared a")
        else:
            out = _full((G, M, N), dtype)
            gemm.weight_grads([[(_stored(a[0], False), _stored(b, False))]], [out], 1.0, cfg=cfg)
            _same(out, ref_a[:G, :M, :N], what + " shared A")
            out = _full((G, M, N), dtype)
            gemm.weight_grads([[(_stored(a, False), _stored(b[0], False))]], [out], 2.0, cfg=cfg)
            _same(out, 2.0 * ref_b[:G, :M, :N], what + " shared B")


@pytest.mark.parametrize("cfg", sorted({c for c, _, _ in X.refused_launches()}))
def test_dispatch_refusals(cfg):
    """Combinations without an instantiation are refused by the launcher (nothing is launched)."""
    from sparse_coding__amd.ops._lib import KernelError

    gemm = _gemm()
    G, M, N, K = 1, 256, 256, 64
    a, b = torch.zeros(G, M, K, device=DEV, dtype=BF), torch.zeros(G, N, K, device=DEV, dtype=BF)
    aux = torch.zeros(G, M, N, device=DEV, dtype=BF)
    mask = torch.zeros(gemm.code_mask_shape(G, M, N), device=DEV, dtype=torch.int64)
    f = lambda *s: torch.zeros(*s, device=DEV)
    for c, epi, layout in X.refused_launches():
        if c != cfg:
            continue
        out = torch.zeros(G, M, N, device=DEV, dtype=F32 if epi in (gemm.EPI_F32, gemm.EPI_ROWMAX) else BF)
        with pytest.raises(KernelError, match="code 8"):
            gemm._launch(epi, layout, M, N, K, 0, G, [gemm._op(a, K if layout & 1 else M, M * K)] * 2,
                         [gemm._op(b, K if layout & 2 else N, N * K)] * 2, [out], [1.0],
                         N, M * N, cfg=cfg, bias=f(G, N), sbias=N, part=f(G, 4, 2), colpart=f(G, 2, N), l1=f(G),
                         aux=aux, ldaux=N, saux=M * N, cmask=mask, act=1)
    a3, b3 = torch.zeros(192, M, device=DEV, dtype=BF), torch.zeros(192, N, device=DEV, dtype=BF)
    with pytest.raises(KernelError, match="code 7"):  # a split range must hold a whole BK64 tile
        gemm._launch(gemm.EPI_F32, 0, M, N, 192, 0, G, [gemm._op(a3, M, 0)] * 2, [gemm._op(b3, N, 0)] * 2,
                     [torch.zeros(4, G, M, N, device=DEV)], [1.0], N, M * N, cfg=cfg, ksplit=4, split_stride=G * M * N)


# ------------------------------------------------------------------ B. fused epilogues
EG, EB, EN = 2, 256, 512  # encoder / code gradient: 2 x 4 tiles of 128x128, 1 x 2 of 256x256


def _enc_case(G, B, n, d, lo=-6, hi=0, live=None, reverse=False):
    def make():
        t = {k: v.to(DEV) for k, v in X.encoder_inputs(G, B, n, d, lo, hi).items()}
        x, w = t["x"].to(BF), t["w"].to(BF)
        ref = X.check_encode(x, w, t["bias"], live, reverse, f"encoder d={d}")
        ref_shared = X.check_encode(x[0], w, t["bias"], live, reverse, f"encoder d={d}, shared x")
        return dict(x=x, w=w, bias=t["bias"].contiguous(), ref=ref, ref_shared=ref_shared)
    return _cached(("enc", G, B, n, d, lo, hi, tuple(live) if live else None, reverse), make)


def _run_encoder(cfg, case, shared, cnt, mask, act=0, nactive=None, host=None, fill=NAN):
    gemm = _gemm()
    G, n, _ = case["w"].shape
    B = case["x"].shape[1]
    c = _full((G, B, n), BF, fill)
    part = _full((G, (B // 128) * (n // 128), 2), F32, fill)
    colpart = _full((G, B // 128, n), F32, fill) if cnt else None
    mask_out = _full(gemm.code_mask_shape(G, B, n), torch.int64, -1 if fill != 0 else 0) if mask else None
    with gemm.force_shape(cfg):
        gemm.encode_relu(case["x"][0].contiguous() if shared else case["x"], case["w"], case["bias"], c, part, colpart,
                         nactive=nactive, mask_out=mask_out, act=act, live_host=host)
    return c, part, colpart, mask_out


def _check_encoder(out, ref, what):
    c, part, colpart, _ = out
    _same(c, ref["c"], what + " codes")
    _sum_same(part[..., 0], ref["l1"], what + " L1 partials")
    _sum_same(part[..., 1], ref["l0"], what + " L0 partials")
    if colpart is not None:
        _same(colpart, ref["cnt"], what + " fire counts")


@pytest.mark.parametrize("cfg", X.ALL_CFGS)
def test_encode_relu(cfg):
    gemm = _gemm()
    if not gemm.shape_fits(cfg, EB, EN):
        pytest.skip("block shape does not tile this problem")
    for d in X.fused_k_values(cfg):
        case = _enc_case(EG, EB, EN, d)
        for shared, cnt, mask in ((True, False, False), (False, True, True), (True, False, True), (False, True, False)):
            out = _run_encoder(cfg, case, shared, cnt, mask)
            _check_encoder(out, case["ref_shared" if shared else "ref"], f"cfg {cfg} d={d} shared={shared} cnt={cnt} mask={mask}")


DB, DD = 256, 256  # decoder: K = n is free


def _dec_case(G, n, live=None):
    def make():
        t = {k: v.to(DEV, BF) for k, v in X.decoder_inputs(G, DB, n, DD).items()}
        if live is not None:
            for g, s in enumerate(live):
                t["c"][g, :, s:] = 0
        t["ref"] = X.check_decode(t["c"], t["wd"], t["x"], f"decoder n={n}", live)
        t["ref_shared"] = X.check_decode(t["c"], t["wd"], t["x"][0], f"decoder n={n}, shared x", live)
        return t
    return _cached(("dec", G, n, tuple(live) if live else None), make)


def _run_decoder(cfg, case, shared, rcol, nactive=None):
    gemm = _gemm()
    G = case["c"].shape[0]
    r = _full((G, DB, DD), BF)
    part = _full((G, (DB // 128) * (DD // 128)), F32)
    rc = _full((G, DB // 128, DD), F32) if rcol else None
    with gemm.force_shape(cfg):
        gemm.decode_residual(case["c"], case["wd"], case["x"][0].contiguous() if shared else case["x"], r, part, rcol=rc,
                             nactive=nactive)
    return r, part, rc


def _check_decoder(out, ref, what):
    r, part, rc = out
    _same(r, ref["r"], what + " r")
    _sum_same(part, ref["sq"], what + " sum r^2 partials")
    if rc is not None:
        _same(rc, ref["rcol"], what + " rcol")


@pytest.mark.parametrize("cfg", X.ALL_CFGS)
def test_decode_residual(cfg):
    gemm = _gemm()
    if not gemm.shape_fits(cfg, DB, DD):
        pytest.skip("block shape does not tile this problem")
    for n in X.fused_k_values(cfg):
        case = _dec_case(2, n)
        for shared, rcol in ((False, True), (True, False), (True, True)):
            _check_decoder(_run_decoder(cfg, case, shared, rcol), case["ref_shared" if shared else "ref"],
                           f"cfg {cfg} n={n} shared={shared} rcol={rcol}")


def _dc_case(G, B, n, d, enc, key, reverse=False, live=None):
    """Code-gradient operands with K = d free; the codes and their activity come from the
    reference of an encoder case (``enc``)."""
    def make():
        t = {k: v.to(DEV) for k, v in X.codegrad_inputs(G, B, n, d).items()}
        r, w = t["r"].to(BF), t["w"].to(BF)
        c = enc["ref"]["c"].float().to(BF)
        on = enc["ref"]["on"]
        ref = X.check_code_grad(r, w, c, on, t["l1"], None if reverse else t["tied_bias"], reverse, f"code gradient d={d}", live)
        return dict(r=r, w=w, c=c, l1=t["l1"].contiguous(), tied_bias=t["tied_bias"].contiguous(), ref=ref)
    return _cached(("dc", G, B, n, d, key, reverse), make)


def _run_code_grad(cfg, case, dot=False, tied=False, mask=None, act=0, nactive=None, host=None, fill=NAN):
    gemm = _gemm()
    G, B, _ = case["r"].shape
    n = case["w"].shape[1]
    dpre = _full((G, B, n), BF, fill)
    colpart = _full((G, B // 128, n), F32, fill)
    dotpart = _full((G, B // 128, n), F32, fill) if dot else None
    with gemm.force_shape(cfg):
        gemm.code_grad(case["r"], case["w"], case["c"], case["l1"], dpre, colpart, dotpart=dotpart,
                       tied_bias=case["tied_bias"] if tied else None, mask=mask, act=act, nactive=nactive, live_host=host)
    return dpre, colpart, dotpart


@pytest.mark.parametrize("cfg", X.ALL_CFGS)
def test_code_grad(cfg):
    gemm = _gemm()
    if not gemm.shape_fits(cfg, EB, EN):
        pytest.skip("block shape does not tile this problem")
    enc = _enc_case(EG, EB, EN, 64)
    mask = _run_encoder(cfg, enc, False, False, True)[3]
    for d in X.fused_k_values(cfg):
        case = _dc_case(EG, EB, EN, d, enc, "relu")
        ref = case["ref"]
        for dot, tied, use_mask in ((False, False, False), (True, False, False), (True, True, False), (False, False, True)):
            what = f"cfg {cfg} d={d} dot={dot} tied={tied} mask={use_mask}"
            dpre, colpart, dotpart = _run_code_grad(cfg, case, dot, tied, mask if use_mask else None)
            _same(dpre, ref["dpre"], what + " dpre")
            _same(colpart, ref["colpart"], what + " colpart")
            if dot:
                _same(dotpart, ref["dot_tied" if tied else "dot"], what + " dotpart")


@pytest.mark.parametrize("cfg", X.FULL_CFGS)
def test_reverse_activation(cfg):
    gemm = _gemm()
    if not gemm.shape_fits(cfg, EB, EN):
        pytest.skip("block shape does not tile this problem")
    for d in X.fused_k_values(cfg):
        enc = _enc_case(EG, EB, EN, d, -3, 3, reverse=True)  # positive biases: codes of either sign
        assert bool((enc["ref"]["c"] < 0).any())
        for shared, cnt in ((False, True), (True, False)):
            out = _run_encoder(cfg, enc, shared, cnt, True, act=gemm.ACT_REVERSE)
            _check_encoder(out, enc["ref_shared" if shared else "ref"], f"cfg {cfg} reverse encoder d={d} shared={shared}")
            if not shared:
                mask = out[3]
        case = _dc_case(EG, EB, EN, d, enc, "reverse", reverse=True)
        dpre, colpart, _ = _run_code_grad(cfg, case, mask=mask, act=gemm.ACT_REVERSE)
        _same(dpre, case["ref"]["dpre"], f"cfg {cfg} reverse code gradient d={d} dpre")
        _same(colpart, case["ref"]["colpart"], f"cfg {cfg} reverse code gradient d={d} column sums")


@pytest.mark.parametrize("cfg", [1, 3])
def test_rowmax_nt(cfg):
    gemm = _gemm()
    G, M, N, K = 2, 130, 257, 65
    a, b = _ops("int", G, M, N, 0, K)
    a, b = a.contiguous(), b.contiguous()
    ref = X.ref_plain(a, b, 0.5)
    X.assert_accumulators(a, b, "rowmax")
    out = gemm.rowmax_nt(a, b, alpha=0.5, cfg=cfg)
    _same(out, ref.amax(-1), f"rowmax cfg {cfg}")


# ------------------------------------------------------------------ C. activity bitmask across block shapes
@pytest.mark.parametrize("reader", X.ALL_CFGS)
@pytest.mark.parametrize("writer", X.ALL_CFGS)
def test_mask_contract(writer, reader):
    """The bitmask one block shape's encoder writes is the one every shape's code gradient reads."""
    G, B, n, d = 2, 256, 256, 64
    enc = _enc_case(G, B, n, d)
    case = _dc_case(G, B, n, d, enc, "pairs")

    def write():
        out = _run_encoder(writer, enc, False, False, True)
        _check_encoder(out, enc["ref"], f"writer cfg {writer}")
        return out[3]
    mask = _cached(("mask", writer), write)
    dpre, colpart, _ = _run_code_grad(reader, case, mask=mask)
    _same(dpre, case["ref"]["dpre"], f"mask of cfg {writer} read by cfg {reader}: dpre")
    _same(colpart, case["ref"]["colpart"], f"mask of cfg {writer} read by cfg {reader}: colpart")
    dpre, colpart, _ = _run_code_grad(reader, case)
    _same(dpre, case["ref"]["dpre"], f"cfg {reader} reading c: dpre")
    _same(colpart, case["ref"]["colpart"], f"cfg {reader} reading c: colpart")


# ------------------------------------------------------------------ D. masked launches
MG, MB, MD = 4, 256, 64
MODES = [(X.MASK_SIZES, False), (X.MASK_SIZES, True), (X.MASK_SIZES_ZERO, False)]  # (live sizes, compacted)


@pytest.mark.parametrize("cfg", X.ALL_CFGS)
def test_masked_encoder_and_code_grad(cfg):
    gemm = _gemm()
    n = X.MASK_N
    for sizes, compact in MODES:
        what = f"cfg {cfg} live {sizes} compacted={compact}"
        enc = _enc_case(MG, MB, n, MD, live=sizes)
        live, host, fill = _i32(sizes), (sizes if compact else None), (0.0 if compact else NAN)
        for cnt in (True, False):
            out = _run_encoder(cfg, enc, True, cnt, True, nactive=live, host=host, fill=fill)
            _check_encoder(out, enc["ref_shared"], what + f" cnt={cnt}")
            mask = out[3]
            for g, s in enumerate(sizes):  # activity words of 64-column blocks wholly past the live size
                assert not mask[g, :, -(-s // 64):].any(), what + f": model {g} mask past the live size"
        case = _dc_case(MG, MB, n, 128, dict(ref=enc["ref_shared"]), ("masked", tuple(sizes)), live=sizes)
        dpre, colpart, _ = _run_code_grad(cfg, case, mask=mask, nactive=live, host=host, fill=fill)
        for g, s in enumerate(sizes):  # dead column tiles of dpre are unwritten by design
            _same(dpre[g, :, :s], case["ref"]["dpre"][g, :, :s], what + f" dpre of model {g}")
        _same(colpart, case["ref"]["colpart"], what + " colpart")


@pytest.mark.parametrize("cfg", X.ALL_CFGS)
def test_masked_decoder(cfg):
    """Live K ranges: the one path that gives a fused epilogue an odd K-tile count on a BK32 ring."""
    gemm = _gemm()
    if not gemm.shape_fits(cfg, DB, DD):
        pytest.skip("block shape does not tile this problem")
    for sizes in (X.MASK_SIZES, X.MASK_SIZES_ZERO):
        case = _dec_case(MG, X.MASK_N, live=sizes)
        for shared in (False, True):
            _check_decoder(_run_decoder(cfg, case, shared, True, nactive=_i32(sizes)), case["ref_shared" if shared else "ref"],
                           f"cfg {cfg} live {sizes} shared={shared}")


@pytest.mark.parametrize("cfg", X.ALL_CFGS)
def test_masked_weight_grad(cfg):
    gemm = _gemm()
    n, d, Bk = X.MASK_N, 256, 256
    if not gemm.shape_fits(cfg, n, d):
        pytest.skip("block shape does not tile this problem")
    for sizes, compact in MODES:
        def make():
            t = {k: v.to(DEV, BF) for k, v in X.wgrad_masked_inputs(MG, Bk, n, d, tuple(sizes)).items()}
            at, bt = t["a"].transpose(1, 2), t["b"].transpose(1, 2)  # logical [G, n, Bk], [G, d, Bk]
            t["ref"] = X.ref_plain(at, bt)
            X.assert_accumulators(at, bt, "masked weight gradient")
            X.assert_bf16_out(t["ref"], "masked weight gradient")
            for g, s in enumerate(sizes):
                if s:
                    X.assert_k_tiles_contribute(at[g:g + 1], bt[g:g + 1], f"masked weight gradient model {g}")
                assert not t["ref"][g, s:].any()
            t["halves"] = [X.ref_plain(at[..., k:k + Bk // 2], bt[..., k:k + Bk // 2]) for k in (0, Bk // 2)]
            return t
        t = _cached(("wg", tuple(sizes)), make)
        live, host, fill = _i32(sizes), (sizes if compact else None), (0.0 if compact else NAN)
        for dtype in (F32, BF):
            for ks in ((1, 2) if cfg == 3 else (1,)):  # (split-K picks its own block shape)
                what = f"cfg {cfg} live {sizes} compacted={compact} {dtype} ksplit={ks}"
                alpha = 0.5 if dtype == F32 else 1.0
                out = _full(((ks,) if ks > 1 else ()) + (MG, n, d), dtype, fill)
                gemm.weight_grads([[(t["a"], t["b"])]], [out], alpha, ksplit=ks, nactive=live, live_host=host, cfg=cfg)
                if ks == 1:
                    _same(out, alpha * t["ref"], what)
                else:
                    for i in range(2):
                        _same(out[i], alpha * t["halves"][i], what + f" slab {i}")
