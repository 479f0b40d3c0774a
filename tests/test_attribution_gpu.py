"""Attribution on the MI355X: the kernels of ``csrc/attribution.hip`` against the torch oracle on the inputs of
``attribution_cases.py`` -- planted rows on which every fp32 operation is exact (``torch.equal``), the order of the
fp64 list sums, list lengths around 64, launch geometry, sentinels, the guards, the forward bound on random rows
-- and ``attribution`` of the engines and the trainer."""

import pytest
import torch

import attribution_cases as C
import sparse_recon_cases as SRC

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = C.G
SENTINEL = -12345.0
OUT_SENTINELS = (-7, -3.0, -5.0, -9.0, -11, -13.0, -15.0)      # one per output of the list walk


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_coding__amd.ops import _lib as L

    L.lib()  # must load: no silent fallback on a GPU box
    yield


def _dev(k):
    return k["sc"].to(DEV), k["D"].to(DEV), k["x"].to(DEV)


def _live(live):
    return torch.tensor(live, dtype=torch.int32, device=DEV)


def _zeros(n=G):
    return torch.zeros(n, dtype=torch.int64, device=DEV)


def _expected_proj(sc, rp, row0=0):
    """What ``proj`` must hold after a launch on a sentinel-filled buffer: the oracle's value at the entries of the
    window's valid rows, the sentinel everywhere else."""
    want = torch.full((sc.n_models, sc.cap), SENTINEL)
    for g in range(sc.n_models):
        for r in torch.nonzero(rp.valid[g]).flatten().tolist():
            lo, hi = int(sc.row_ptr[g, row0 + r]), int(sc.row_ptr[g, row0 + r + 1])
            want[g, lo:hi] = rp.proj[g, lo:hi]
    return want


# ----------------------------------------------------------------------------- 1. planted rows: every bit
@pytest.mark.parametrize("case", C.PLANTED, ids=C.PLANTED_IDS)
def test_planted_is_bit_exact(case):
    from sparse_coding__amd.engine import attribution as at
    from sparse_coding__amd.ops import attribution as at_ops
    from sparse_coding__amd.ops import sparse_recon as sr_ops

    k = C.planted(*case)
    sc, D, x = _dev(k)
    live = _live(k["live"])
    assert sorted(set(k["lens"]))[:3] == [0, 1, 2] and case[1] in k["lens"]
    for shared in (False, True):
        ref, rp = C.planted_reference(*case, shared)
        xs = x[0].contiguous() if shared else x
        for _ in range(2):                                          # (twice in a row: the same bits)
            sk = _zeros()
            proj = torch.full((G, sc.cap), SENTINEL, device=DEV)
            sse = torch.full((G, sc.n_rows), SENTINEL, device=DEV)
            at_ops.residual_proj(sc.row_ptr, sc.col, sc.val, D, xs, sk, nactive=live, proj=proj, sse_row=sse)
            assert torch.equal(proj.cpu(), _expected_proj(k["sc"], rp)) and torch.equal(sse.cpu(), rp.sse_row)
            assert not sk.any() and bool(rp.valid.all())
            assert torch.equal(rp.proj.double(), rp.proj64) and torch.equal(rp.sse_row.double(), rp.sse64)
        split = sr_ops.recon_split(sc.row_ptr, sc.col, sc.val, D, xs, _zeros(), nactive=live)
        assert torch.equal(split[..., 0], sse)                      # the bits of recon_split's full residual
        got = at.attribution(sc, D, xs, k["live"], return_proj=True)
        assert got.A.is_cuda and got.check() is got
        C.same(got, ref, C.RAW + ("q", "sse_full", "s2", "skipped", "missing", "proj"))
        assert torch.equal(got.delta_sse.cpu(), ref.delta_sse) and torch.equal(got.top_mask(5).cpu(), ref.top_mask(5))
    # a row window with row0 > 0: only its entries are written
    n_win = sc.n_rows - C.ROW0
    proj = torch.full((G, sc.cap), SENTINEL, device=DEV)
    _, sse = at_ops.residual_proj(sc.row_ptr, sc.col, sc.val, D, x[:, C.ROW0:].contiguous(), _zeros(), row0=C.ROW0,
                                  n_rows=n_win, nactive=live, proj=proj)
    from sparse_coding__amd.engine.attribution import residual_proj_reference

    win = residual_proj_reference(k["sc"], k["D"], k["x"][:, C.ROW0:], k["live"], row0=C.ROW0, n_rows=n_win)
    _, rp = C.planted_reference(*case, False)
    want = _expected_proj(k["sc"], win, C.ROW0)
    assert torch.equal(proj.cpu(), want) and torch.equal(sse.cpu(), rp.sse_row[:, C.ROW0:])
    assert bool((want[:, 0] == SENTINEL).all()) and bool((want != SENTINEL).any())


# ----------------------------------------------------------------------------- 2. the list walk
def _walk(k, sc=None, fc=None, proj=None, waves=4, out=None):
    from sparse_coding__amd.ops import attribution as at_ops

    sc = k["sc"] if sc is None else sc
    fc = k["fc"] if fc is None else fc
    proj = k["proj"] if proj is None else proj
    missing = _zeros()
    got = at_ops.attr_list_sums(fc.col_ptr.to(DEV), fc.row.to(DEV), fc.val.to(DEV), sc.row_ptr.to(DEV).contiguous(),
                                sc.col.to(DEV), proj.to(DEV), k["q"].to(DEV), missing, waves=waves, out=out)
    torch.cuda.synchronize()
    return [t.cpu() for t in got] + [missing.cpu()]


def test_list_sums_order_lengths_geometry_and_sentinels():
    k = C.lists()
    want = k["want"]
    assert want[0][0, :7].tolist() == [0, 1, 63, 64, 65, 129, C.LIST_ROWS]
    for waves in (1, 2, 4):
        for _ in range(2):
            out = tuple(torch.full((G, C.LIST_N), s, device=DEV, dtype=w.dtype) for s, w in zip(OUT_SENTINELS, want))
            got = _walk(k, waves=waves, out=out)
            for name, a, b in zip(C.RAW + ("missing",), got, want):
                assert a.dtype == b.dtype and torch.equal(a, b), (waves, name)
    A, P1 = got[1], got[2]
    for g in range(G):      # the literals that follow from the stated order
        assert A[g, C.F_ORDER_LANE0].item() == C.ORDER_LANE0 == 9007199254740992.0
        assert A[g, C.F_ORDER_012].item() == C.ORDER_012 == 9007199254740992.0
        assert A[g, C.F_ORDER_MIX].item() == C.ORDER_MIX == 9007199254740994.0 != C.SEQUENTIAL
        assert P1[g, C.F_ORDER_MIX].item() == C.ORDER_MIX
    with pytest.raises(ValueError, match="waves"):
        _walk(k, waves=3)


def _lane_sums(col_ptr, terms):
    """fp64 [G, n]: ``terms`` [G, cap] summed per list in the stated order, in plain torch."""
    Gm, n = col_ptr.shape[0], col_ptr.shape[1] - 1
    cnt = col_ptr[:, 1:] - col_ptr[:, :-1]
    lanes = torch.arange(64)
    s = torch.zeros(Gm, n, 64, dtype=torch.float64)
    for c0 in range(0, int(cnt.max()), 64):
        idx = col_ptr[:, :-1, None] + c0 + lanes
        live = (c0 + lanes) < cnt[..., None]
        t = terms.gather(1, idx.clamp(max=terms.shape[1] - 1).view(Gm, -1)).view(Gm, n, 64)
        s = s + torch.where(live, t, torch.zeros((), dtype=torch.float64))
    for o in (1, 2, 4, 8, 16, 32):
        s = s + s[..., lanes ^ o]
    return s[..., 0]


def test_by_feature_of_proj_is_an_independent_cross_check():
    """``by_feature`` moves ``val`` bits verbatim: transposing codes whose values are ``proj`` gives a list aligned
    with the feature's codes, without any search."""
    from sparse_coding__amd.engine.sparse_codes import SparseCodes

    k = C.lists()
    sc = k["sc"].to(DEV)
    fc = sc.by_feature()
    fp = SparseCodes(sc.n_rows, sc.n, sc.row_ptr, sc.col, k["proj"].to(DEV)).by_feature()
    torch.cuda.synchronize()
    assert torch.equal(fc.col_ptr, fp.col_ptr) and torch.equal(fc.row, fp.row)
    got = _walk(k, fc=fc)
    c, p = fc.val.cpu().double(), fp.val.cpu().double()
    assert torch.equal(got[1], _lane_sums(fc.col_ptr.cpu(), c * p))
    assert torch.equal(got[2], _lane_sums(fc.col_ptr.cpu(), p))
    assert torch.equal(got[3], _lane_sums(fc.col_ptr.cpu(), c * c))


# ----------------------------------------------------------------------------- 3. the guards
BIG_CASE = (64, 320)


def _guarded(row_ptr=None, live=None):
    """Run both kernels and the oracle on the planted case with a changed ``row_ptr`` / ``nactive`` and compare
    every output; returns (the Attribution, the oracle's ResidualProj, what ``proj`` must hold)."""
    from sparse_coding__amd.engine import attribution as at
    from sparse_coding__amd.engine.sparse_codes import SparseCodes
    from sparse_coding__amd.ops import attribution as at_ops

    k = C.planted(*BIG_CASE)
    live = k["live"] if live is None else live
    sc = k["sc"] if row_ptr is None else SparseCodes(k["sc"].n_rows, k["sc"].n, row_ptr, k["sc"].col, k["sc"].val)
    rp = at.residual_proj_reference(sc, k["D"], k["x"], live)
    ref = at.attribution_reference(sc, k["D"], k["x"], live, residual=rp)
    dsc, D, x = sc.to(DEV), k["D"].to(DEV), k["x"].to(DEV)
    sk = _zeros()
    proj = torch.full((G, sc.cap), SENTINEL, device=DEV)
    _, sse = at_ops.residual_proj(dsc.row_ptr, dsc.col, dsc.val, D, x, sk, nactive=_live(live), proj=proj)
    got = at.attribution(dsc, D, x, live)
    torch.cuda.synchronize()
    want = _expected_proj(sc, rp)
    assert torch.equal(proj.cpu(), want)                  # (skipped rows store nothing)
    assert torch.equal(sse.cpu(), rp.sse_row) and torch.equal(sk.cpu(), rp.skipped)
    C.same(got, ref)
    return got, rp, want


def test_rows_with_bad_pointers_are_skipped_and_store_nothing():
    k = C.planted(*BIG_CASE)
    sc = k["sc"]
    rp_ = sc.row_ptr.clone()
    rp_[1, 4] = sc.cap + 7                       # row 3 of model 1 runs past the buffers, row 4 ends before it starts
    got, rp, want = _guarded(row_ptr=rp_)
    assert got.skipped.tolist() == [0, 2] and not rp.valid[1, 3:5].any() and not rp.sse_row[1, 3:5].any()
    lo, hi = int(sc.row_ptr[1, 3]), int(sc.row_ptr[1, 5])
    assert hi - lo == 63 + 64 and bool((want[1, lo:hi] == SENTINEL).all())
    rp_ = sc.row_ptr.clone()
    rp_[1, -1] = sc.cap + 5                      # the last row of model 1 runs past the buffers
    got, rp, want = _guarded(row_ptr=rp_)
    assert got.skipped.tolist() == [0, 1] and not rp.valid[1, -1]
    lo = int(sc.row_ptr[1, -2])
    assert lo < sc.cap and bool((want[1, lo:] == SENTINEL).all())
    with pytest.raises(Exception):
        got.check()
    rp_ = sc.row_ptr.clone()
    rp_[0, 0] = -1                               # row 0 starts before the buffers
    got, _, _ = _guarded(row_ptr=rp_)
    assert got.skipped.tolist() == [1, 0]


def test_a_column_past_nactive_skips_its_row_only():
    k = C.planted(*BIG_CASE)
    rows = int((k["dense"][1, :, 200:] > 0).any(-1).sum())
    got, rp, _ = _guarded(live=[320, 200])
    assert got.skipped.tolist() == [0, rows] and 0 < rows < C.N_PLANTED
    assert not got.cnt[1, 200:].any() and not got.missing.any()


def test_list_entries_outside_the_rows_or_of_other_codes_are_missing():
    from sparse_coding__amd.engine.sparse_codes import SparseCodes, sparse_codes_reference

    k = C.lists()
    sc, fc = k["sc"], k["fc"]
    dense = torch.stack([sc.to_dense(g) for g in range(G)]) > 0
    # the CSR holds 60 rows fewer than the lists were built from
    short = SparseCodes(sc.n_rows - 60, sc.n, sc.row_ptr[:, :-60].contiguous(), sc.col, sc.val)
    got = _walk(k, sc=short)
    assert got[7].tolist() == dense[:, -60:].sum((1, 2)).tolist() and bool(got[7].all())
    assert torch.equal(got[0], dense[:, :-60].sum(1))
    # lists built from other codes: the search fails wherever the CSR has no such column in that row
    from sparse_coding__amd.engine import attribution as at

    other = sparse_codes_reference([torch.flip(sc.to_dense(0), [1]).unsqueeze(0).repeat(G, 1, 1)])
    proj = torch.randn(G, other.cap, generator=torch.Generator().manual_seed(5))
    got = _walk(k, sc=other, proj=proj)
    dense_b = torch.stack([other.to_dense(g) for g in range(G)]) > 0
    assert got[7].tolist() == (dense & ~dense_b).sum((1, 2)).tolist() and bool(got[7].all())
    assert torch.equal(got[0], (dense & dense_b).sum(1))
    want = at.attr_list_sums_reference(fc, other, proj, k["q"])
    for name, a, b in zip(C.RAW + ("missing",), got, want):
        assert torch.equal(a, b), name


def test_host_refusals_and_graph_capture():
    from sparse_coding__amd.ops import attribution as at_ops
    from sparse_coding__amd.ops.interference import row_norm2

    k = C.planted(512, 96)
    sc, D, x = _dev(k)
    live = _live(k["live"])
    sk = _zeros()
    for d in (32, 96, 1088):
        with pytest.raises(ValueError, match="d % 64"):
            at_ops.residual_proj(sc.row_ptr, sc.col, sc.val, torch.zeros(G, sc.n, d, device=DEV, dtype=torch.bfloat16),
                                 torch.zeros(G, sc.n_rows, d, device=DEV, dtype=torch.bfloat16), sk)
    with pytest.raises(ValueError, match="x must be"):
        at_ops.residual_proj(sc.row_ptr, sc.col, sc.val, D, x.cpu(), sk)
    with pytest.raises(ValueError, match="proj"):
        at_ops.residual_proj(sc.row_ptr, sc.col, sc.val, D, x, sk, proj=torch.zeros(G, sc.cap + 1, device=DEV))
    assert not sk.any()
    # both launches inside one captured graph
    ref, rp = C.planted_reference(512, 96, False)
    fc = sc.by_feature(k["live"])
    q = row_norm2(D)
    proj = torch.zeros(G, sc.cap, device=DEV)
    sse = torch.empty(G, sc.n_rows, device=DEV)
    missing = _zeros()
    out = tuple(torch.empty(G, sc.n, device=DEV, dtype=getattr(ref, f).dtype) for f in C.RAW)

    def run():
        at_ops.residual_proj(sc.row_ptr, sc.col, sc.val, D, x, sk, nactive=live, proj=proj, sse_row=sse)
        at_ops.attr_list_sums(fc.col_ptr, fc.row, fc.val, sc.row_ptr, sc.col, proj, q, missing, out=out)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    proj.fill_(SENTINEL)
    sse.fill_(SENTINEL)
    for t in out:
        t.fill_(-3)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(proj.cpu(), _expected_proj(k["sc"], rp)) and torch.equal(sse.cpu(), rp.sse_row)
    for f, t in zip(C.RAW, out):
        assert torch.equal(t.cpu(), getattr(ref, f)), f
    assert not sk.any() and not missing.any()


# ----------------------------------------------------------------------------- 4. random rows: the forward bound
def test_random_rows_stay_inside_the_fp32_bound():
    """``|p^_e - p_e| <= gamma_L sum_k |a_k| m_k + gamma_{P + 6} sum_k |r_k| |a_k|`` with the oracle's exact values
    (``ResidualProj.bound``).  Measured on one MI355X: see profiles/r19/attribution/README.md."""
    from sparse_coding__amd.engine import attribution as at
    from sparse_coding__amd.ops import sparse_recon as sr_ops

    k = C.random_rows()
    sc, D, x = _dev(k)
    ref = k["ref"]
    got = at.attribution(sc, D, x, return_proj=True)
    torch.cuda.synchronize()
    stored = torch.arange(sc.cap).unsqueeze(0) < k["sc"].row_ptr[:, -1:]
    err = (got.proj.cpu().double() - ref.proj64).abs()
    ratio = float((err[stored] / ref.bound[stored]).max())
    print(f"random rows: largest |proj - exact| / bound = {ratio:.4f}, largest |proj - exact| = "
          f"{float(err[stored].max()):.3e}, entries = {int(stored.sum())}")
    assert bool((err <= ref.bound)[stored].all()) and not got.proj.cpu()[~stored].any()
    split = sr_ops.recon_split(sc.row_ptr, sc.col, sc.val, D, x, _zeros())
    assert torch.equal(split[..., 0].sum(1, dtype=torch.float64), got.sse_full)
    # the list walk on the kernel's own proj and q: the oracle's bits
    want = at.attribution_reference(k["sc"], k["D"], k["x"], proj=got.proj.cpu(), q=got.q.cpu(), residual=ref)
    C.same(got, want)
    assert torch.equal(got.q.cpu(), at.row_norm2_reference(k["D"]))
    assert bool((got.n_harm > 0).any()) and bool((got.rescale.cpu()[want.cnt > 0] > 0).all())


# ----------------------------------------------------------------------------- 5. engines
B_ENG, N_DICT, D_ACT = 128, 256, 256      # (the shapes test_sparse_recon_gpu.py builds its engines at)
N_POOL = 3 * B_ENG
GE = 3


def _models(kind, dict_size=None):
    from sparse_coding__amd.models import signatures as S

    l1s = [1e-4, 1e-3, 1e-2]
    if dict_size is not None:
        return S.FunctionalMaskedSAE, [S.FunctionalMaskedSAE.init(D_ACT, k, N_DICT, l1, device=DEV)
                                       for k, l1 in zip(dict_size, l1s)]
    sig = S.FunctionalSAE if kind == "untied" else S.FunctionalTiedSAE
    if kind == "centred":
        gen = torch.Generator(device=DEV).manual_seed(11)
        models = []
        for l1 in l1s:
            rot = torch.linalg.qr(torch.randn(D_ACT, D_ACT, device=DEV, generator=gen)).Q.contiguous()
            models.append(sig.init(D_ACT, N_DICT, l1, device=DEV, rotation=rot,
                                   translation=torch.randn(D_ACT, device=DEV, generator=gen) * 0.1,
                                   scaling=torch.rand(D_ACT, device=DEV, generator=gen) + 0.5))
        return sig, models
    return sig, [sig.init(D_ACT, N_DICT, l1, device=DEV) for l1 in l1s]


def _engine(sig, models, **kw):
    from sparse_coding__amd.engine.fused import FusedSAEEnsemble

    models = [({k: t.clone() for k, t in p.items()}, b) for p, b in models]
    return FusedSAEEnsemble(models, sig, lr=1e-3, batch_size=B_ENG, device=DEV, count_every=1, **kw)


def _data(seed=0, batches=3):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    feats = torch.nn.functional.normalize(torch.randn(1024, D_ACT, device=DEV, generator=gen), dim=-1)
    codes = torch.relu(torch.randn(batches * B_ENG, 1024, device=DEV, generator=gen) - 2.0)
    return (codes @ feats).to(torch.bfloat16)


def _state_tensors(eng):
    out = {f"p.{k}": t for k, t in eng.params.items()}
    out.update({f"m.{k}": t for k, t in eng.m.items()})
    out.update({f"v.{k}": t for k, t in eng.v.items()})
    out.update(enc_shadow=eng.enc_shadow, dec_shadow=eng.dec_shadow, norms=eng.norms, out=eng.out,
               step_dev=eng.step_dev, feature_counts=eng.feature_counts)
    return out


def _prepared(eng, pool):
    B = eng.batch_size
    return torch.cat([eng.prepare(pool[i:i + B]).clone() for i in range(0, pool.shape[0], B)], dim=-2)


def _assert_attribution(got, codes, shadow, x, live=None):
    """``got`` (with ``proj``) against the oracle on the engine's own sparse codes, bf16 shadow and prepared rows:
    ``proj`` inside its bound, ``sse_row`` sums inside theirs, and the per-feature sums bit-equal to the oracle fed
    the kernel's ``proj`` and ``q``.  Returns (the oracle's ResidualProj, per-feature bound on ``delta_sse``)."""
    from sparse_coding__amd.engine import attribution as at

    torch.cuda.synchronize()
    sc, Dc, xc = codes.to("cpu"), shadow.cpu(), x.cpu()
    rp = at.residual_proj_reference(sc, Dc, xc, live)
    want = at.attribution_reference(sc, Dc, xc, live, proj=got.proj.cpu(), q=got.q.cpu(), residual=rp)
    C.same(got, want)
    assert got.A.is_cuda and got.n_rows == sc.n_rows
    err = (got.proj.cpu().double() - rp.proj64).abs()
    ok = rp.bound > 0
    assert bool((err <= rp.bound)[ok].all()) and not got.proj.cpu()[~ok & (rp.proj64 == 0)].any()
    assert torch.allclose(got.sse_full.cpu(), rp.sse64.sum(1), rtol=1e-5)
    assert torch.allclose(got.s1.cpu(), want.s1, rtol=1e-12, atol=1e-9) and torch.allclose(got.s2.cpu(), want.s2)
    tol = torch.zeros(sc.n_models, sc.n, dtype=torch.float64)
    for g in range(sc.n_models):
        kk = min(int(sc.row_ptr[g, -1]), sc.cap)
        tol[g].index_add_(0, sc.col[g, :kk].long(), 2 * sc.val[g, :kk].double() * rp.bound[g, :kk])
    tol += want.C2 * want.q.double() * at._gamma(Dc.shape[2] // 16 + 4)
    return rp, tol


def _all_but(f, Gm, n):
    mask = torch.ones(Gm, n, dtype=torch.bool, device=DEV)
    mask[:, f] = False
    return mask


def _assert_agrees_with_recon_profile(eng, pool, got, codes, shadow, x, tol, live=None):
    """``delta_sse[:, f]`` against ``recon_profile(keep=all-but-f).sse_keep - sse_full`` for three features, within
    the sum of the two error bounds (the projection's and the two residual norms')."""
    from sparse_coding__amd.engine import sparse_recon as sr

    Gm, n = got.A.shape
    d = shadow.shape[2]
    busiest = got.cnt[0].argmax().item()
    for f in (busiest, int(got.delta_sse[0].argmax()), int(got.delta_sse[0].argmin())):
        mask = _all_but(f, Gm, n)
        prof = eng.recon_profile(pool, max_kept=0, keep=mask)
        torch.cuda.synchronize()
        ref = sr.sparse_recon_reference(codes.to("cpu"), shadow.cpu(), x.cpu(), 0, mask.cpu(), live)
        b = SRC.value_bound(ref.split, ref.split_rm, ref.split_mm, ref.split_cnt, d).sum(1)
        diff = (prof.sse_keep - prof.sse_full).cpu()
        mine = got.delta_sse[:, f].cpu()
        bound = tol[:, f] + b[:, 0] + b[:, 1]
        print(f"feature {f}: delta_sse {mine.tolist()}, recon_profile difference {diff.tolist()}, "
              f"bound {bound.tolist()}")
        assert bool(((diff - mine).abs() <= bound * (1 + 1e-9)).all())


@pytest.mark.parametrize("kind", ["untied", "centred"])
def test_sae_engine_attribution_matches_oracle(kind):
    from sparse_coding__amd.engine import attribution as at

    sig, models = _models(kind)
    eng = _engine(sig, models)
    assert (eng.centering is not None) == (kind == "centred")
    eng.step_batch(_data(seed=2, batches=1))  # biases and moments away from their initial values
    pool = _data(seed=1)
    got = eng.attribution(pool, return_proj=True)
    codes = eng.encode_sparse(pool)
    x = _prepared(eng, pool)
    assert x.dim() == (3 if kind == "centred" else 2)
    rp, tol = _assert_attribution(got, codes, eng.dec_shadow, x)
    assert not rp.skipped.any() and got.check() is got and got.live is None
    assert torch.equal(got.sse_full, eng.recon_profile(pool, max_kept=0).sse_full)
    _assert_agrees_with_recon_profile(eng, pool, got, codes, eng.dec_shadow, x, tol)
    # chunk by chunk through state= is merge of the separate calls
    a, b = eng.attribution(pool[:B_ENG]), eng.attribution(pool[B_ENG:])
    part = eng.attribution(pool[B_ENG:], state=a)
    torch.cuda.synchronize()
    C.same(part, a.merge(b), C.RAW + ("q", "sse_full", "s1", "s2", "skipped", "missing"))
    for f in ("cnt", "n_harm", "min_delta", "max_delta"):
        assert torch.equal(getattr(part, f), getattr(got, f)), f
    assert torch.allclose(part.A, got.A, rtol=1e-9, atol=1e-9)
    # a budget that is too small: the rows that lost entries are skipped and counted
    budget = max(1, int(codes.nnz().min()) // N_POOL // 2)
    tight = eng.attribution(pool, budget=budget, return_proj=True)
    rp, _ = _assert_attribution(tight, eng.encode_sparse(pool, budget=budget), eng.dec_shadow, x)
    assert bool((rp.skipped > 0).all()) and not tight.missing.any()
    with pytest.raises(at.AttributionSkipped):
        tight.check()
    top, rest = eng.fvu_top_activating(pool, 4, rank_by="delta_sse")
    want = eng.recon_profile(pool, max_kept=0, keep=got.top_mask(4))
    assert torch.equal(top, want.fvu_keep) and torch.equal(rest, want.fvu_rest)
    for bad in (pool[: B_ENG + 64], pool[:0], pool[:, :128]):
        with pytest.raises(ValueError):
            eng.attribution(bad)
    with pytest.raises(ValueError):
        eng.attribution(pool, state="no state")


def test_masked_sae_engine_attribution():
    sizes = [128, 256, 256]
    sig, models = _models("untied", sizes)
    eng = _engine(sig, models)
    pool = _data(seed=7)
    got = eng.attribution(pool, return_proj=True)
    rp, _ = _assert_attribution(got, eng.encode_sparse(pool), eng.dec_shadow, _prepared(eng, pool), live=sizes)
    assert not rp.skipped.any() and not got.cnt[0, 128:].any() and bool(got.cnt[1, 128:].any())
    mask = got.top_mask(200)
    assert mask.sum(1).tolist() == [128, 200, 200] and not mask[0, 128:].any()


def test_attribution_leaves_training_state_alone():
    sig, models = _models("untied")
    a, b = _engine(sig, models).enable_graph(), _engine(sig, models).enable_graph()
    xs = _data(seed=3, batches=2)
    pool = _data(seed=4)
    for e in (a, b):
        e.step_batch(xs[:B_ENG])
    graphs = dict(a._graph)
    a.attribution(pool)
    a.attribution(pool, budget=64, return_proj=True)
    for e in (a, b):
        e.step_batch(xs[B_ENG:])
    torch.cuda.synchronize()
    assert set(a._graph) == set(graphs) and all(a._graph[k] is g for k, g in graphs.items())
    assert a.step_count == b.step_count == 2 and a.rows_seen == b.rows_seen
    sa, sb = _state_tensors(a), _state_tensors(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_unsupported_kinds_are_refused():
    from sparse_coding__amd.models.signatures import FunctionalReverseSAE

    models = [FunctionalReverseSAE.init(D_ACT, N_DICT, l1, device=DEV) for l1 in (1e-4, 1e-3, 1e-2)]
    eng = _engine(FunctionalReverseSAE, models)
    with pytest.raises(NotImplementedError, match="attribution: reverse"):
        eng.attribution(_data(seed=1, batches=1))


TK_B, TK_N, TK_D = 256, 512, 256
KS = (4, 24, 64)


def _topk_engine(seed=101, n_batches=2):
    from sparse_coding__amd.engine.topk import FusedTopKEnsemble
    from sparse_coding__amd.models.topk import TopKEncoder

    gen = torch.Generator().manual_seed(seed)
    W = torch.randn(GE, TK_N, TK_D, generator=gen)
    x = torch.randn(n_batches * TK_B, TK_D, generator=gen).to(torch.bfloat16)
    models = []
    for g, k in enumerate(KS):
        p, b = TopKEncoder.init(TK_D, TK_N, k, device=DEV)
        p["dict"] = W[g].to(DEV).clone()
        models.append((p, b))
    return FusedTopKEnsemble(models, batch_size=TK_B, device=DEV, lr=1e-3), models, x.to(DEV)


def test_topk_engine_attribution_matches_oracle():
    eng, _, pool = _topk_engine()
    before = {k: t.clone() for k, t in eng.params.items()}
    shadow, steps = eng.shadow.clone(), eng.step_count
    got = eng.attribution(pool, return_proj=True)
    codes = eng.encode_sparse(pool)
    rp, tol = _assert_attribution(got, codes, eng.shadow, pool)
    assert not rp.skipped.any() and got.check() is got
    assert int(got.cnt[0].sum()) == 4 * 2 * TK_B
    _assert_agrees_with_recon_profile(eng, pool, got, codes, eng.shadow, pool, tol)
    part = eng.attribution(pool[TK_B:], state=eng.attribution(pool[:TK_B]))
    torch.cuda.synchronize()
    C.same(part, eng.attribution(pool[:TK_B]).merge(eng.attribution(pool[TK_B:])),
           C.RAW + ("q", "sse_full", "s1", "s2", "skipped", "missing"))
    top, rest = eng.fvu_top_activating(pool, 3, rank_by="delta_sse")
    want = eng.recon_profile(pool, max_kept=0, keep=got.top_mask(3))
    assert torch.equal(top, want.fvu_keep) and torch.equal(rest, want.fvu_rest)
    torch.cuda.synchronize()
    assert eng.step_count == steps and torch.equal(eng.shadow, shadow)
    for k in before:
        assert torch.equal(eng.params[k], before[k])
    with pytest.raises(ValueError):
        eng.attribution(pool[:100])


def test_trainer_routes_to_the_engines():
    from sparse_coding__amd.engine import attribution as at
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.topk import TopKEncoder

    sig, models = _models("untied")
    tr = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV)
    assert tr.kind == "fused-sae"
    pool = _data(seed=5)
    got, want = tr.attribution(pool.cpu(), budget=N_DICT), tr.impl.attribution(pool, budget=N_DICT)
    torch.cuda.synchronize()
    assert isinstance(got, at.Attribution) and got.A.is_cuda and got.n_rows == N_POOL
    C.same(got, want, C.RAW + ("q", "sse_full", "s1", "s2", "skipped", "missing"))
    top, rest = tr.fvu_top_activating(pool, 2, rank_by="delta_sse")
    prof = tr.impl.recon_profile(pool, max_kept=0, keep=want.top_mask(2))
    assert torch.equal(top, prof.fvu_keep) and torch.equal(rest, prof.fvu_rest)
    top_s, rest_s = tr.fvu_top_activating(pool, 2)
    again = tr.fvu_top_activating(pool, 2, rank_by="sum")
    assert torch.equal(top_s, again[0]) and torch.equal(rest_s, again[1])
    _, tk_models, x = _topk_engine(seed=102, n_batches=1)
    tr = EnsembleTrainer(tk_models, TopKEncoder, lr=1e-3, batch_size=TK_B, device="cuda:0")
    assert tr.kind == "fused-topk"
    got, want = tr.attribution(x.cpu()), tr.impl.attribution(x)
    torch.cuda.synchronize()
    C.same(got, want, C.RAW + ("q", "sse_full", "s1", "s2", "skipped", "missing"))
    # the torch path on the device (analytic engine)
    an = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV, engine="analytic")
    res = an.attribution(pool[:B_ENG])
    assert res.n_rows == B_ENG and not res.skipped.any() and int(res.cnt.sum()) > 0
