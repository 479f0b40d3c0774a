"""Whole-dictionary ridge probes on the MI355X: the kernels of ``csrc/probe.hip`` against their fp64 oracles -- an
exact tier (codes from {0.5, 1, 2, 3}, small-integer operands: every fp64 sum is exact in any order, so the
comparison is ``torch.equal``) and a realistic tier (random fp32 operands, one fp32 rounding plus the fp64
accumulation) -- the solver against the dense normal equations, graph capture, and ``ridge_probes`` of the engines
and the trainer."""

import pytest
import torch

import probe_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 64
MARK = -7777.0                            # what the outputs hold before a launch
WAVES = (1, 4, 2, 4)                      # (the last repeats a geometry: a second run, the same bits)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_coding__amd.ops import _lib as L

    L.lib()  # must load: no silent fallback on a GPU box
    yield


def _padded(shape, dtype=torch.float32):
    """A ``MARK``-filled buffer of ``shape`` cut from a flat one with PAD spare elements on either side."""
    flat = torch.full((torch.Size(shape).numel() + 2 * PAD,), MARK, device=DEV, dtype=dtype)
    return flat, flat[PAD:flat.numel() - PAD].view(shape)


def _intact(flat, out):
    """Canaries on both sides untouched, every element in between written."""
    return bool((flat[:PAD] == MARK).all()) and bool((flat[-PAD:] == MARK).all()) and not bool((out == MARK).any())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _rows(sc, P, shift=None, mask=None, nactive=None, waves=4):
    from sparse_coding__amd.ops import probe as pr

    dev = sc.to(DEV)
    G, N = sc.n_models, sc.n_rows
    flat, Q = _padded((G, N, 32))
    args = [None if t is None else t.to(DEV) for t in (P, shift, mask)]
    live = None if nactive is None else torch.tensor(nactive, dtype=torch.int32, device=DEV)
    keep = [t.clone() for t in (dev.row_ptr, dev.col, dev.val, args[0])]
    out, skipped = pr.rows_matmul(dev.row_ptr, dev.col, dev.val, args[0], shift=args[1], mask=args[2], nactive=live,
                                  out=Q, waves=waves)
    torch.cuda.synchronize()
    assert out is Q and _intact(flat, Q)
    for a, b in zip(keep, (dev.row_ptr, dev.col, dev.val, args[0])):
        assert torch.equal(a, b)
    return Q.cpu(), skipped.cpu()


def _lists(fc, R, segment=None, waves=4):
    from sparse_coding__amd.ops import probe as pr

    dev, dR = fc.to(DEV), R.to(DEV)
    flat, S = _padded((fc.n_models, fc.n, 32))
    keep = [t.clone() for t in (dev.col_ptr, dev.row, dev.val, dR)]
    kw = {} if segment is None else {"segment": segment}
    out = pr.lists_matmul(dev.col_ptr, dev.row, dev.val, dR, out=S, waves=waves, **kw)
    torch.cuda.synchronize()
    assert out is S and _intact(flat, S)
    for a, b in zip(keep, (dev.col_ptr, dev.row, dev.val, dR)):
        assert torch.equal(a, b)
    return S.cpu()


# ----------------------------------------------------------------------------- exact tier
@pytest.mark.parametrize("n", [70, 130])
def test_rows_matmul_exact(n):
    from sparse_coding__amd.engine import probe as pb
    from sparse_coding__amd.engine.sparse_codes import SparseCodes

    sc = C.crafted(n)
    P = C.int_operand(3, n, 1)
    shift = C.int_operand(3, 1, 2)[:, 0].double().contiguous()
    mask = (torch.arange(C.N_EXACT) % 3 != 1).to(torch.uint8)
    bad = SparseCodes(sc.n_rows, sc.n, sc.row_ptr, sc.col.clone(), sc.val)        # rows with a bad column
    lo = sc.row_ptr[0].tolist()
    r1 = int(torch.nonzero(sc.row_ptr[1, 1:] > sc.row_ptr[1, :-1])[0])             # a row of model 1 with entries
    bad.col[0, lo[5] + 64], bad.col[0, lo[3]], bad.col[1, sc.row_ptr[1, r1]] = n, -1, 2 ** 31 - 1
    cases = [(sc, None, None, None), (sc, shift, mask, None), (sc, shift, None, C.NACTIVE[n]), (bad, None, mask, None)]
    for codes, c, w, live in cases:
        want, skipped = pb.rows_matmul_reference(codes, P, c, w, live)
        assert float(want.abs().max()) < 2 ** 24                                 # exact in fp32 too
        for waves in WAVES:
            Q, sk = _rows(codes, P, c, w, live, waves)
            assert torch.equal(_bits(Q), _bits(want.float())), waves
            assert torch.equal(sk, skipped)
    assert skipped.tolist() == [2, 1, 0]
    assert bool((Q[0, 5] == 0).all()) and bool((Q[0, 3] == 0).all()) and bool((Q[1, r1] == 0).all())   # zeros
    _, sk = _rows(sc, P, None, None, C.NACTIVE[n])
    assert sk.tolist()[:2] == [0, 0] and sk[2] > 0


@pytest.mark.parametrize("n", [70, 130])
def test_lists_matmul_exact(n):
    from sparse_coding__amd.engine import probe as pb
    from sparse_coding__amd.engine.feature_codes import FeatureCodes, feature_codes_reference

    R = C.int_operand(3, C.N_EXACT, 3)
    plain = feature_codes_reference(C.crafted(n))
    assert (plain.col_ptr[1, 1:9] - plain.col_ptr[1, :8]).tolist() == list(C.LIST_LENS)
    masked = feature_codes_reference(C.crafted(n), C.NACTIVE[n])
    assert int(masked.col_ptr[2, -1]) == int(masked.col_ptr[2, C.NACTIVE[n][2]]) and int(masked.skipped[2]) > 0
    stray = FeatureCodes(plain.n_rows, n, plain.col_ptr, plain.row.clone(), plain.val, plain.skipped)
    at = plain.col_ptr[1].tolist()
    for pos, r in ((at[7], C.N_EXACT), (at[7] + 64, -1), (at[7] + 65, 2 ** 31 - 1), (at[3] + 63, -2 ** 31)):
        stray.row[1, pos] = r                                                    # rows outside [0, N): skipped
    for fc in (plain, masked, stray):
        want = pb.lists_matmul_reference(fc.col_ptr, fc.row, fc.val, R)
        assert float(want.abs().max()) < 2 ** 24
        for segment in (None, 64):
            for waves in WAVES:
                S = _lists(fc, R, segment, waves)
                assert torch.equal(_bits(S), _bits(want.float())), (segment, waves)
    assert bool((S[1, 0] == 0).all())                                            # an empty list writes zeros


def test_lists_matmul_cuts_long_lists_at_probe_seg():
    from sparse_coding__amd.engine import probe as pb
    from sparse_coding__amd.engine.feature_codes import feature_codes_reference
    from sparse_coding__amd.engine.sparse_codes import sparse_codes_reference
    from sparse_coding__amd.ops import probe as pr

    seg = pr.PROBE_SEG
    fc = feature_codes_reference(sparse_codes_reference([C.long_lists_dense(seg)]))
    assert (fc.col_ptr[0, 1:] - fc.col_ptr[0, :-1]).tolist() == [seg - 1, seg, seg + 1, 2 * seg + 3, 0, 5]
    R = C.int_operand(1, fc.n_rows, 4)
    want = pb.lists_matmul_reference(fc.col_ptr, fc.row, fc.val, R)
    assert float(want.abs().max()) < 2 ** 24
    for waves in WAVES:
        assert torch.equal(_bits(_lists(fc, R, None, waves)), _bits(want.float())), waves
    assert torch.equal(_bits(_lists(fc, R, 2 ** 20)), _bits(want.float()))       # one segment per list


@pytest.mark.parametrize("M", [1, 1023, 1024, 1025, 2049, 3000])
def test_col_dots_and_axpby_exact(M):
    """The slab boundaries of ``col_dots`` (1024 rows per slab), and the vector update."""
    from sparse_coding__amd.engine import probe as pb
    from sparse_coding__amd.ops import probe as pr

    A, B = C.int_operand(3, M, 5), C.int_operand(3, M, 6)
    dA, dB = A.to(DEV), B.to(DEV)
    for b, db in ((B, dB), (A, dA), (None, None)):
        want = pb.col_dots_reference(A, b)
        for waves in WAVES:
            flat, out = _padded((3, 32), torch.float64)
            assert pr.col_dots(dA, db, out=out, waves=waves) is out
            torch.cuda.synchronize()
            assert _intact(flat, out) and torch.equal(_bits(out.cpu()), _bits(want)), waves
    assert torch.equal(dA.cpu(), A) and torch.equal(dB.cpu(), B)
    a = torch.randint(-3, 4, (3, 32), generator=torch.Generator().manual_seed(M)).double()
    b = torch.randint(-3, 4, (3, 32), generator=torch.Generator().manual_seed(M + 1)).double()
    flat, y = _padded((3, M, 32))
    y.copy_(dB)
    pr.axpby_(y, dA, a.to(DEV), b.to(DEV))
    torch.cuda.synchronize()
    assert _intact(flat, y) and torch.equal(dA.cpu(), A)
    assert torch.equal(y.cpu(), (a.unsqueeze(1) * A.double() + b.unsqueeze(1) * B.double()).float())


# ----------------------------------------------------------------------------- realistic tier
def test_ops_realistic_within_one_rounding_and_the_fp64_accumulation():
    from sparse_coding__amd.engine import probe as pb
    from sparse_coding__amd.engine.feature_codes import feature_codes_reference
    from sparse_coding__amd.engine.sparse_codes import sparse_codes_reference
    from sparse_coding__amd.ops import probe as pr

    G, N, n = 2, 320, 130
    dense = C.random_codes(G, N, n, 0.25, 9)
    dense[1, :, 3] = C.random_codes(1, N, 1, 1.0, 10)[0, :, 0]                    # a list of all rows
    sc = sparse_codes_reference([dense])
    P, R = C.real_operand(G, n, 11), C.real_operand(G, N, 12)
    shift = torch.randn(G, 32, generator=torch.Generator().manual_seed(13), dtype=torch.float64)
    want, _ = pb.rows_matmul_reference(sc, P, shift)
    terms = dense.double() @ P.double().abs() + shift.abs().unsqueeze(1)
    length = (dense != 0).sum(-1, keepdim=True).double() + 1
    Q, _ = _rows(sc, P, shift)
    assert bool(((Q.double() - want).abs() <= C.realistic_bound(want, terms, length)).all())
    fc = feature_codes_reference(sc)
    want = pb.lists_matmul_reference(fc.col_ptr, fc.row, fc.val, R)
    terms = dense.double().transpose(1, 2) @ R.double().abs()
    length = (dense != 0).sum(1).unsqueeze(-1).double() + 4                       # (and the fold of its partials)
    for segment in (None, 64):
        S = _lists(fc, R, segment)
        assert bool(((S.double() - want).abs() <= C.realistic_bound(want, terms, length)).all()), segment
    big = C.real_operand(G, 2500, 14)
    for other in (C.real_operand(G, 2500, 15), big, None):
        got = pr.col_dots(big.to(DEV), None if other is None else other.to(DEV)).cpu()
        want = pb.col_dots_reference(big, other)
        terms = (big.double() * (1.0 if other is None else other.double())).abs().sum(1)
        assert bool(((got - want).abs() <= 2500 * 2.0 ** -52 * terms).all())       # (fp64 out: no fp32 rounding)


# ----------------------------------------------------------------------------- the solver
_SOLVED = {}


def _solved(K):
    """Per K, computed once: the case, its codes on the device, the closed form, the plain fp32 evaluation of the
    recurrence (torch, CPU) and the device route's result."""
    if K not in _SOLVED:
        from sparse_coding__amd.engine import probe as pb
        from sparse_coding__amd.engine.sparse_codes import sparse_codes_reference

        dense, bits, fit = C.solver_case(K)
        sc = sparse_codes_reference([dense])
        wc, bc = pb.ridge_closed_form_reference(dense, bits, 1.0, fit)
        plain = pb.ridge_probes_reference(sc, bits, fit_rows=fit, dtype=torch.float32)
        dev = sc.to(DEV)
        res = dev.ridge_probes(C.flags_of(bits).to(DEV), K, fit_rows=fit.to(DEV))
        torch.cuda.synchronize()
        _SOLVED[K] = (dense, bits, fit, dev, wc, bc, plain, res)
    return _SOLVED[K]


@pytest.mark.parametrize("K", [32, 5])
def test_solver_matches_the_normal_equations(K):
    from sparse_coding__amd.engine import probe as pb

    dense, bits, fit, dev, wc, bc, plain, res = _solved(K)
    assert isinstance(res, pb.LinearProbes) and res.weight.is_cuda and res.weight.dtype == torch.float32
    assert res.weight.shape == (2, 96, K) and res.intercept.shape == (2, K) and res.intercept.dtype == torch.float64
    e32, err = C.rel_weight_error(plain.weight, wc), C.rel_weight_error(res.weight, wc)
    print(f"K={K}: device {err:.3e}, plain fp32 {e32:.3e}, iters {int(res.iters.max())}")
    assert err <= 4 * e32
    assert bool(res.converged.all()) and int(res.iters.max()) < 64 and res.skipped.tolist() == [0, 0]
    assert float((res.intercept.cpu() - bc).abs().max()) <= 4 * max(float((plain.intercept - bc).abs().max()), 1e-7)
    assert not bool(res.auroc().isnan().any()) and float(res.auroc()[0].min()) > 0.9
    assert not bool(res.auroc_heldout().isnan().any()) and float(res.auroc_heldout()[0].min()) > 0.8


@pytest.mark.parametrize("K", [32, 5])
def test_solver_is_frozen_past_the_stop_and_reproducible(K):
    dense, bits, fit, dev, wc, bc, plain, res = _solved(K)
    fl, dfit = C.flags_of(bits).to(DEV), fit.to(DEV)
    C.same_probes(dev.ridge_probes(fl, K, fit_rows=dfit, max_iter=200), res)
    for waves in (4, 1, 2):
        C.same_probes(dev.ridge_probes(fl, K, fit_rows=dfit, waves=waves), res)
    C.same_probes(dev.ridge_probes(bits.to(DEV), fit_rows=dfit, feature_codes=dev.by_feature()), res)


@pytest.mark.parametrize("K", [32, 5])
def test_rank_sums_equal_the_pair_count_on_the_devices_own_scores(K):
    from sparse_coding__amd.engine import probe as pb

    dense, bits, fit, dev, wc, bc, plain, res = _solved(K)
    scores = res.scores(dev)
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.shape == (2, 512, K)
    want = dense.double() @ res.weight.double().cpu() + res.intercept.cpu().unsqueeze(1)
    assert float((scores.cpu() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    host = res.to("cpu")
    for rows, names in ((fit, ("u2_fit", "pos_fit", "cnt_fit", "tp_fit", "tn_fit")),
                        (~fit, ("u2_held", "pos_held", "cnt_held", "tp_held", "tn_held"))):
        for name, b in zip(names, pb.score_auroc_reference(scores.cpu(), bits, rows)):
            assert torch.equal(getattr(host, name), b), name


def test_degenerate_concepts_and_refusals_on_the_device():
    from sparse_coding__amd.engine import probe as pb
    from sparse_coding__amd.engine.sparse_codes import SparseCodes, SparseCodesOverflow

    from sparse_coding__amd.engine.feature_codes import FeatureCodesSkipped
    from sparse_coding__amd.engine.sparse_codes import sparse_codes_reference

    lim = C.NACTIVE[70][2]
    dense = C.crafted_dense(70).clone()
    dense[2, :, lim:] = 0                                                        # a masked model
    sc = sparse_codes_reference([dense])
    gen = torch.Generator().manual_seed(3)
    bits = torch.rand(C.N_EXACT, 3, generator=gen) < 0.4
    bits[:, 1], bits[:, 2] = True, False
    res = sc.to(DEV).ridge_probes(bits.to(DEV), nactive=C.NACTIVE[70]).to("cpu")
    want = pb.ridge_probes_reference(sc, bits, nactive=C.NACTIVE[70])
    for k, sign in ((1, 1.0), (2, -1.0)):
        assert bool((res.weight[:, :, k] == 0).all()) and bool((res.intercept[:, k] == sign).all())
        assert bool(res.converged[:, k].all()) and bool((res.iters[:, k] == 0).all())
        assert bool(res.auroc()[:, k].isnan().all())
    assert bool(res.converged.all()) and res.skipped.tolist() == [0, 0, 0]
    assert bool((res.weight[2, lim:] == 0).all()) and bool((res.weight[2, :lim, 0] != 0).any())
    radius = C.stop_radius(dense, bits[:, :1], None, 1.0, 1e-5)[:, 0]
    gap = (res.weight[:, :, 0].double() - want.weight[:, :, 0]).abs().amax(1)    # (two converged routes)
    assert bool((gap <= 2 * radius + 1e-6).all()), (gap, radius)
    with pytest.raises(FeatureCodesSkipped):                                     # rows that fail the skip rule
        C.crafted(70).to(DEV).ridge_probes(bits.to(DEV), nactive=C.NACTIVE[70])
    short = SparseCodes(sc.n_rows, sc.n, sc.row_ptr, sc.col[:, :100].contiguous(), sc.val[:, :100].contiguous())
    with pytest.raises(SparseCodesOverflow):
        short.to(DEV).ridge_probes(bits.to(DEV))
    with pytest.raises(ValueError, match="tol"):
        sc.to(DEV).ridge_probes(bits.to(DEV), tol=1e-7)


# ----------------------------------------------------------------------------- graph capture
def test_the_ops_are_graph_capturable():
    from sparse_coding__amd.engine.feature_codes import feature_codes_reference
    from sparse_coding__amd.ops import probe as pr

    sc = C.crafted(130)
    dev, fc = sc.to(DEV), feature_codes_reference(sc).to(DEV)
    P, R = C.real_operand(3, 130, 21).to(DEV), C.real_operand(3, C.N_EXACT, 22).to(DEV)
    a = torch.randn(3, 32, device=DEV, dtype=torch.float64)
    y0 = C.real_operand(3, 130, 23).to(DEV)

    def run():
        Q, _ = pr.rows_matmul(dev.row_ptr, dev.col, dev.val, P)
        S = pr.lists_matmul(fc.col_ptr, fc.row, fc.val, R, segment=64)
        y = y0.clone()
        pr.axpby_(y, S, a, a)
        return Q, S, pr.col_dots(Q, Q), pr.col_dots(R), y

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        want = [t.clone() for t in run()]  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = run()
    for t in got:
        t.fill_(MARK)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert torch.equal(_bits(x), _bits(y))


# ----------------------------------------------------------------------------- engines
G_ENG, D_ENG, N_ENG, B_ENG, N_POOL, K_ENG = 2, 256, 128, 128, 512, 5   # (d = 256: the narrowest the engines take)


def _pool(seed=0, scale=1.0):
    """(bf16 pool [512, 256], bool concepts [512, 5], fit rows): the concepts are noisy linear functions of the
    sparse causes of the pool.  ``scale``: the top-k models' atoms are not unit vectors (norm 16 at d = 256), so
    their codes on the unscaled pool reach 14 and CGLS at alpha = 1 needs more than 64 iterations; at 0.1 it
    needs about 30 (the fp64 oracle, on the CPU)."""
    gen = torch.Generator().manual_seed(seed)
    feats = torch.nn.functional.normalize(torch.randn(64, D_ENG, generator=gen), dim=-1)
    causes = torch.relu(torch.randn(N_POOL, 64, generator=gen) - 1.0)
    z = causes @ torch.randn(64, K_ENG, generator=gen) + 0.3 * torch.randn(N_POOL, K_ENG, generator=gen)
    return ((scale * causes @ feats).to(torch.bfloat16).to(DEV), z > z.median(0).values,
            torch.rand(N_POOL, generator=gen) < 0.75)


def _sae_models(sizes=None):
    from sparse_coding__amd.models import signatures as S

    torch.manual_seed(7)
    if sizes is not None:
        return S.FunctionalMaskedSAE, [S.FunctionalMaskedSAE.init(D_ENG, k, N_ENG, 1e-3, device=DEV) for k in sizes]
    return S.FunctionalSAE, [S.FunctionalSAE.init(D_ENG, N_ENG, l1, device=DEV) for l1 in (1e-4, 1e-3)]


def _sae_engine(sig, models, **kw):
    from sparse_coding__amd.engine.fused import FusedSAEEnsemble

    models = [({k: t.clone() for k, t in p.items()}, b) for p, b in models]
    return FusedSAEEnsemble(models, sig, lr=1e-3, batch_size=B_ENG, device=DEV, count_every=1, **kw)


def _check_engine(codes, nactive, res, bits, fit):
    """The solver rule on the engine's own ``encode_sparse`` output: within 4x the error of the plain fp32
    evaluation against the dense normal equations, converged inside the budget, the oracle's counts."""
    from sparse_coding__amd.engine import probe as pb

    host = codes.to("cpu")
    dense, bad = pb._dense_codes(host, nactive, torch.float64)
    assert int(bad.sum()) == 0 and res.skipped.tolist() == [0] * host.n_models
    wc, bc = pb.ridge_closed_form_reference(dense, bits, 1.0, fit)
    plain = pb.ridge_probes_reference(host, bits, fit_rows=fit, nactive=nactive, dtype=torch.float32)
    e32, err = C.rel_weight_error(plain.weight, wc), C.rel_weight_error(res.weight, wc)
    print(f"engine: device {err:.3e}, plain fp32 {e32:.3e}, iters {int(res.iters.max())}")
    assert res.weight.is_cuda and err <= 4 * e32
    assert bool(res.converged.all()) and int(res.iters.max()) < 64
    assert torch.equal(res.pos_fit.cpu(), (bits & fit.unsqueeze(1)).sum(0)) and int(res.cnt_held) == int((~fit).sum())
    want = pb.score_auroc_reference(res.scores(codes).cpu(), bits, ~fit)
    assert torch.equal(res.u2_held.cpu(), want[0]) and torch.equal(res.tp_held.cpu(), want[3])


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_sae_engine_ridge_probes(masked):
    from sparse_coding__amd.engine.sparse_codes import SparseCodesOverflow

    sizes = [64, 128] if masked else None
    eng = _sae_engine(*_sae_models(sizes))
    pool, bits, fit = _pool()
    eng.step_batch(pool[:B_ENG])
    codes = eng.encode_sparse(pool)
    res = eng.ridge_probes(pool, bits.to(DEV), fit_rows=fit.to(DEV))
    torch.cuda.synchronize()
    assert res.weight.shape == (G_ENG, N_ENG, K_ENG) and res.n_rows == N_POOL
    _check_engine(codes, sizes, res, bits, fit)
    if masked:
        assert bool((res.weight[0, 64:] == 0).all()) and bool((res.weight[1, 64:] != 0).any())
    budget = max(1, int(codes.nnz().min()) // N_POOL // 2)
    with pytest.raises(SparseCodesOverflow):
        eng.ridge_probes(pool, bits.to(DEV), budget=budget)


def test_ridge_probes_leave_training_state_alone():
    from test_sparse_codes_gpu import _state_tensors

    sig, models = _sae_models()
    a, b = _sae_engine(sig, models).enable_graph(), _sae_engine(sig, models).enable_graph()
    pool, bits, fit = _pool(1)
    for e in (a, b):
        e.step_batch(pool[:B_ENG])
    graphs = dict(a._graph)
    a.ridge_probes(pool, bits.to(DEV), fit_rows=fit.to(DEV))
    for e in (a, b):
        e.step_batch(pool[B_ENG:2 * B_ENG])
    torch.cuda.synchronize()
    assert set(a._graph) == set(graphs) and all(a._graph[k] is g for k, g in graphs.items())
    assert a.step_count == b.step_count == 2 and a.rows_seen == b.rows_seen
    sa, sb = _state_tensors(a), _state_tensors(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def _topk_models():
    from sparse_coding__amd.models.topk import TopKEncoder

    torch.manual_seed(8)
    return [TopKEncoder.init(D_ENG, N_ENG, k, device=DEV) for k in (8, 32)]


def test_topk_engine_ridge_probes():
    from sparse_coding__amd.engine.topk import FusedTopKEnsemble

    eng = FusedTopKEnsemble(_topk_models(), batch_size=B_ENG, device=DEV, lr=1e-3)
    pool, bits, fit = _pool(2, 0.1)
    codes = eng.encode_sparse(pool)
    res = eng.ridge_probes(pool, bits.to(DEV), fit_rows=fit.to(DEV))
    torch.cuda.synchronize()
    _check_engine(codes, None, res, bits, fit)


def test_trainer_routes_ridge_probes_and_refuses():
    from sparse_coding__amd.engine import probe as pb
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.eval import metrics
    from sparse_coding__amd.models.signatures import FunctionalSAE
    from sparse_coding__amd.models.topk import TopKEncoder

    sig, models = _sae_models()
    pool, bits, fit = _pool(3)
    tr = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV)
    assert tr.kind == "fused-sae"
    res = tr.ridge_probes(pool.cpu(), bits, fit_rows=fit)
    assert isinstance(res, pb.LinearProbes)
    _check_engine(tr.encode_sparse(pool), None, res, bits, fit)
    out = metrics.ensemble_ridge_regression_auroc(tr, pool, bits[:, 0])
    assert out.shape == (G_ENG,) and out.is_cuda and bool(((out > 0.5) & (out <= 1)).all())
    tk = EnsembleTrainer(_topk_models(), TopKEncoder, lr=1e-3, batch_size=B_ENG, device="cuda:0")
    assert tk.kind == "fused-topk"
    small = _pool(3, 0.1)[0]
    _check_engine(tk.encode_sparse(small), None, tk.ridge_probes(small, bits, fit_rows=fit), bits, fit)
    # an eager SAE: the oracle on its torch codes, on the device
    eager = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV, engine="eager")
    assert eager.kind == "eager"
    rows = pool.float()
    got = eager.ridge_probes(rows, bits, fit_rows=fit)
    host = eager.encode_sparse(rows).to("cpu")
    want = pb.ridge_probes_reference(host, bits, fit_rows=fit)
    assert got.weight.is_cuda and got.weight.dtype == torch.float32 and bool(got.converged.all())
    radius = C.stop_radius(pb._dense_codes(host, None, torch.float64)[0], bits, fit, 1.0, 1e-5)
    gap = (got.weight.cpu().double() - want.weight).abs().amax(1)                # (two converged routes)
    assert bool((gap <= 2 * radius + 1e-6).all()), (gap, radius)
    cpu_models = [FunctionalSAE.init(16, 32, 1e-3) for _ in range(2)]
    dp = EnsembleTrainer(cpu_models, FunctionalSAE, batch_size=16, device="cpu", engine="eager", parallel="dp")
    with pytest.raises(NotImplementedError, match="data-parallel"):
        dp.ridge_probes(torch.randn(64, 16), torch.zeros(64, dtype=torch.int32))
    for kind in ("threshold", "reverse"):
        eng = _sae_engine(sig, models)
        eng.kind = kind
        with pytest.raises(NotImplementedError, match=f"ridge_probes: .*{kind}"):
            eng.ridge_probes(pool, bits.to(DEV))
    eng.kind, eng.learned_center = "tied", True
    with pytest.raises(NotImplementedError, match="learned centering"):
        eng.ridge_probes(pool, bits.to(DEV))
