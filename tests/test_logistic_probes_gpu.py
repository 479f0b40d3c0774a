"""Whole-dictionary logistic probes on the MI355X: the logistic kernels of ``csrc/probe.hip`` against their fp64
oracles -- a saturated exact tier (``logistic_probe_cases``: every sum is a sum of integers, so the comparison is
``torch.equal``) and a realistic tier (one fp32 rounding plus the fp64 evaluation and accumulation) -- the Newton-CG
solver against the dense Newton reference, graph capture, and ``logistic_probes`` of the engines and the trainer."""

import pytest
import torch

import logistic_probe_cases as L
import probe_cases as C
from test_probes_gpu import (B_ENG, G_ENG, K_ENG, N_ENG, N_POOL, _bits, _intact, _padded, _pool, _sae_engine,
                             _sae_models, _topk_models)

pytestmark = pytest.mark.gpu

DEV = "cuda"
WAVES = (1, 4, 2, 4)                      # (the last repeats a geometry: a second run, the same bits)
SLAB = 1024


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_coding__amd.ops import _lib as lib_
    from sparse_coding__amd.ops import probe as pr

    lib_.lib()  # must load: no silent fallback on a GPU box
    assert pr.PROBE_SLAB == SLAB and pr.LINE_STEPS == 8
    yield


def _logit(Z, flags, mask, waves):
    from sparse_coding__amd.ops import probe as pr

    G, N = Z.shape[:2]
    (fr, R), (fd, D), (fl, loss) = _padded((G, N, 32)), _padded((G, N, 32)), _padded((G, 32), torch.float64)
    dZ, dfl, dm = Z.to(DEV), flags.to(DEV), mask.to(DEV)
    out = pr.logit_terms(dZ, dfl, dm, out=(R, D, loss), waves=waves)
    torch.cuda.synchronize()
    assert out[0] is R and out[1] is D and out[2] is loss
    assert _intact(fr, R) and _intact(fd, D) and _intact(fl, loss)
    assert torch.equal(dZ.cpu(), Z) and torch.equal(dfl.cpu(), flags) and torch.equal(dm.cpu(), mask)
    return R.cpu(), D.cpu(), loss.cpu()


def _line(Z, U, flags, mask, waves):
    from sparse_coding__amd.ops import probe as pr

    flat, out = _padded((Z.shape[0], 8, 32), torch.float64)
    dZ, dU = Z.to(DEV), U.to(DEV)
    assert pr.line_losses(dZ, dU, flags.to(DEV), mask.to(DEV), out=out, waves=waves) is out
    torch.cuda.synchronize()
    assert _intact(flat, out) and torch.equal(dZ.cpu(), Z) and torch.equal(dU.cpu(), U)
    return out.cpu()


# ----------------------------------------------------------------------------- saturated exact tier
@pytest.mark.parametrize("G,N,K,slab", [(3, 192, 32, 0), (3, 192, 5, 0), (1, SLAB - 1, 5, 0), (1, SLAB, 32, 0),
                                        (1, SLAB + 1, 5, 0), (1, 2 * SLAB + 3, 7, SLAB)])
def test_logit_terms_and_line_losses_saturated_exact(G, N, K, slab):
    from sparse_coding__amd.engine import probe as pb

    Z, U, flags, mask = L.saturated(G, N, K, 40 + N + K, slab)
    if slab:
        assert not bool(mask[slab:2 * slab].any()) and bool(mask[2 * slab:].any())          # a slab of nothing
    wr, wd, wl = pb.logit_terms_reference(Z, flags, mask)
    wj = pb.line_losses_reference(Z, U, flags, mask)
    fit = (mask != 0)
    exact = [k for k in range(K) if k != L.ZERO_COL]
    assert bool((wl[:, exact] == wl[:, exact].round()).all()) and float(wj.abs().max()) < 2 ** 53
    zero_rows = (Z[..., L.ZERO_COL] == 0) & fit
    assert bool(zero_rows.any()) and bool((wd[..., L.ZERO_COL][zero_rows] == 0.25).all())
    assert bool((wr[..., L.ZERO_COL][zero_rows].abs() == 0.5).all())
    soft = [k for k in range(32) if k not in exact]                     # columns with z = 0 rows: log 2 terms
    nfit = float(fit.sum())
    first = None
    for waves in WAVES:
        R, D, loss = _logit(Z, flags, mask, waves)
        assert torch.equal(R, wr.float()) and torch.equal(D, wd.float()), waves
        assert bool((R[:, ~fit] == 0).all()) and bool((D[:, ~fit] == 0).all())
        assert torch.equal(loss[:, exact], wl[:, exact]), waves
        bound = L.sum_bound(L.loss_abs_terms(Z.double(), mask), nfit)
        assert bool(((loss - wl).abs()[:, soft] <= bound[:, soft]).all())
        line = _line(Z, U, flags, mask, waves)
        assert torch.equal(line[:, :, exact], wj[:, :, exact]), waves
        bound = L.sum_bound(L.loss_abs_terms(Z.double().abs() + U.double().abs(), mask), nfit).unsqueeze(1)
        assert bool(((line - wj).abs()[:, :, soft] <= bound[:, :, soft]).all())
        if first is None:
            first = (R, D, loss, line)
        for a, b in zip(first, (R, D, loss, line)):                      # every geometry, and twice: the same bits
            assert torch.equal(_bits(a), _bits(b)), waves


# ----------------------------------------------------------------------------- rows_scaled exact tier
@pytest.mark.parametrize("n", [70, 130])
def test_rows_matmul_scaled_exact(n):
    from sparse_coding__amd.engine import probe as pb
    from sparse_coding__amd.engine.sparse_codes import SparseCodes
    from sparse_coding__amd.ops import probe as pr

    sc = C.crafted(n)
    P = C.int_operand(3, n, 1)
    shift = C.int_operand(3, 1, 2)[:, 0].double().contiguous()
    mask = (torch.arange(C.N_EXACT) % 3 != 1).to(torch.uint8)
    D = torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (3, C.N_EXACT, 32),
                                                          generator=torch.Generator().manual_seed(n))]
    bad = SparseCodes(sc.n_rows, sc.n, sc.row_ptr, sc.col.clone(), sc.val)        # rows with a bad column
    lo = sc.row_ptr[0].tolist()
    bad.col[0, lo[5] + 64], bad.col[0, lo[3]] = n, -1
    cases = [(sc, None, None, None), (sc, shift, mask, None), (sc, shift, None, C.NACTIVE[n]), (bad, None, mask, None)]
    for codes, c, w, live in cases:
        plain, skipped = pb.rows_matmul_reference(codes, P, c, w, live)
        want = plain * D.double()
        assert float(plain.abs().max()) < 2 ** 16                                # exact in fp32 with the quarter too
        dev = codes.to(DEV)
        args = [None if t is None else t.to(DEV) for t in (P, c, w, D)]
        nact = None if live is None else torch.tensor(live, dtype=torch.int32, device=DEV)
        for waves in WAVES:
            flat, Q = _padded((3, C.N_EXACT, 32))
            out, sk = pr.rows_matmul(dev.row_ptr, dev.col, dev.val, args[0], shift=args[1], mask=args[2],
                                     nactive=nact, out=Q, waves=waves, scale=args[3])
            old, sk0 = pr.rows_matmul(dev.row_ptr, dev.col, dev.val, args[0], shift=args[1], mask=args[2],
                                      nactive=nact, waves=waves)
            torch.cuda.synchronize()
            assert out is Q and _intact(flat, Q) and torch.equal(args[3].cpu(), D)
            assert torch.equal(Q.cpu(), want.float()), waves
            assert torch.equal(_bits(old.cpu()), _bits(plain.float())), waves    # the unscaled entry: its old bits
            assert torch.equal(sk.cpu(), skipped) and torch.equal(sk0.cpu(), skipped)
    assert skipped.tolist() == [2, 0, 0]
    with pytest.raises(ValueError, match="scale"):
        pr.rows_matmul(dev.row_ptr, dev.col, dev.val, args[0], scale=args[3][:, :5].contiguous())
    with pytest.raises(ValueError, match="different buffers"):
        pr.rows_matmul(dev.row_ptr, dev.col, dev.val, args[0], scale=args[3], out=args[3])


# ----------------------------------------------------------------------------- realistic tier
def test_logistic_ops_realistic_within_one_rounding_and_the_fp64_evaluation():
    from sparse_coding__amd.engine import probe as pb

    G, N = 2, SLAB + 300
    Z, U, flags, mask = L.realistic(G, N, 51)
    wr, wd, wl = pb.logit_terms_reference(Z, flags, mask)
    R, D, loss = _logit(Z, flags, mask, 4)
    er, ed = (R.double() - wr).abs(), (D.double() - wd).abs()
    print(f"r: worst {float((er / wr.abs().clamp(min=1e-300)).max()):.3e} relative, D: "
          f"{float((ed / wd.abs().clamp(min=1e-300)).max()):.3e} (one fp32 rounding: {2.0 ** -24:.3e})")
    assert bool((er <= L.elem_bound(wr)).all()) and bool((ed <= L.elem_bound(wd)).all())
    nfit = float((mask != 0).sum())
    terms = L.loss_abs_terms(Z.double(), mask)
    print(f"loss: worst {float(((loss - wl).abs() / terms).max() / L.ULP64):.2f} ulp of the terms, allowed "
          f"{nfit + L.EVAL_ULPS:.0f}")
    assert bool(((loss - wl).abs() <= L.sum_bound(terms, nfit)).all())
    wj = pb.line_losses_reference(Z, U, flags, mask)
    line = _line(Z, U, flags, mask, 4)
    terms = L.loss_abs_terms(Z.double().abs() + U.double().abs(), mask).unsqueeze(1)
    assert bool(((line - wj).abs() <= L.sum_bound(terms, nfit)).all())
    still = _line(Z, torch.zeros_like(U), flags, mask, 4)                     # no step: the loss itself, to the bit,
    for j in range(8):                                                        # which the Armijo test relies on
        assert torch.equal(_bits(still[:, j].contiguous()), _bits(loss)), j
    from sparse_coding__amd.ops import probe as pr

    for bad in (dict(Z=Z[:, :, :31].contiguous()), dict(flags=flags.long()), dict(mask=mask.bool())):
        kw = {k: v.to(DEV) for k, v in {**dict(Z=Z, flags=flags, mask=mask), **bad}.items()}
        with pytest.raises(ValueError):
            pr.logit_terms(kw["Z"], kw["flags"], kw["mask"])


# ----------------------------------------------------------------------------- the solver
_SOLVED = {}


def _solved():
    """Computed once: ``solver_case(5)``, its codes on the device, the Newton reference, the plain fp32 evaluation
    of the recurrence (torch, CPU) and the device route's result."""
    if not _SOLVED:
        from sparse_coding__amd.engine import probe as pb
        from sparse_coding__amd.engine.sparse_codes import sparse_codes_reference

        dense, bits, fit = C.solver_case(5)
        sc = sparse_codes_reference([dense])
        wn, bn = L.newton(5)
        plain = pb.logistic_probes_reference(sc, bits, fit_rows=fit, dtype=torch.float32)
        dev = sc.to(DEV)
        res = dev.logistic_probes(C.flags_of(bits).to(DEV), 5, fit_rows=fit.to(DEV))
        torch.cuda.synchronize()
        _SOLVED["x"] = (dense, bits, fit, dev, wn, bn, plain, res)
    return _SOLVED["x"]


def test_solver_matches_the_newton_reference():
    from sparse_coding__amd.engine import probe as pb

    dense, bits, fit, dev, wn, bn, plain, res = _solved()
    assert isinstance(res, pb.LogisticProbes) and res.weight.is_cuda and res.weight.dtype == torch.float32
    assert res.weight.shape == (2, 96, 5) and res.intercept.shape == (2, 5) and res.intercept.dtype == torch.float64
    e32, err = C.rel_weight_error(plain.weight, wn), C.rel_weight_error(res.weight, wn)
    print(f"device {err:.3e}, plain fp32 {e32:.3e}, outer {int(res.iters.max())}, CG {int(res.cg_iters.max())}")
    assert err <= 4 * e32
    assert bool(res.converged.all()) and not bool(res.stalled.any()) and int(res.iters.max()) < 12
    assert res.skipped.tolist() == [0, 0] and float(res.resid.max()) <= 1e-4
    assert float((res.intercept.cpu() - bn).abs().max()) <= 4 * max(float((plain.intercept - bn).abs().max()), 1e-7)
    f, _, _ = L.objective(dense, bits, fit, 1.0, res.weight.cpu(), res.intercept.cpu())
    assert float((f - res.loss.cpu()).abs().max()) <= 1e-5 * float(f.abs().max())
    assert not bool(res.auroc().isnan().any()) and float(res.auroc()[0].min()) > 0.9
    assert not bool(res.auroc_heldout().isnan().any()) and float(res.auroc_heldout()[0].min()) > 0.8


def test_solver_is_frozen_past_the_stop_and_reproducible():
    dense, bits, fit, dev, wn, bn, plain, res = _solved()
    fl, dfit = C.flags_of(bits).to(DEV), fit.to(DEV)
    assert int(res.iters.max()) < 12                                             # (every step past it is frozen)
    L.same_probes(dev.logistic_probes(fl, 5, fit_rows=dfit), res)                # a second run
    for max_iter in (12, 40):                                                    # without early_stop: 5 / 33 frozen
        for early_stop in (True, False):                                         # steps run on the kernels
            L.same_probes(dev.logistic_probes(fl, 5, fit_rows=dfit, max_iter=max_iter, early_stop=early_stop), res)
    for waves in (1, 2):
        L.same_probes(dev.logistic_probes(fl, 5, fit_rows=dfit, waves=waves), res)
    L.same_probes(dev.logistic_probes(bits.to(DEV), fit_rows=dfit, feature_codes=dev.by_feature()), res)


def test_rank_sums_equal_the_pair_count_on_the_devices_own_logits():
    from sparse_coding__amd.engine import probe as pb

    dense, bits, fit, dev, wn, bn, plain, res = _solved()
    scores = res.scores(dev)
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.shape == (2, 512, 5)
    want = dense.double() @ res.weight.double().cpu() + res.intercept.cpu().unsqueeze(1)
    assert float((scores.cpu() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    assert torch.equal(res.predict_proba(dev), torch.sigmoid(scores))
    host = res.to("cpu")
    for rows, names in ((fit, ("u2_fit", "pos_fit", "cnt_fit", "tp_fit", "tn_fit")),
                        (~fit, ("u2_held", "pos_held", "cnt_held", "tp_held", "tn_held"))):
        for name, b in zip(names, pb.score_auroc_reference(scores.cpu(), bits, rows)):
            assert torch.equal(getattr(host, name), b), name


def test_the_loop_without_early_stop_is_graph_capturable():
    from sparse_coding__amd.engine import probe as pb
    from sparse_coding__amd.engine.value_order import concept_words

    dense, bits, fit, dev, wn, bn, plain, res = _solved()
    dbits, dfit = bits.to(DEV), fit.to(DEV)
    ops = pb._KernelLogitOps(dev, dev.by_feature().check(), dfit, None, None, concept_words(dbits))
    pos = pb._pad((dbits & dfit.unsqueeze(1)).sum(0))

    def run():
        w, b, it, cg, conv, stalled, resid, f = pb._newton_cg(ops, 96, pos, 1.0, 12, 16, 1e-4, early_stop=False)
        return w, b - ops.mu_dot(w), it, cg, conv, stalled, resid, f

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        want = [t.clone() for t in run()]  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = run()
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert torch.equal(x, y) and x.dtype == y.dtype
    assert torch.equal(got[0][..., :5], res.weight) and torch.equal(got[1][:, :5], res.intercept)
    assert torch.equal(got[2][:, :5], res.iters) and torch.equal(got[7][:, :5], res.loss)
    long = pb._newton_cg(ops, 96, pos, 1.0, 40, 16, 1e-4, early_stop=False)       # (uncaptured) 40 steps: the same bits
    for x, y in zip((long[0], long[2], long[3], long[7]), (want[0], want[2], want[3], want[7])):
        assert torch.equal(x, y)


def test_degenerate_concepts_and_refusals_on_the_device():
    from sparse_coding__amd.engine import probe as pb
    from sparse_coding__amd.engine.feature_codes import FeatureCodesSkipped
    from sparse_coding__amd.engine.sparse_codes import SparseCodes, SparseCodesOverflow, sparse_codes_reference

    lim = C.NACTIVE[70][2]
    dense = C.crafted_dense(70).clone()
    dense[2, :, lim:] = 0                                                        # a masked model
    sc = sparse_codes_reference([dense])
    gen = torch.Generator().manual_seed(3)
    bits = torch.rand(C.N_EXACT, 4, generator=gen) < 0.4
    bits[:, 1], bits[:, 2] = True, False
    bits[:, 3] = False
    bits[17, 3] = True                                                           # a single positive
    res = sc.to(DEV).logistic_probes(bits.to(DEV), nactive=C.NACTIVE[70]).to("cpu")
    clip = float(torch.log(torch.tensor(2.0 * C.N_EXACT, dtype=torch.float64)))
    for k, sign in ((1, 1.0), (2, -1.0)):
        assert bool((res.weight[:, :, k] == 0).all()) and bool((res.intercept[:, k] == sign * clip).all())
        assert bool(res.converged[:, k].all()) and bool((res.iters[:, k] == 0).all())
        assert bool(res.auroc()[:, k].isnan().all())
    assert bool(res.converged.all()) and not bool(res.stalled.any()) and res.skipped.tolist() == [0, 0, 0]
    assert bool((res.weight[2, lim:] == 0).all()) and bool((res.weight[2, :lim, 0] != 0).any())
    wn, bn = pb.logistic_newton_reference(dense, bits, 1.0)
    live = [0, 3]
    radius = (L.stop_radius(dense, bits, None, 1.0, 1e-4) + L.distance_bound(dense, bits, None, 1.0, wn, bn))[:, live]
    gap = L.weight_gap(res.weight, wn)[:, live]
    assert bool((gap <= radius + 1e-5).all()), (gap, radius)                     # (+ the fp32 weights' own rounding)
    with pytest.raises(FeatureCodesSkipped):                                     # rows that fail the skip rule
        C.crafted(70).to(DEV).logistic_probes(bits.to(DEV), nactive=C.NACTIVE[70])
    short = SparseCodes(sc.n_rows, sc.n, sc.row_ptr, sc.col[:, :100].contiguous(), sc.val[:, :100].contiguous())
    with pytest.raises(SparseCodesOverflow):
        short.to(DEV).logistic_probes(bits.to(DEV))
    for bad, word in (({"tol": 9e-6}, "tol"), ({"C": 0.0}, "C must"), ({"C": float("inf")}, "C must")):
        with pytest.raises(ValueError, match=word):
            sc.to(DEV).logistic_probes(bits.to(DEV), **bad)


# ----------------------------------------------------------------------------- engines
def _check_engine(codes, nactive, res, bits, fit, **kw):
    """The solver rule on the engine's own ``encode_sparse`` output: within 4x the error of the plain fp32
    evaluation against the dense Newton reference, converged inside the budget, the oracle's counts."""
    from sparse_coding__amd.engine import probe as pb

    host = codes.to("cpu")
    dense, bad = pb._dense_codes(host, nactive, torch.float64)
    assert int(bad.sum()) == 0 and res.skipped.tolist() == [0] * host.n_models
    wn, bn = pb.logistic_newton_reference(dense, bits, 1.0, fit)
    plain = pb.logistic_probes_reference(host, bits, fit_rows=fit, nactive=nactive, dtype=torch.float32, **kw)
    e32, err = C.rel_weight_error(plain.weight, wn), C.rel_weight_error(res.weight, wn)
    print(f"engine: device {err:.3e}, plain fp32 {e32:.3e}, outer {int(res.iters.max())}, CG {int(res.cg_iters.max())}")
    assert res.weight.is_cuda and err <= 4 * e32
    assert bool(res.converged.all()) and not bool(res.stalled.any()) and int(res.iters.max()) < 12   # the defaults
    assert torch.equal(res.pos_fit.cpu(), (bits & fit.unsqueeze(1)).sum(0)) and int(res.cnt_held) == int((~fit).sum())
    want = pb.score_auroc_reference(res.scores(codes).cpu(), bits, ~fit)
    assert torch.equal(res.u2_held.cpu(), want[0]) and torch.equal(res.tp_held.cpu(), want[3])


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_sae_engine_logistic_probes(masked):
    from sparse_coding__amd.engine.sparse_codes import SparseCodesOverflow

    sizes = [64, 128] if masked else None
    eng = _sae_engine(*_sae_models(sizes))
    pool, bits, fit = _pool()
    eng.step_batch(pool[:B_ENG])
    codes = eng.encode_sparse(pool)
    res = eng.logistic_probes(pool, bits.to(DEV), fit_rows=fit.to(DEV))
    torch.cuda.synchronize()
    assert res.weight.shape == (G_ENG, N_ENG, K_ENG) and res.n_rows == N_POOL
    _check_engine(codes, sizes, res, bits, fit)
    if masked:
        assert bool((res.weight[0, 64:] == 0).all()) and bool((res.weight[1, 64:] != 0).any())
    budget = max(1, int(codes.nnz().min()) // N_POOL // 2)
    with pytest.raises(SparseCodesOverflow):
        eng.logistic_probes(pool, bits.to(DEV), budget=budget)


def test_logistic_probes_leave_training_state_alone():
    from test_sparse_codes_gpu import _state_tensors

    sig, models = _sae_models()
    a, b = _sae_engine(sig, models).enable_graph(), _sae_engine(sig, models).enable_graph()
    pool, bits, fit = _pool(1)
    for e in (a, b):
        e.step_batch(pool[:B_ENG])
    graphs = dict(a._graph)
    a.logistic_probes(pool, bits.to(DEV), fit_rows=fit.to(DEV))
    for e in (a, b):
        e.step_batch(pool[B_ENG:2 * B_ENG])
    torch.cuda.synchronize()
    assert set(a._graph) == set(graphs) and all(a._graph[k] is g for k, g in graphs.items())
    assert a.step_count == b.step_count == 2 and a.rows_seen == b.rows_seen
    sa, sb = _state_tensors(a), _state_tensors(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_topk_engine_logistic_probes():
    from sparse_coding__amd.engine.topk import FusedTopKEnsemble

    eng = FusedTopKEnsemble(_topk_models(), batch_size=B_ENG, device=DEV, lr=1e-3)
    pool, bits, fit = _pool(2, 0.1)
    codes = eng.encode_sparse(pool)
    res = eng.logistic_probes(pool, bits.to(DEV), fit_rows=fit.to(DEV))
    torch.cuda.synchronize()
    _check_engine(codes, None, res, bits, fit)


def test_trainer_routes_logistic_probes_and_refuses():
    from sparse_coding__amd.engine import probe as pb
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.eval import metrics
    from sparse_coding__amd.models.signatures import FunctionalSAE
    from sparse_coding__amd.models.topk import TopKEncoder

    sig, models = _sae_models()
    pool, bits, fit = _pool(3)
    tr = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV)
    assert tr.kind == "fused-sae"
    res = tr.logistic_probes(pool.cpu(), bits, fit_rows=fit)
    assert isinstance(res, pb.LogisticProbes)
    _check_engine(tr.encode_sparse(pool), None, res, bits, fit)
    out = metrics.ensemble_logistic_regression_auroc(tr, pool, bits[:, 0])
    assert out.shape == (G_ENG,) and out.is_cuda and bool(((out > 0.5) & (out <= 1)).all())
    tk = EnsembleTrainer(_topk_models(), TopKEncoder, lr=1e-3, batch_size=B_ENG, device="cuda:0")
    assert tk.kind == "fused-topk"
    small = _pool(3, 0.1)[0]
    _check_engine(tk.encode_sparse(small), None, tk.logistic_probes(small, bits, fit_rows=fit), bits, fit)
    # an eager SAE: the oracle on its torch codes, on the device
    eager = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV, engine="eager")
    assert eager.kind == "eager"
    rows = pool.float()
    got = eager.logistic_probes(rows, bits, fit_rows=fit)
    host = eager.encode_sparse(rows).to("cpu")
    want = pb.logistic_probes_reference(host, bits, fit_rows=fit)
    assert got.weight.is_cuda and got.weight.dtype == torch.float32 and bool(got.converged.all())
    radius = L.stop_radius(pb._dense_codes(host, None, torch.float64)[0], bits, fit, 1.0, 1e-4)
    gap = L.weight_gap(got.weight, want.weight)                                  # (two converged routes)
    assert bool((gap <= 2 * radius + 1e-6).all()), (gap, radius)
    cpu_models = [FunctionalSAE.init(16, 32, 1e-3) for _ in range(2)]
    for parallel in ("dp", "zero1"):
        dp = EnsembleTrainer(cpu_models, FunctionalSAE, batch_size=16, device="cpu", engine="eager", parallel=parallel)
        with pytest.raises(NotImplementedError, match="data-parallel"):
            dp.logistic_probes(torch.randn(64, 16), torch.zeros(64, dtype=torch.int32))
    for kind in ("threshold", "reverse"):
        eng = _sae_engine(sig, models)
        eng.kind = kind
        with pytest.raises(NotImplementedError, match=f"logistic_probes: .*{kind}"):
            eng.logistic_probes(pool, bits.to(DEV))
    eng.kind, eng.learned_center = "tied", True
    with pytest.raises(NotImplementedError, match="learned centering"):
        eng.logistic_probes(pool, bits.to(DEV))
