"""Whole-dictionary ridge probes without a GPU: the fp64 oracle of ``engine/probe.py`` against the dense normal
equations and against scikit-learn, the freeze rule, degenerate concepts, the exact AUROC integers against a
brute-force pair count, planted errors, the segment table of ``ops.probe.lists_plan``, the result type and the
surfaces."""

import math

import pytest
import torch

import probe_cases as C

from sparse_coding__amd.engine import probe as pb
from sparse_coding__amd.engine.sparse_codes import sparse_codes_reference

TIGHT = dict(max_iter=600, tol=1e-12)


def _closed_gap(dense, bits, fit, alpha, w, resid):
    """(max |w - w_closed|, its bound): the iterate's gradient is ``s = A (w* - w)`` with ``A = Xc^T Xc + alpha I >=
    alpha I``, so ``|w - w*|_2 <= |s| / alpha = resid sqrt(gamma0) / alpha``; 1e-11 relative covers fp64 rounding
    of both sides."""
    wc, bc = pb.ridge_closed_form_reference(dense, bits, alpha, fit)
    X = dense.double() if fit is None else dense.double()[:, fit]
    y = (bits.double() * 2 - 1) if fit is None else (bits.double() * 2 - 1)[fit]
    g0 = ((X - X.mean(1, keepdim=True)).transpose(1, 2) @ (y - y.mean(0))).pow(2).sum(1)        # [G, K]
    bound = resid * g0.sqrt() / alpha + 1e-11 * wc.abs().amax(1)
    return (w.double() - wc).abs().amax(1), bound, wc, bc


@pytest.mark.parametrize("K", [32, 5])
@pytest.mark.parametrize("held", [False, True], ids=["all-rows", "fit-rows"])
def test_oracle_matches_the_normal_equations(K, held):
    dense, bits, fit = C.solver_case(K)
    fit = fit if held else None
    sc = sparse_codes_reference([dense])
    res = pb.ridge_probes_reference(sc, bits, alpha=1.0, fit_rows=fit, **TIGHT)
    assert res.weight.dtype == torch.float64 and res.weight.shape == (2, 96, K)
    assert bool(res.converged.all()) and int(res.iters.max()) < TIGHT["max_iter"] and float(res.resid.max()) <= 1e-12
    gap, bound, wc, bc = _closed_gap(dense, bits, fit, 1.0, res.weight, res.resid)
    assert bool((gap <= bound).all()), (gap.max(), bound.min())
    assert float((res.intercept - bc).abs().max()) <= 96 * float(bound.max())     # |mu . (w - w*)| <= n max|mu| gap
    # the default tolerance: converged well inside the iteration budget, and close
    dflt = pb.ridge_probes_reference(sc, C.flags_of(bits), K, alpha=1.0, fit_rows=fit)
    assert bool(dflt.converged.all()) and int(dflt.iters.max()) < 64
    gap, bound, _, _ = _closed_gap(dense, bits, fit, 1.0, dflt.weight, dflt.resid)
    assert bool((gap <= bound).all())
    if held:
        a, h = res.auroc(), res.auroc_heldout()
        assert not bool(h.isnan().any()) and bool((a >= h - 0.05).all())
        assert float(h[0].min()) > 0.8 and float(h[1].max()) < 0.7   # the concepts are functions of model 0's code
    else:
        assert bool(res.auroc_heldout().isnan().all()) and int(res.cnt_held) == 0


def test_closed_form_and_oracle_match_sklearn():
    sk = pytest.importorskip("sklearn.linear_model")
    from sklearn.metrics import roc_auc_score

    dense, bits, fit = C.solver_case(5)
    sc = sparse_codes_reference([dense])
    for alpha, rows in ((1.0, None), (0.25, fit)):
        wc, bc = pb.ridge_closed_form_reference(dense, bits, alpha, rows)
        res = pb.ridge_probes_reference(sc, bits, alpha=alpha, fit_rows=rows, **TIGHT)
        sel = slice(None) if rows is None else rows
        for g in range(2):
            X = dense[g].double().numpy()
            for k in range(5):
                y = bits[:, k].numpy()
                clf = sk.RidgeClassifier(alpha=alpha).fit(X[sel], y[sel])
                coef = torch.from_numpy(clf.coef_).reshape(-1)
                icpt = float(torch.as_tensor(clf.intercept_).reshape(-1)[0])
                assert float((coef - wc[g, :, k]).abs().max()) <= 1e-12
                assert abs(icpt - float(bc[g, k])) <= 1e-12
                dec = torch.from_numpy(clf.decision_function(X))
                assert float((dec - (dense[g].double() @ wc[g, :, k] + bc[g, k])).abs().max()) <= 1e-12
                # the reference's number: the AUROC of the hard predictions, and the exact AUROC of the scores
                want = roc_auc_score(y[sel], clf.predict(X[sel]))
                assert res.auroc_predicted()[g, k].item() == pytest.approx(want, abs=1e-15)
                assert res.auroc()[g, k].item() == pytest.approx(roc_auc_score(y[sel], dec.numpy()[sel]), abs=1e-12)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_a_finished_concept_is_frozen(dtype):
    dense, bits, fit = C.solver_case(32)
    sc = sparse_codes_reference([dense])
    a = pb.ridge_probes_reference(sc, bits, fit_rows=fit, max_iter=64, dtype=dtype)
    b = pb.ridge_probes_reference(sc, bits, fit_rows=fit, max_iter=200, dtype=dtype)
    assert bool(a.converged.all()) and int(a.iters.max()) < 64
    C.same_probes(a, b)
    few = pb.ridge_probes_reference(sc, bits, fit_rows=fit, max_iter=3, dtype=dtype)
    assert not bool(few.converged.any()) and bool((few.iters == 3).all())


def test_degenerate_concepts_and_masked_widths():
    from sparse_coding__amd.engine.feature_codes import FeatureCodesSkipped

    lim = C.NACTIVE[70][2]
    dense = C.crafted_dense(70).clone()
    dense[2, :, lim:] = 0                                            # a masked model: nothing at or past its width
    sc = sparse_codes_reference([dense])
    gen = torch.Generator().manual_seed(3)
    bits = torch.rand(C.N_EXACT, 4, generator=gen) < 0.4
    bits[:, 1], bits[:, 2] = True, False
    fit = torch.rand(C.N_EXACT, generator=gen) < 0.8
    bits[fit, 3] = True                                              # constant on the fit rows only
    res = pb.ridge_probes_reference(sc, bits, fit_rows=fit, nactive=C.NACTIVE[70])
    for k, sign in ((1, 1.0), (2, -1.0), (3, 1.0)):
        assert bool((res.weight[:, :, k] == 0).all()) and bool((res.intercept[:, k] == sign).all())
        assert bool(res.converged[:, k].all()) and bool((res.iters[:, k] == 0).all())
        assert bool((res.resid[:, k] == 0).all()) and bool(res.auroc()[:, k].isnan().all())
    assert not bool(res.auroc()[:, 0].isnan().any()) and bool(res.converged.all())
    # the masked model: the features at or past its width weigh nothing
    assert res.skipped.tolist() == [0, 0, 0]
    assert bool((res.weight[2, lim:] == 0).all()) and bool((res.weight[2, :lim, 0] != 0).any())
    wc, bc = pb.ridge_closed_form_reference(dense, bits[:, :1], 1.0, fit)
    tight = pb.ridge_probes_reference(sc, bits[:, :1], fit_rows=fit, nactive=C.NACTIVE[70], **TIGHT)
    assert float((tight.weight - wc).abs().max()) <= 1e-9 and float((tight.intercept - bc).abs().max()) <= 1e-9
    # a row with a column at or past the width fails the skip rule: the fit refuses it, a scoring pass gives it 0
    wide = C.crafted(70)
    out = (C.crafted_dense(70)[2][:, lim:] != 0).any(1)
    with pytest.raises(FeatureCodesSkipped, match=f"{int(out.sum())}"):
        pb.ridge_probes_reference(wide, bits, fit_rows=fit, nactive=C.NACTIVE[70])
    scores = tight.scores(wide, C.NACTIVE[70])
    assert scores.dtype == torch.float32 and bool((scores[2][out] == 0).all()) and bool((scores[2][~out] != 0).all())
    with pytest.raises(ValueError, match="tol"):
        pb.ridge_probes_reference(sc, bits, tol=1e-7, dtype=torch.float32)
    with pytest.raises(ValueError, match="tol"):
        pb.check_solver(1.0, 64, 9e-7)
    with pytest.raises(ValueError, match="fit_rows"):
        pb.ridge_probes_reference(sc, bits, fit_rows=torch.ones(5, dtype=torch.bool))


def test_score_auroc_integers_match_the_pair_count():
    gen = torch.Generator().manual_seed(11)
    N, K = 160, 6
    scores = torch.randn(2, N, K, generator=gen)
    scores[:, :, 1] = scores[:, :, 1].round()                        # many ties
    scores[:, :, 2] = 0.25                                           # one tie run
    scores[0, ::3, 3], scores[0, 1::3, 3] = 0.0, -0.0                # -0.0 ties with +0.0
    scores[1, :, 4] = scores[1, :, 4].round(decimals=1)
    bits = torch.rand(N, K, generator=gen) < torch.linspace(0.1, 0.6, K)
    bits[:, 5] = False
    rows = torch.rand(N, generator=gen) < 0.6
    for sel in (rows, ~rows, torch.ones(N, dtype=torch.bool), torch.zeros(N, dtype=torch.bool)):
        got, want = pb.score_auroc(scores, bits, sel), pb.score_auroc_reference(scores, bits, sel)
        for a, b in zip(got, want):
            assert a.dtype == torch.int64 and torch.equal(a, b)
    u2, pos, cnt, _, _ = pb.score_auroc(scores, bits, rows)
    assert bool((u2[:, 2] == pos[2] * (cnt - pos[2])).all())         # all tied: every pair counts half


class _NoCentring(pb._DenseOps):
    def __init__(self, *a):
        super().__init__(*a)
        self.mu = torch.zeros_like(self.mu)


class _NoMeanTerm(pb._DenseOps):
    def adjoint(self, u, w, alpha):
        return self.X.transpose(1, 2) @ u - alpha * w


def test_planted_errors_fail_the_closed_form_comparison():
    dense, bits, _ = C.solver_case(5)
    fit = torch.ones(dense.shape[1], dtype=torch.bool)
    y = bits.double() * 2 - 1
    ybar, yc = pb._targets(bits, fit, torch.float64)
    yc = yc.unsqueeze(0).expand(2, -1, -1).contiguous()
    raw = y.unsqueeze(0).expand(2, -1, -1).contiguous()

    def gap(ops, targets, n=96):
        w, _, conv, resid, _ = pb._cgls(ops, targets, n, 1.0, 600, 1e-12)
        assert bool(conv.all())
        g, bound, _, _ = _closed_gap(dense, bits, None, 1.0, w[:, :96], resid)
        return g, bound

    g, bound = gap(pb._DenseOps(dense, fit, torch.float64), yc)
    assert bool((g <= bound).all())                                  # the recurrence as it stands passes
    g, bound = gap(_NoCentring(dense, fit, torch.float64), raw)      # centring dropped: no intercept at all
    assert bool((g > 100 * bound).all())
    # the mu (sum u) term dropped: with centred targets sum r stays 0 exactly only in theory, so break it where it
    # matters -- uncentred targets, where that term carries the whole intercept (concept 2 has as many positives
    # as negatives: its targets sum to 0 and the term vanishes)
    assert int(y.sum(0)[2]) == 0
    g, bound = gap(_NoMeanTerm(dense, fit, torch.float64), raw)
    assert bool((g > 100 * bound)[:, [0, 1, 3, 4]].all())
    # alpha applied to the intercept: a column of ones, penalised like any other, no centring
    aug = torch.cat([dense.double(), torch.ones(2, dense.shape[1], 1, dtype=torch.float64)], 2)
    g, bound = gap(_NoCentring(aug, fit, torch.float64), raw, n=97)
    assert bool((g > 100 * bound).all())


def test_segment_table_covers_every_list_once():
    from sparse_coding__amd.engine.feature_codes import feature_codes_reference
    from sparse_coding__amd.ops import probe as pr

    seg = 64
    fc = feature_codes_reference(sparse_codes_reference([C.long_lists_dense(seg)]))
    plan = pr.lists_plan(fc.col_ptr, fc.cap, seg)
    lens = (fc.col_ptr[0, 1:] - fc.col_ptr[0, :-1]).tolist()
    assert lens == [seg - 1, seg, seg + 1, 2 * seg + 3, 0, 5]
    assert (plan.seg_ptr[0, 1:] - plan.seg_ptr[0, :-1]).tolist() == [1, 1, 2, 3, 1, 1]
    assert plan.seg_feat.shape == (1, 6 + fc.cap // seg) and plan.seg_feat.dtype == torch.int32
    assert plan.seg_feat[0].tolist() == [0, 1, 2, 2, 3, 3, 3, 4, 5] + [-1] * (plan.seg_feat.shape[1] - 9)
    assert pr.PROBE_SEG == 512 and pr.lists_plan(fc.col_ptr, fc.cap).seg_feat.shape[1] == 6
    for bad in (63, 65, 0, 2 ** 31):
        with pytest.raises(ValueError, match="segment"):
            pr.lists_plan(fc.col_ptr, fc.cap, bad)
    with pytest.raises(ValueError, match="waves"):
        pr.col_dots(torch.zeros(1, 4, 32), waves=3)
    with pytest.raises(ValueError, match="A must be"):
        pr.col_dots(torch.zeros(1, 4, 31))


def test_op_oracles_agree_with_dense_algebra():
    from sparse_coding__amd.engine.feature_codes import feature_codes_reference

    dense, sc = C.crafted_dense(70), C.crafted(70)
    P, R = C.int_operand(3, 70, 1), C.int_operand(3, C.N_EXACT, 2)
    shift = C.int_operand(3, 1, 3)[:, 0].double()
    mask = (torch.arange(C.N_EXACT) % 3 != 0).to(torch.uint8)
    Q, skipped = pb.rows_matmul_reference(sc, P, shift, mask)
    want = (dense.double() @ P.double() - shift.unsqueeze(1)) * (mask != 0).view(1, -1, 1)
    assert torch.equal(Q, want) and skipped.tolist() == [0, 0, 0]
    fc = feature_codes_reference(sc)
    S = pb.lists_matmul_reference(fc.col_ptr, fc.row, fc.val, R)
    assert torch.equal(S, dense.double().transpose(1, 2) @ R.double())
    assert torch.equal(pb.col_dots_reference(P, P), P.double().pow(2).sum(1))
    assert torch.equal(pb.col_dots_reference(R), R.double().sum(1))


def test_result_type_round_trips(tmp_path):
    dense, bits, fit = C.solver_case(5)
    sc = sparse_codes_reference([dense])
    res = sc.ridge_probes(bits, fit_rows=fit)
    assert isinstance(res, pb.LinearProbes) and res.weight.dtype == torch.float32 and res.n_concepts == 5
    assert res.intercept.dtype == torch.float64 and res.iters.dtype == torch.int32 and res.converged.dtype == torch.bool
    res.save(tmp_path / "probes.pt")
    C.same_probes(pb.LinearProbes.load(tmp_path / "probes.pt"), res)
    C.same_probes(res.to("cpu"), res)
    assert set(res.state_dict()) == set(res._TENSORS) | {"alpha", "n_rows"}
    feat, w = res.top_features(3)
    assert feat.shape == (2, 5, 3) and torch.equal(w, torch.gather(res.weight.transpose(1, 2), -1, feat))
    order = sorted(range(96), key=lambda f: (-abs(float(res.weight[1, f, 2])), f))[:3]
    assert feat[1, 2].tolist() == order
    with pytest.raises(ValueError, match="m must be"):
        res.top_features(0)
    other = sparse_codes_reference([dense[:, :100]])
    s = res.scores(other)
    want = dense[:, :100].double() @ res.weight.double() + res.intercept.unsqueeze(1)
    assert s.shape == (2, 100, 5) and float((s - want).abs().max()) <= 1e-5
    from sparse_coding__amd.eval import metrics

    assert torch.equal(metrics.ridge_probe_auroc(sc, bits, fit_rows=fit), res.auroc())
    with pytest.raises(TypeError, match="device route"):
        sc.ridge_probes(bits, waves=4)


def test_surfaces_route_and_refuse():
    from sparse_coding__amd.engine.analysis import CodeAnalyses, TorchCodeAnalyses
    from sparse_coding__amd.engine.fused import FusedSAEEnsemble
    from sparse_coding__amd.engine.topk import FusedTopKEnsemble
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.eval import metrics
    from sparse_coding__amd.models.signatures import FunctionalSAE

    want = CodeAnalyses.__dict__["ridge_probes"]
    for cls in (FusedSAEEnsemble, FusedTopKEnsemble, TorchCodeAnalyses):
        assert getattr(cls, "ridge_probes") is want and want.__doc__
    eng = object.__new__(FusedSAEEnsemble)
    for kind, learned, word in (("threshold", False, "threshold"), ("reverse", False, "reverse"),
                                ("tied", True, "learned centering")):
        eng.kind, eng.learned_center = kind, learned
        with pytest.raises(NotImplementedError, match=f"ridge_probes: .*{word}"):
            eng.ridge_probes(torch.zeros(128, 256), torch.zeros(128, dtype=torch.int32))
    torch.manual_seed(0)
    models = [FunctionalSAE.init(16, 32, 1e-3) for _ in range(2)]
    tr = EnsembleTrainer(models, FunctionalSAE, batch_size=16, device="cpu", engine="eager")
    rows = torch.randn(64, 16)
    labels = rows[:, 0] > 0
    res = tr.ridge_probes(rows, labels.unsqueeze(1), fit_rows=torch.arange(64) < 48)
    assert isinstance(res, pb.LinearProbes) and res.weight.shape == (2, 32, 1) and int(res.cnt_held) == 16
    C.same_probes(res, tr.encode_sparse(rows).ridge_probes(labels.unsqueeze(1), fit_rows=torch.arange(64) < 48))
    out = metrics.ensemble_ridge_regression_auroc(tr, rows, labels)
    assert out.shape == (2,) and torch.equal(out, tr.ridge_probes(rows, labels.unsqueeze(1)).auroc_predicted()[:, 0])
    assert metrics.ensemble_ridge_regression_auroc(tr, rows, torch.stack([labels, ~labels], 1).long()).shape == (2, 2)
    dp = EnsembleTrainer(models, FunctionalSAE, batch_size=16, device="cpu", engine="eager", parallel="dp")
    with pytest.raises(NotImplementedError, match="data-parallel"):
        dp.ridge_probes(rows, labels.unsqueeze(1))
    assert math.isfinite(float(res.auroc()[0, 0]))
