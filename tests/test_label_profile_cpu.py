"""Label profiles off the GPU: the torch oracle against a brute-force group-by on dense codes, ``take_rows``,
the argument checks, persistence, the derived views, the trainer's routing and the consumers.  Every comparison
of profile outputs is ``torch.equal``."""

import pytest
import torch

import label_profile_cases as C
from sparse_coding__amd.engine import label_profile as lp
from sparse_coding__amd.engine.sparse_codes import (SparseCodes, SparseCodesOverflow, sparse_codes_reference,
                                                    take_rows_reference)

CASE_IDS = ["N%d-n%d-%s" % c for c in C.CASES]


# ----------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("rank_by", C.RANKS)
@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_oracle_matches_a_brute_force_group_by(case, rank_by):
    sc, labels, n_classes, _, pool = C.case(*case)
    for m in C.MS:
        ref = C.reference(*case, m, rank_by)
        want = C.brute_profile(pool, labels, m, rank_by)
        C.same_tuple(tuple(getattr(ref, k) for k in C.FIELDS), want)
        assert ref.n_rows == case[0] - C.DROPPED and ref.skipped.tolist() == [0] * C.G
        assert ref.top_label.shape == (C.G, case[1], m)
        if n_classes is not None:
            assert torch.equal(ref.label_rows, torch.bincount(labels[labels >= 0], minlength=n_classes))


@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_the_order_sensitive_runs_read_their_literals(case):
    ref = C.reference(*case, 8, "sum")
    for g in range(C.G):
        assert ref.top_sum[g, C.F_ORDER_A, 0].item() == C.ORDER_SUM_A == 2.0 ** 53
        assert ref.top_sum[g, C.F_ORDER_B, 0].item() == C.ORDER_SUM_B == 2.0 ** 53 + 2.0
        assert ref.top_count[g, C.F_ORDER_A, :2].tolist() == [3, 1]
        assert ref.total[g, C.F_ORDER_A].item() == 2.0 ** 53 + 4.0      # (+ 3.0 rounds to even: up)


def test_crafted_features_look_as_designed():
    sc, labels, _, notes, _ = C.case(384, 640, "L5")
    ref = C.reference(384, 640, "L5", 8, "count")
    M = 384 - C.DROPPED
    assert {"len129", "span3", "end64"} <= notes
    assert ref.n_entries[0, [C.F_EMPTY, C.F_ONE, C.F_63, C.F_64, C.F_65, C.F_129, C.F_EVERY]].tolist() == \
        [0, 1, 63, 64, 65, 129, M]
    assert ref.n_labels[0, C.F_EVERY].item() == 5 and ref.n_labels[0, C.F_ONELABEL].item() == 1
    assert ref.top_label[0, C.F_EMPTY].tolist() == [-1] * 8
    assert ref.top_count[0, C.F_SPAN3, 0].item() == 140 and ref.n_labels[0, C.F_SPAN3].item() == 1
    assert ref.n_labels[0, C.F_RUNS[5]].item() == 5
    tie = C.reference(128, 128, "sparse", 8, "sum")
    assert tie.top_sum[1, C.F_TIE, :3].tolist() == [1.5, 1.5, 1.25] and tie.top_count[1, C.F_TIE, :2].tolist() == [2, 2]
    assert tie.top_label[1, C.F_TIE, 0] < tie.top_label[1, C.F_TIE, 1]
    assert int(tie.top_label.max()) == C.LABEL_MAX
    runs = C.reference(384, 640, "L70", 64, "count")
    for k, f in C.F_RUNS.items():
        assert runs.n_labels[2, f].item() == k and int((runs.top_label[2, f] >= 0).sum()) == min(k, 64)


def test_masked_model_skips_the_row_with_a_dead_column():
    sc, labels, nactive = C.masked_case()
    ref = lp.label_profile_reference(sc, labels, m=8, nactive=nactive, n_classes=5)
    assert ref.skipped.tolist() == [0, 0, 1]
    pool = torch.stack([sc.to_dense(g) for g in range(C.G)])
    pool[2, int(torch.nonzero(labels >= 0).flatten()[9])] = 0.0
    pool[2, :, 100:] = 0.0
    C.same_tuple(tuple(getattr(ref, k) for k in C.FIELDS), C.brute_profile(pool, labels, 8, "sum"))
    assert not ref.n_entries[2, 100:].any() and bool((ref.top_label[2, 100:] == -1).all())


def test_label_profile_on_cpu_tensors_is_the_oracle():
    sc, labels, n_classes, _, _ = C.case(128, 128, "L70")
    for rank_by in C.RANKS:
        C.same(lp.label_profile(sc, labels, m=8, rank_by=rank_by, n_classes=n_classes), C.reference(128, 128, "L70", 8, rank_by))
        C.same(sc.label_profile(labels.to(torch.int32), m=8, rank_by=rank_by, n_classes=n_classes),
               C.reference(128, 128, "L70", 8, rank_by))
    none = sc.label_profile(torch.full_like(labels, -1), m=4)
    assert none.n_rows == 0 and not none.n_entries.any() and bool((none.top_label == -1).all())


def test_lists_oracle_on_label_ordered_codes_is_the_csr_oracle():
    """The route of the device on the host: take_rows in label order, transpose, walk the lists."""
    from sparse_coding__amd.engine.feature_codes import feature_codes_reference

    sc, labels, _, _, _ = C.case(128, 128, "sparse")
    kept = torch.nonzero(labels >= 0).flatten()
    lab, order = torch.sort(labels[kept], stable=True)
    fc = feature_codes_reference(sc.take_rows(kept[order]))
    for rank_by in C.RANKS:
        got = lp.profile_lists_reference(fc.col_ptr, fc.row, fc.val, lab.to(torch.int32), 8, rank_by)
        ref = C.reference(128, 128, "sparse", 8, rank_by)
        C.same_tuple(got, tuple(getattr(ref, k) for k in C.FIELDS))


# ----------------------------------------------------------------------------- take_rows
def test_take_rows_reference_matches_dense_row_indexing():
    sc, _, _, _, pool = C.case(128, 128, "L5")
    gen = torch.Generator().manual_seed(4)
    for index in (torch.randint(0, 128, (300,), generator=gen), torch.tensor([5, 5, 5, 0, 127, 5]),
                  torch.arange(127, -1, -1), torch.zeros(0, dtype=torch.int64)):
        for got in (take_rows_reference(sc, index), sc.take_rows(index)):
            assert got.n_rows == index.numel() and got.n == sc.n and got.row_ptr.shape == (C.G, index.numel() + 1)
            assert got.cap == int(got.nnz().max()) if index.numel() else got.cap == 0
            got.check()
            want = sparse_codes_reference([pool[:, index]]) if index.numel() else None
            if want is not None:
                for k in ("row_ptr", "col", "val"):
                    assert torch.equal(getattr(got, k), getattr(want, k)), k


def test_narrow_rows_is_take_rows_of_a_range():
    sc = C.case(128, 128, "L70")[0]
    for lo, hi in ((0, 128), (17, 90), (40, 40), (127, 128)):
        a, b = sc.narrow_rows(lo, hi), sc.take_rows(torch.arange(lo, hi))
        assert a.n_rows == b.n_rows
        for k in ("row_ptr", "col", "val"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (lo, hi, k)


def test_take_rows_argument_checks():
    sc, _, _, _, pool = C.case(128, 128, "L5")
    for bad in (torch.tensor([0, 128]), torch.tensor([-1])):
        with pytest.raises(IndexError):
            sc.take_rows(bad)
    for bad in (torch.tensor([0, 1], dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64), [0, 1]):
        with pytest.raises(ValueError):
            sc.take_rows(bad)
    with pytest.raises(TypeError):
        sc.take_rows(torch.tensor([0]), waves=2)
    over = sparse_codes_reference([pool], cap=int(sc.nnz().min()) // 2)
    with pytest.raises(SparseCodesOverflow):
        over.take_rows(torch.tensor([0]))


# ----------------------------------------------------------------------------- arguments, persistence, views
def test_argument_checks():
    sc, labels, _, _, _ = C.case(128, 128, "L5")
    with pytest.raises(ValueError, match="one label per row"):
        lp.label_profile(sc, labels[:-1])
    with pytest.raises(ValueError, match="n_classes"):
        lp.label_profile(sc, labels, n_classes=4)
    with pytest.raises(ValueError, match="2\\^31"):
        lp.label_profile(sc, torch.full_like(labels, 2 ** 31 - 1))
    for m in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="1..64"):
            lp.label_profile(sc, labels, m=m)
    with pytest.raises(ValueError, match="rank_by"):
        lp.label_profile(sc, labels, rank_by="mean")
    with pytest.raises(ValueError):
        lp.label_profile(sc, labels.float())
    with pytest.raises(ValueError, match="n_classes"):
        C.reference(128, 128, "sparse", 8, "sum").recall()


def test_save_load_round_trip(tmp_path):
    for kind in ("L5", "sparse"):
        ref = C.reference(128, 128, kind, 8, "count")
        ref.save(tmp_path / "p.pt")
        C.same(lp.LabelProfile.load(tmp_path / "p.pt"), ref)
        C.same(ref.to("cpu"), ref)


def test_derived_views_match_the_direct_formulas():
    sc, labels, n_classes, _, pool = C.case(128, 128, "L5")
    ref = C.reference(128, 128, "L5", 8, "sum")
    kept = labels >= 0
    fires = (pool > 0) & kept.view(1, -1, 1)
    tot = torch.where(fires, pool, torch.zeros(())).double().sum(1)
    per_label = torch.stack([(fires & (labels == v).view(1, -1, 1)).sum(1) for v in range(5)], 1).double()   # [G, L, n]
    sums = torch.stack([torch.where(fires & (labels == v).view(1, -1, 1), pool, torch.zeros(())).double().sum(1)
                        for v in range(5)], 1)
    rows = torch.bincount(labels[kept], minlength=5).double()
    share, prec, rec, f1, eff = ref.share(), ref.precision(), ref.recall(), ref.f1(), ref.effective_labels()
    for t in (share, prec, rec, f1, eff):
        assert t.dtype == torch.float64
    live = ref.top_label >= 0
    at = ref.top_label.clamp(min=0).long().transpose(1, 2)                                               # [G, m, n]
    ne = fires.sum(1).double()
    div = lambda a, b: torch.where(b > 0, a / b.clamp(min=1e-300), torch.zeros_like(a))
    want_p = torch.where(live, div(per_label.gather(1, at).transpose(1, 2), ne.unsqueeze(-1).expand(-1, -1, 8)), torch.zeros(()).double())
    want_r = torch.where(live, per_label.gather(1, at).transpose(1, 2) / rows[ref.top_label.clamp(min=0).long()], torch.zeros(()).double())
    want_s = torch.where(live, div(sums.gather(1, at).transpose(1, 2), tot.unsqueeze(-1).expand(-1, -1, 8)), torch.zeros(()).double())
    assert torch.allclose(prec, want_p, rtol=1e-12, atol=0) and torch.allclose(rec, want_r, rtol=1e-12, atol=0)
    assert torch.allclose(share, want_s, rtol=1e-12, atol=0)
    assert torch.allclose(f1, div(2 * want_p * want_r, want_p + want_r), rtol=1e-12, atol=0)
    assert torch.allclose(eff, div(ne * ne, (per_label ** 2).sum(1)), rtol=1e-12, atol=0)
    assert not share[0, C.F_EMPTY].any() and eff[0, C.F_EMPTY].item() == 0.0 and eff[0, C.F_ONELABEL].item() == 1.0
    assert prec[0, C.F_ONELABEL, 0].item() == 1.0 and rec[0, C.F_ONELABEL, 0].item() == 1.0


# ----------------------------------------------------------------------------- trainer routing
def _sae_trainer(engine, parallel=None, n_models=2, d=16, n=32):
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.signatures import FunctionalSAE

    torch.manual_seed(0)
    models = [FunctionalSAE.init(d, n, 1e-3) for _ in range(n_models)]
    kw = {} if parallel is None else {"parallel": parallel}
    return EnsembleTrainer(models, FunctionalSAE, batch_size=16, device="cpu", engine=engine, **kw)


@pytest.mark.parametrize("engine", ["analytic", "eager"])
def test_trainer_routes_the_torch_engines_to_the_oracle(engine):
    tr = _sae_trainer(engine)
    rows = torch.randn(64, 16, generator=torch.Generator().manual_seed(1))
    labels = torch.randint(-1, 6, (64,), generator=torch.Generator().manual_seed(2))
    got = tr.label_profile(rows, labels, m=4, rank_by="count", n_classes=6)
    assert isinstance(got, lp.LabelProfile) and got.top_label.shape == (2, 32, 4)
    C.same(got, lp.label_profile_reference(tr.encode_sparse(rows), labels, m=4, rank_by="count", n_classes=6))
    assert int(got.n_entries.sum()) > 0


def test_trainer_refusals():
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.topk import TopKEncoder

    rows, labels = torch.randn(64, 16), torch.zeros(64, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        _sae_trainer("eager", parallel="dp").label_profile(rows, labels)
    torch.manual_seed(0)
    tk = EnsembleTrainer([TopKEncoder.init(16, 32, 4) for _ in range(2)], TopKEncoder, batch_size=16, device="cpu",
                         engine="eager")
    with pytest.raises(NotImplementedError, match="label_profile"):
        tk.label_profile(rows, labels)


# ----------------------------------------------------------------------------- consumers
def _planted():
    """Two models, 4 features, 12 rows of tokens 0 .. 3: feature 0 fires exactly on token 2; feature 1 on token 1
    and on one row of token 3; feature 2 everywhere; feature 3 never."""
    tokens = torch.tensor([0, 1, 2, 3, 2, 1, 0, 2, 3, 3, 1, 0])
    dense = torch.zeros(2, 12, 4)
    dense[:, tokens == 2, 0] = 1.5
    dense[:, tokens == 1, 1] = 2.0
    dense[:, 3, 1] = 0.25
    dense[:, :, 2] = 0.5
    return sparse_codes_reference([dense]), tokens


def test_label_selectivity_on_a_planted_example():
    from sparse_coding__amd.eval.metrics import label_selectivity

    sc, tokens = _planted()
    label, p, r, f = label_selectivity(sc, tokens, 4)
    assert label.shape == (2, 4) and p.dtype == torch.float64
    assert label[0].tolist() == [2, 1, 0, -1]
    assert p[0, 0].item() == r[0, 0].item() == f[0, 0].item() == 1.0
    assert p[0, 1].item() == 0.75 and r[0, 1].item() == 1.0
    assert p[1, 2].item() == 0.25 and r[1, 2].item() == 1.0 and p[0, 3].item() == r[0, 3].item() == f[0, 3].item() == 0.0
    label3, _, _, f3 = label_selectivity(sc, tokens, 4, m=3)
    assert label3[0].tolist() == [2, 1, 0, -1] and bool((f3 >= f).all())


def test_token_profile_explainer_reads_the_planted_token():
    from sparse_coding__amd.interp.autointerp import Explainer, TokenListSimulator, TokenProfileExplainer

    sc, tokens = _planted()
    prof = sc.label_profile(tokens, m=4, n_classes=4)
    detok = lambda t: "tok%d" % t
    ex = TokenProfileExplainer(prof, 1, detok, k=2)
    one: Explainer = ex.for_feature(0)
    assert one.explain([], 0.0) == "tokens: tok2"
    assert ex.for_feature(1).explain([], 0.0) == "tokens: tok1 | tok3"
    assert ex.for_feature(3).explain([], 0.0) == "tokens: "
    assert TokenListSimulator().simulate(one.explain([], 0.0), ["tok0", "tok2"]) == [0.0, 1.0]
    with pytest.raises(ValueError):
        ex.explain([], 0.0)
    with pytest.raises(IndexError):
        ex.for_feature(4)


def test_token_labels_and_ensemble_token_profiles():
    import feature_codes_cases as FC
    from sparse_coding__amd.interp.activations import ensemble_token_profiles, token_labels

    frags = torch.tensor([[3, 4, 5, 4], [7, 3, 3, 9]])
    assert token_labels(frags).tolist() == [3, 4, 5, 4, 7, 3, 3, 9]
    assert token_labels(frags, "prev").tolist() == [-1, 3, 4, 5, -1, 7, 3, 3]
    assert token_labels(frags, "self", ignore=(3, 9)).tolist() == [-1, 4, 5, 4, 7, -1, -1, -1]
    with pytest.raises(ValueError):
        token_labels(frags, "next")
    tr = _sae_trainer("eager")
    lm = FC.TinyLM(16)
    gen = torch.Generator().manual_seed(3)
    frags = torch.randint(0, 50, (7, 6), generator=gen)            # 42 rows: padded to 48
    for context in ("self", "prev"):
        got = ensemble_token_profiles(lm, tr, 0, "residual", frags, m=3, context=context, ignore=(0,), n_classes=50)
        rows = torch.zeros(48, 16)
        rows[:42] = lm.emb[frags].reshape(42, 16)
        labels = torch.full((48,), -1, dtype=torch.int64)
        labels[:42] = token_labels(frags, context, (0,))
        C.same(got, lp.label_profile_reference(tr.encode_sparse(rows), labels, m=3, n_classes=50))
        assert got.n_rows == int((labels >= 0).sum())
    assert lm.calls == 2
