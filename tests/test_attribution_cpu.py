"""The attribution oracles on the CPU (``engine/attribution.py``): against a dense brute force, the algebra they
rest on, ``merge`` / ``state=``, ``top_mask``, masked models, persistence, the trainer's torch route and
``fvu_top_activating(rank_by=)``."""

import pytest
import torch

import attribution_cases as C
from sparse_coding__amd.engine import attribution as at
from sparse_coding__amd.engine import sparse_recon as sr
from sparse_coding__amd.engine.sparse_codes import SparseCodes, sparse_codes_reference

SMALL = (64, 96)     # the planted case the dense brute force can afford


def test_delta_sse_is_the_dense_leave_one_out_difference():
    k = C.planted(*SMALL)
    ref, _ = C.planted_reference(*SMALL)
    dense = at.attribution_dense_reference(k["sc"], k["D"], k["x"])
    assert not ref.skipped.any() and not ref.missing.any() and ref.check() is ref
    assert torch.equal(ref.delta_sse, dense)            # (planted: every number is an exact dyadic rational)
    assert bool((dense != 0).any()) and bool((dense < 0).any()) and bool((dense > 0).any())
    assert torch.equal(ref.cnt, (k["dense"] > 0).sum(1))
    # random bf16 rows: the fp32 order of proj and q stays within the forward bound
    r = C.random_rows()
    sc, D, x = r["sc"].narrow_rows(0, 24), r["D"], r["x"][:, :24].contiguous()
    got = at.attribution_reference(sc, D, x)
    rp = at.residual_proj_reference(sc, D, x)
    dense = at.attribution_dense_reference(sc, D, x)
    tol = torch.zeros_like(dense)
    for g in range(C.G):
        kk = int(sc.row_ptr[g, -1])
        tol[g].index_add_(0, sc.col[g, :kk].long(), 2 * sc.val[g, :kk].double() * rp.bound[g, :kk])
    tol += got.C2 * got.q.double() * at._gamma(D.shape[2] // 16 + 4) + 1e-9 * dense.abs()
    assert bool(((got.delta_sse - dense).abs() <= tol).all()) and bool((tol < 1e-3 * dense.abs().max()).all())


def test_removing_one_entry_changes_its_row_by_delta_e():
    r = C.random_rows()
    sc, D, x = r["sc"], r["D"].double(), r["x"].double()
    ref = r["ref"]
    q = (D * D).sum(-1)
    for g in range(C.G):
        rows = sc.entry_rows(g)
        for e in range(0, int(sc.row_ptr[g, -1]), 97):
            i, f, c = int(rows[e]), int(sc.col[g, e]), sc.val[g, e].double()
            cols, vals = sc.row(g, i)
            res = x[g, i] - (vals.double().unsqueeze(1) * D[g, cols.long()]).sum(0)
            want = (res + c * D[g, f]).pow(2).sum() - res.pow(2).sum()
            got = 2 * c * ref.proj64[g, e] + c * c * q[g, f]
            assert abs(float(want - got)) <= 1e-12 * float(res.pow(2).sum() + c * c)
            assert abs(float(ref.proj[g, e]) - float(ref.proj64[g, e])) <= float(ref.bound[g, e])


def test_rescale_lowers_the_dense_sse_by_rescale_gain():
    k = C.planted(*SMALL)
    ref, _ = C.planted_reference(*SMALL)
    D, x = k["D"].double(), k["x"].double()
    for g in range(C.G):
        dense = k["sc"].to_dense(g).double()
        full = (x[g] - dense @ D[g]).pow(2).sum()
        assert float(full) == float(ref.sse_full[g])
        for f in torch.nonzero(ref.cnt[g] > 0).flatten()[::7].tolist():
            scaled = dense.clone()
            scaled[:, f] *= ref.rescale[g, f]
            after = (x[g] - scaled @ D[g]).pow(2).sum()
            assert abs(float(full - after) - float(ref.rescale_gain[g, f])) <= 1e-9 * float(full)
            assert float(ref.rescale_gain[g, f]) >= 0


def test_views_and_an_empty_feature():
    ref, _ = C.planted_reference(*SMALL)
    live = C.live_of(96)
    dead = ref.cnt == 0
    assert bool(dead[0, live[0]:].all()) and bool(dead.any())       # model 0 is masked to 70 features
    for v in (ref.delta_sse, ref.delta_fvu, ref.rescale, ref.rescale_gain, ref.harmful_fraction, ref.mean_proj,
              ref.A, ref.P1, ref.C2, ref.min_delta.double(), ref.max_delta.double(), ref.n_harm.double()):
        assert v.dtype == torch.float64 and not v[dead].any()
    some = ~dead
    assert torch.equal(ref.delta_sse, 2 * ref.A + ref.q.double() * ref.C2)
    assert torch.equal(ref.delta_fvu[some], (ref.delta_sse / ref.variance.unsqueeze(1))[some])
    assert torch.equal(ref.rescale[some], (1 + ref.A / (ref.q.double() * ref.C2))[some])
    assert torch.equal(ref.harmful_fraction[some], (ref.n_harm.double() / ref.cnt.double())[some])
    assert torch.equal(ref.mean_proj[some], (ref.P1 / ref.cnt.double())[some])
    assert bool((ref.min_delta <= ref.max_delta).all()) and bool((ref.n_harm <= ref.cnt).all())
    assert torch.equal(ref.n_harm == 0, (ref.min_delta >= 0))
    assert torch.allclose(ref.variance, sr.recon_profile_reference(C.planted(*SMALL)["sc"], C.planted(*SMALL)["D"],
                                                                   C.planted(*SMALL)["x"], 0).variance)


def test_merge_and_state_add_the_raw_sums():
    k = C.planted(*SMALL)
    sc, D, x, live = k["sc"], k["D"], k["x"], k["live"]
    whole, _ = C.planted_reference(*SMALL)
    cut = 7
    a = at.attribution_reference(sc.narrow_rows(0, cut), D, x[:, :cut], live)
    b = at.attribution_reference(sc.narrow_rows(cut, sc.n_rows), D, x[:, cut:], live)
    m = a.merge(b)
    via_state = at.attribution_reference(sc.narrow_rows(cut, sc.n_rows), D, x[:, cut:], live, state=a)
    C.same(via_state, m)
    assert m.n_rows == sc.n_rows and torch.equal(m.A, a.A + b.A) and torch.equal(m.cnt, a.cnt + b.cnt)
    for f in ("cnt", "n_harm", "min_delta", "max_delta", "skipped", "missing"):     # chunk-invariant
        assert torch.equal(getattr(m, f), getattr(whole, f)), f
    for f in ("A", "P1", "C2", "sse_full", "s2"):       # (planted sums are exact, so here even these agree)
        assert torch.equal(getattr(m, f), getattr(whole, f)), f
    # random rows: integers and extrema agree with one call, the fp64 sums only to rounding
    r = C.random_rows()
    sc, D, x = r["sc"], r["D"], r["x"]
    one = at.attribution_reference(sc, D, x)
    two = at.attribution_reference(sc.narrow_rows(0, 50), D, x[:, :50]).merge(
        at.attribution_reference(sc.narrow_rows(50, sc.n_rows), D, x[:, 50:]))
    for f in ("cnt", "n_harm", "min_delta", "max_delta"):
        assert torch.equal(getattr(one, f), getattr(two, f)), f
    assert torch.allclose(one.A, two.A, rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError):
        one.merge(whole)
    with pytest.raises(ValueError):
        at.attribution_reference(sc, D, x, state="no state")


def test_top_mask_breaks_ties_to_the_lower_index_below_nactive():
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt)
    A = torch.tensor([[1.0, 3.0, 3.0, 0.5, 3.0, 9.0], [2.0, 2.0, 2.0, 2.0, 2.0, 2.0]], dtype=torch.float64) / 2
    attr = at.Attribution(4, torch.ones(2, 6, dtype=torch.int64), A, z(2, 6), z(2, 6), z(2, 6, dt=torch.int64),
                          z(2, 6, dt=torch.float32), z(2, 6, dt=torch.float32), torch.ones(2, 6), z(2), z(2, 64), z(2),
                          z(2, dt=torch.int64), z(2, dt=torch.int64), torch.tensor([5, 6], dtype=torch.int32))
    assert attr.delta_sse.tolist() == (2 * A).tolist()
    assert attr.top_mask(2).tolist() == [[False, True, True, False, False, False],     # (feature 5 is not live)
                                         [True, True, False, False, False, False]]
    assert attr.top_mask(0).sum() == 0 and attr.top_mask(6).sum(1).tolist() == [5, 6]


def test_a_column_past_nactive_skips_its_row():
    k = C.planted(*SMALL)
    sc = k["sc"]
    ref = at.attribution_reference(sc, k["D"], k["x"], [70, 60])        # model 1 has columns up to 95
    rows = (torch.stack([(k["dense"][1, r, 60:] > 0).any() for r in range(sc.n_rows)])).sum()
    assert ref.skipped.tolist() == [0, int(rows)] and int(rows) > 0 and not ref.missing.any()
    assert not ref.cnt[1, 60:].any()
    with pytest.raises(at.AttributionSkipped):
        ref.check()


def test_shape_limits_raise_value_error():
    sc = sparse_codes_reference([torch.ones(1, 2, 4)])
    for d in (32, 96, 1088):
        with pytest.raises(ValueError, match="d % 64"):
            at.attribution_reference(sc, torch.zeros(1, 4, d), torch.zeros(2, d))
    with pytest.raises(ValueError):
        at.attribution_reference(sc, torch.zeros(1, 5, 64), torch.zeros(2, 64))
    with pytest.raises(ValueError):
        at.attribution_reference(sc, torch.zeros(1, 4, 64), torch.zeros(3, 64))
    with pytest.raises(TypeError):
        sc.attribution(torch.zeros(1, 4, 64), torch.zeros(2, 64), waves=2)


def test_sparse_codes_method_metrics_and_save_load(tmp_path):
    from sparse_coding__amd.eval import metrics

    k = C.planted(*SMALL)
    ref, _ = C.planted_reference(*SMALL)
    got = k["sc"].attribution(k["D"], k["x"], nactive=k["live"], return_proj=True)
    C.same(got, ref)
    assert torch.equal(got.proj, ref.proj)
    dsse, dfvu = metrics.ablation_effects(k["sc"], k["D"], k["x"], k["live"])
    assert torch.equal(dsse, ref.delta_sse) and torch.equal(dfvu, ref.delta_fvu)
    assert torch.equal(metrics.feature_shrinkage(k["sc"], k["D"], k["x"], k["live"]), ref.rescale)
    got.save(tmp_path / "a.pt")
    back = at.Attribution.load(tmp_path / "a.pt")
    C.same(back, got, C.RAW + ("q", "sse_full", "s1", "s2", "skipped", "missing", "live", "proj"))
    assert torch.equal(back.to("cpu").delta_sse, got.delta_sse)


def test_list_walk_oracle_reads_the_order_literals_and_matches_a_direct_sum():
    k = C.lists()
    cnt, A, P1, C2, n_harm, mn, mx, missing = k["want"]
    assert not missing.any()
    for g in range(C.G):
        assert A[g, C.F_ORDER_LANE0].item() == C.ORDER_LANE0 and A[g, C.F_ORDER_012].item() == C.ORDER_012
        assert A[g, C.F_ORDER_MIX].item() == C.ORDER_MIX != C.SEQUENTIAL
        assert P1[g, C.F_ORDER_MIX].item() == C.ORDER_MIX
    assert cnt[0, :7].tolist() == [0, 1, 63, 64, 65, 129, C.LIST_ROWS]
    sc = k["sc"]
    for g in range(C.G):
        kk = int(sc.row_ptr[g, -1])
        c, p, col = sc.val[g, :kk].double(), k["proj"][g, :kk].double(), sc.col[g, :kk].long()
        direct = torch.zeros(C.LIST_N, dtype=torch.float64).index_add_(0, col, c * p)
        plain = [f for f in range(C.LIST_N) if f not in C.ORDER_TERMS]
        assert torch.allclose(A[g, plain], direct[plain], rtol=1e-12, atol=1e-12)
        delta = 2 * p + c * k["q"][g].double()[col]
        harm = torch.zeros(C.LIST_N, dtype=torch.int64).index_add_(0, col, (delta < 0).long())
        assert torch.equal(n_harm[g], harm) and bool(harm.any())
    assert not mn[0, C.F_EMPTY] and not mx[0, C.F_EMPTY] and not A[0, C.F_EMPTY]


def test_entries_that_cannot_be_found_are_counted_missing():
    k = C.lists()
    sc, fc = k["sc"], k["fc"]
    other = sparse_codes_reference([torch.flip(sc.to_dense(0), [1]).unsqueeze(0).repeat(C.G, 1, 1)])
    got = at.attr_list_sums_reference(fc, other, torch.zeros(C.G, other.cap), k["q"])
    dense_a, dense_b = torch.stack([sc.to_dense(g) for g in range(C.G)]) > 0, \
        torch.stack([other.to_dense(g) for g in range(C.G)]) > 0
    assert got[7].tolist() == (dense_a & ~dense_b).sum((1, 2)).tolist() and bool(got[7].all())
    assert torch.equal(got[0], (dense_a & dense_b).sum(1))
    short = SparseCodes(sc.n_rows - 60, sc.n, sc.row_ptr[:, :-60].contiguous(), sc.col, sc.val)
    got = at.attr_list_sums_reference(fc, short, k["proj"], k["q"])
    assert got[7].tolist() == (dense_a[:, -60:]).sum((1, 2)).tolist()


# ----------------------------------------------------------------------------- trainer routing
def _sae_trainer(engine, parallel=None, n_models=2, d=64, n=32):
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.signatures import FunctionalSAE

    torch.manual_seed(0)
    models = [FunctionalSAE.init(d, n, 1e-3) for _ in range(n_models)]
    kw = {} if parallel is None else {"parallel": parallel}
    return EnsembleTrainer(models, FunctionalSAE, batch_size=16, device="cpu", engine=engine, **kw)


def _dicts(tr):
    lds = tr.impl.to_learned_dicts("cpu")
    return torch.stack([ld.get_learned_dict().detach().float() for ld in lds])


def test_trainer_routes_the_analytic_engine_to_the_oracle():
    tr = _sae_trainer("analytic")
    rows = torch.randn(48, 64, generator=torch.Generator().manual_seed(1))
    got = tr.attribution(rows)
    codes = tr.encode_sparse(rows)
    want = at.attribution_reference(codes, _dicts(tr), rows.unsqueeze(0).expand(2, -1, -1), [32, 32])
    C.same(got, want)
    assert isinstance(got, at.Attribution) and int(got.cnt.sum()) > 0 and got.check() is got
    dense = at.attribution_dense_reference(codes, _dicts(tr), rows)
    assert torch.allclose(got.delta_sse, dense, rtol=1e-4, atol=1e-4 * float(dense.abs().max()))
    part = tr.attribution(rows[16:], state=tr.attribution(rows[:16]))
    assert part.n_rows == 48 and torch.equal(part.cnt, got.cnt) and torch.allclose(part.A, got.A, atol=1e-9)


def test_trainer_refusals():
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.topk import TopKEncoder

    rows = torch.randn(64, 64)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        _sae_trainer("eager", parallel="dp").attribution(rows)
    torch.manual_seed(0)
    tk = EnsembleTrainer([TopKEncoder.init(64, 32, 4) for _ in range(2)], TopKEncoder, batch_size=16, device="cpu",
                         engine="eager")
    with pytest.raises(NotImplementedError, match="attribution"):
        tk.attribution(rows)


def test_fvu_top_activating_rank_by():
    tr = _sae_trainer("analytic")
    rows = torch.randn(48, 64, generator=torch.Generator().manual_seed(3))
    top, rest = tr.fvu_top_activating(rows, 3)
    again = tr.fvu_top_activating(rows, 3, rank_by="sum")
    live = torch.tensor([32, 32])
    want = tr.recon_profile(rows, max_kept=0, keep=sr.top_features(tr.feature_stats(rows).sums[:, 0], 3, live))
    assert torch.equal(top, again[0]) and torch.equal(rest, again[1])
    assert torch.equal(top, want.fvu_keep) and torch.equal(rest, want.fvu_rest)
    top, rest = tr.fvu_top_activating(rows, 3, rank_by="delta_sse")
    mask = tr.attribution(rows).top_mask(3)
    want = tr.recon_profile(rows, max_kept=0, keep=mask)
    assert mask.sum(1).tolist() == [3, 3]
    assert torch.equal(top, want.fvu_keep) and torch.equal(rest, want.fvu_rest)
    with pytest.raises(ValueError, match="rank_by"):
        tr.fvu_top_activating(rows, 3, rank_by="max")
