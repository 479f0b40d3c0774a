"""Feature-major sparse codes on the MI355X: the kernels of ``csrc/feature_codes.hip`` against the torch oracles
on the crafted inputs of ``feature_codes_cases.py`` (both histogram paths, segment boundaries, undersized
buffers, the skip rule), the example-fragment and record kernels, ``feature_examples`` of the engines and the
trainer, and agreement with the dense activation dataset.  Every comparison is ``torch.equal``."""

import pytest
import torch

import feature_codes_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = C.G
ROW_SENTINEL, VAL_SENTINEL = -7, -1.0
FIELDS = ("col_ptr", "row", "val", "skipped")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_coding__amd.ops import _lib as L

    L.lib()  # must load: no silent fallback on a GPU box
    yield


@pytest.fixture(scope="module", params=C.SHAPES, ids=lambda s: f"N{s[0]}-n{s[1]}")
def case(request):
    from sparse_coding__amd.engine import feature_codes as fcm

    N, n = request.param
    sc = C.codes(C.crafted_dense(N, n, seed=N + n))
    return sc.to(DEV), fcm.feature_codes_reference(sc)


def _same(got, ref, fields=FIELDS):
    for k in fields:
        a, b = getattr(got, k), getattr(ref, k)
        assert a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu()), k


# ----------------------------------------------------------------------------- the transposition
@pytest.mark.parametrize("lds_bins", [8192, 64], ids=["lds", "global"])
def test_by_feature_matches_oracle_under_any_geometry(case, lds_bins):
    sc, ref = case
    runs = [sc.by_feature(segment_rows=C.SEGMENT_ROWS, lds_bins=lds_bins) for _ in range(2)]
    runs += [sc.by_feature(segment_rows=s, lds_bins=lds_bins) for s in (64, 256, 8192)]  # 8192: 256 bitmap words
    runs.append(sc.by_feature(segment_rows=C.SEGMENT_ROWS, lds_bins=lds_bins, rows_per_block=32))
    torch.cuda.synchronize()
    for got in runs:
        assert got.row.is_cuda and got.n_rows == ref.n_rows and got.n == ref.n and got.cap == ref.cap
        _same(got, ref)
    _same(sc.by_feature(), ref)   # the defaults


def _buffers(cap, pad=64):
    fr = torch.full((G * cap + pad,), ROW_SENTINEL, device=DEV, dtype=torch.int32)
    fv = torch.full((G * cap + pad,), VAL_SENTINEL, device=DEV, dtype=torch.float32)
    return fr, fv, fr[: G * cap].view(G, cap), fv[: G * cap].view(G, cap)


@pytest.mark.parametrize("lds_bins", [8192, 64], ids=["lds", "global"])
def test_undersized_buffers_keep_the_prefix_and_write_nothing_outside(case, lds_bins):
    from sparse_coding__amd.ops import feature_codes as fc_ops

    sc, ref = case
    total = ref.col_ptr[:, -1].tolist()
    for cap_out in (sc.cap, sc.cap - 1, sc.cap // 2, 0):
        fr, fv, row, val = _buffers(cap_out)
        col_ptr, _, _, skipped = fc_ops.by_feature(sc.row_ptr, sc.col, sc.val, sc.n, segment_rows=C.SEGMENT_ROWS,
                                                   lds_bins=lds_bins, out=(row, val))
        torch.cuda.synchronize()
        assert torch.equal(col_ptr.cpu(), ref.col_ptr) and not skipped.any()   # the true counts
        for g in range(G):
            k = min(total[g], cap_out)
            assert torch.equal(row[g, :k].cpu(), ref.row[g, :k]) and torch.equal(val[g, :k].cpu(), ref.val[g, :k])
            assert bool((row[g, k:] == ROW_SENTINEL).all()) and bool((val[g, k:] == VAL_SENTINEL).all())
        assert bool((fr[G * cap_out:] == ROW_SENTINEL).all()) and bool((fv[G * cap_out:] == VAL_SENTINEL).all())


@pytest.mark.parametrize("lds_bins", [8192, 64], ids=["lds", "global"])
@pytest.mark.parametrize("name", ["decreasing_pointer", "column_at_n", "column_at_nactive", "overflowed_budget"])
def test_skip_rule_on_the_device(name, lds_bins):
    from sparse_coding__amd.engine import feature_codes as fcm

    sc, nactive, lost = C.skip_cases()[name]
    ref = fcm.feature_codes_reference(sc, nactive)
    assert ref.skipped.tolist() == [len(lost.get(g, ())) for g in range(G)]
    got = sc.to(DEV).by_feature(nactive, segment_rows=64, lds_bins=lds_bins)
    torch.cuda.synchronize()
    _same(got, ref)
    with pytest.raises(fcm.FeatureCodesSkipped):
        got.check()


def test_transposition_is_graph_capturable():
    from sparse_coding__amd.engine import feature_codes as fcm

    a = C.codes(C.crafted_dense(128, 128, seed=31))
    b = C.codes(C.crafted_dense(128, 128, seed=32))
    cap = max(a.cap, b.cap)
    pad = lambda t: torch.nn.functional.pad(t, (0, cap - t.shape[1]))
    col, val, rp = pad(a.col).to(DEV), pad(a.val).to(DEV), a.row_ptr.to(DEV)
    from sparse_coding__amd.engine.sparse_codes import SparseCodes

    live = SparseCodes(128, 128, rp, col, val)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        live.by_feature()  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = live.by_feature()
        ex = out.fragment_examples(64, 4, 4, 1)
    col.copy_(pad(b.col))
    val.copy_(pad(b.val))
    rp.copy_(b.row_ptr)
    graph.replay()
    torch.cuda.synchronize()
    ref = fcm.feature_codes_reference(SparseCodes(128, 128, b.row_ptr, pad(b.col), pad(b.val)))
    _same(out, ref)
    assert torch.equal(ex.top_frag.cpu(), ref.fragment_examples(64, 4, 4, 1).top_frag)


# ----------------------------------------------------------------------------- example fragments and records
@pytest.fixture(scope="module", params=[1, 3, 64], ids=lambda L: f"L{L}")
def frag_case(request):
    L = request.param
    dense = C.plant_equal_maxima(C.crafted_dense(384, 640, seed=5), L)
    ref = C.codes(dense).by_feature()
    return L, dense, ref, ref.to(DEV)


@pytest.mark.parametrize("Kt,Kr", [(0, 0), (1, 32), (20, 20), (32, 1)])
def test_fragment_examples_match_oracle(frag_case, Kt, Kr):
    L, _, ref, fc = frag_case
    want = ref.fragment_examples(L, Kt, Kr, 12345)
    got = fc.fragment_examples(L, Kt, Kr, 12345)
    torch.cuda.synchronize()
    for k in ("n_frags", "top_frag", "top_max", "rand_frag"):
        a, b = getattr(got, k), getattr(want, k)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b), k
    F = 384 // L
    if Kt >= 20:   # equal maxima go to the lower fragment; fewer active fragments than K leave (-1, 0.0)
        assert got.top_frag[0, C.F_TIES, :5].tolist() == [0, 1, F - 1, 2, -1]
        assert got.top_max[0, C.F_TIES, :5].tolist() == [500.0, 500.0, 500.0, 3.0, 0.0]
    if L == 64:    # the run of 64 entries at list positions 40 .. 103 is one fragment
        assert ref.feature(0, C.F_STRADDLE)[0][40:104].tolist() == list(range(128, 192))
        assert int(got.n_frags[0, C.F_STRADDLE]) == 4


def test_fragment_acts_match_oracle(frag_case):
    L, dense, ref, fc = frag_case
    n, N = ref.n, ref.n_rows
    ex = ref.fragment_examples(L, 20, 20, 3)
    by_frag = dense.view(G, N // L, L, n)
    for frags in (ex.top_frag, ex.rand_frag):
        got = fc.fragment_acts(frags.to(DEV), fragment_len=L)
        want = ref.fragment_acts(frags, fragment_len=L)
        torch.cuda.synchronize()
        assert got.shape == (G, n, 20, L) and torch.equal(got.cpu(), want)
        g, f = 1, C.F_EVERY
        assert torch.equal(got[g, f, 0].cpu(), by_frag[g, int(frags[g, f, 0]), :, f])
    # a hand-made table (-1, out of range, a silent fragment, fragment 0) on a feature sub-range, into a
    # sentinel-filled output: every element is written
    silent = int(torch.nonzero(by_frag[0, :, :, C.F_TIES].amax(1) == 0)[0])
    frags = torch.tensor([-1, N // L, silent, 0], dtype=torch.int32).expand(G, 4, 4).contiguous()
    feats = slice(C.F_TIES - 1, C.F_TIES + 3)
    want = ref.fragment_acts(frags, feats, L)
    from sparse_coding__amd.ops import feature_codes as fc_ops

    out = torch.full((G, 4, 4, L), -5.0, device=DEV)
    fc_ops.fragment_acts(fc.col_ptr, fc.row, fc.val, N, L, frags.to(DEV), feats.start, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want) and not want[:, :, :2].any() and want[:, :, 3].any()
    assert torch.equal(fc.fragment_acts(frags.to(DEV), feats, L).cpu(), want)


# ----------------------------------------------------------------------------- engines
from test_sparse_codes_gpu import (B_ENG, N_DICT, N_POOL, TK_B, TK_N, _data, _engine, _models, _state_tensors,  # noqa: E402
                                   _topk_case, _topk_models)


def _check_examples(codes, nactive, fc, ex, L, K, seed):
    """``(fc, ex)`` equal the oracles run on the engine's own sparse codes."""
    from sparse_coding__amd.engine import feature_codes as fcm

    ref = fcm.feature_codes_reference(codes.to("cpu"), nactive)
    _same(fc, ref)
    want = ref.fragment_examples(L, K, K, seed)
    for k in ("n_frags", "top_frag", "top_max", "rand_frag"):
        assert torch.equal(getattr(ex, k).cpu(), getattr(want, k)), k
    assert ex.fragment_len == L and ex.seed == seed
    return ref


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_sae_engine_feature_examples(masked):
    from sparse_coding__amd.engine import feature_codes as fcm

    sizes = [128, 256, 256] if masked else None
    sig, models = _models("untied", sizes)
    eng = _engine(sig, models)
    eng.step_batch(_data(seed=2, batches=1))
    pool = _data(seed=1)
    codes = eng.encode_sparse(pool)
    fc, ex = eng.feature_examples(pool, fragment_len=32, n_top=10, n_random=10, seed=4)
    torch.cuda.synchronize()
    assert fc.row.is_cuda and fc.n_rows == N_POOL and fc.n == N_DICT
    _check_examples(codes, sizes, fc, ex, 32, 10, 4)
    fc.check()
    if masked:
        assert not fc.counts()[0, 128:].any() and bool(fc.counts()[1, 128:].any())
    # fire counts: with fragments of one row a fragment is a row
    _, ex1 = eng.feature_examples(pool, fragment_len=1, n_top=0, n_random=0)
    assert torch.equal(ex1.n_frags, eng.feature_stats(pool).count)
    # a budget that is too small: whole rows are skipped and counted, check() raises, nothing faults
    budget = max(1, int(codes.nnz().min()) // N_POOL // 2)
    tight = eng.encode_sparse(pool, budget=budget)
    fct, ext = eng.feature_examples(pool, fragment_len=32, n_top=10, n_random=10, seed=4, budget=budget)
    torch.cuda.synchronize()
    _check_examples(tight, sizes, fct, ext, 32, 10, 4)
    assert bool((fct.skipped > 0).all())
    with pytest.raises(fcm.FeatureCodesSkipped):
        fct.check()
    with pytest.raises(ValueError):
        eng.feature_examples(pool, fragment_len=5)


def test_feature_examples_leave_training_state_alone():
    sig, models = _models("untied")
    a, b = _engine(sig, models).enable_graph(), _engine(sig, models).enable_graph()
    xs = _data(seed=3, batches=2)
    pool = _data(seed=4)
    for e in (a, b):
        e.step_batch(xs[:B_ENG])
    graphs = dict(a._graph)
    a.feature_examples(pool)
    a.feature_examples(pool, fragment_len=32, budget=4)
    for e in (a, b):
        e.step_batch(xs[B_ENG:])
    torch.cuda.synchronize()
    assert set(a._graph) == set(graphs) and all(a._graph[k] is g for k, g in graphs.items())
    assert a.step_count == b.step_count == 2 and a.rows_seen == b.rows_seen
    sa, sb = _state_tensors(a), _state_tensors(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_topk_engine_feature_examples():
    from sparse_coding__amd.engine.topk import FusedTopKEnsemble

    W, x = _topk_case()
    eng = FusedTopKEnsemble(_topk_models(W), batch_size=TK_B, device=DEV, lr=1e-3)
    pool = x.to(DEV)
    codes = eng.encode_sparse(pool)
    fc, ex = eng.feature_examples(pool, fragment_len=64, n_top=20, n_random=20, seed=9)
    torch.cuda.synchronize()
    assert fc.n == TK_N and fc.n_rows == pool.shape[0]
    _check_examples(codes, None, fc, ex, 64, 20, 9)
    _, ex1 = eng.feature_examples(pool, fragment_len=1, n_top=0, n_random=0)
    assert torch.equal(ex1.n_frags, eng.feature_stats(pool).count)


def test_trainer_routes_feature_examples():
    from sparse_coding__amd.engine import feature_codes as fcm
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.topk import TopKEncoder

    sig, models = _models("untied")
    pool = _data(seed=5)
    tr = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV)
    assert tr.kind == "fused-sae"
    fc, ex = tr.feature_examples(pool.cpu(), fragment_len=64, n_top=5, n_random=5, seed=2, budget=N_DICT // 2)
    fc2, ex2 = tr.impl.feature_examples(pool, fragment_len=64, n_top=5, n_random=5, seed=2, budget=N_DICT // 2)
    assert isinstance(fc, fcm.FeatureCodes) and fc.row.is_cuda
    _same(fc, fc2)
    assert torch.equal(ex.top_frag, ex2.top_frag) and torch.equal(ex.rand_frag, ex2.rand_frag)
    W, x = _topk_case(n_batches=1, zero_rows=0, seed=102)
    tk = EnsembleTrainer(_topk_models(W), TopKEncoder, lr=1e-3, batch_size=TK_B, device="cuda:0")
    assert tk.kind == "fused-topk"
    fc, ex = tk.feature_examples(x, fragment_len=64)
    _check_examples(tk.encode_sparse(x), None, fc, ex, 64, 20, 0)
    # an eager SAE: the oracles on its torch codes
    eager = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV, engine="eager")
    assert eager.kind == "eager"
    rows = pool.float()
    fc, ex = eager.feature_examples(rows, fragment_len=64, n_top=5, n_random=5)
    _check_examples(eager.encode_sparse(rows), None, fc, ex, 64, 5, 0)


def test_data_parallel_trainer_refuses():
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.signatures import FunctionalSAE

    models = [FunctionalSAE.init(16, 32, 1e-3) for _ in range(2)]
    tr = EnsembleTrainer(models, FunctionalSAE, batch_size=16, device="cpu", engine="eager", parallel="dp")
    with pytest.raises(NotImplementedError, match="data-parallel"):
        tr.feature_examples(torch.randn(64, 16))


@pytest.mark.parametrize("F", [12, 10], ids=["whole_batches", "padded"])
def test_ensemble_example_sets_through_a_masked_fused_trainer(F):
    """One LM pass (a stand-in LM) through the fused trainer: 384 rows are three whole batches, 320 rows are
    padded for the encode and cut back; a masked model never lists a feature at or past its dict size."""
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.interp import activations as A
    from test_sparse_codes_gpu import D

    sizes = [128, 256, 256]
    sig, models = _models("untied", sizes)
    tr = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV)
    assert tr.kind == "fused-sae"
    L, K = 32, 6
    lm = C.TinyLM(D, DEV)
    fragments = torch.randint(0, 50, (F, L), generator=torch.Generator().manual_seed(9))
    sets = A.ensemble_feature_example_sets(lm, tr, 2, "residual", fragments, n_examples=K, seed=3, batch_size=5)
    dense = A.ensemble_feature_activation_datasets(lm, tr, 2, "residual", fragments, batch_size=5)
    assert len(sets) == G
    for g, (es, ds) in enumerate(zip(sets, dense)):
        assert torch.equal(es.n_frags, (ds.maxes > 0).sum(0)) and int(es.n_frags.max()) > 0
        assert not es.n_frags[sizes[g]:].any() and int(es.top_frag.max()) < F
        for f in range(0, N_DICT, 5):
            for table, acts in ((es.top_frag, es.top_acts), (es.rand_frag, es.rand_acts)):
                assert int((table[f] >= 0).sum()) == min(K, int(es.n_frags[f]))
                for j, fr in enumerate(table[f].tolist()):
                    assert torch.equal(acts[f, j], ds.acts[fr, :, f] if fr >= 0 else torch.zeros(L, dtype=torch.float16))


# ----------------------------------------------------------------------------- agreement with the dense dataset
def test_example_sets_agree_with_the_dense_activation_dataset():
    from sparse_coding__amd.engine import feature_codes as fcm
    from sparse_coding__amd.interp import activations as A

    sig, models = _models("untied")
    eng = _engine(sig, models)
    pool = _data(seed=9)
    L, K = 32, 10
    F = N_POOL // L
    tokens = torch.arange(F * L).view(F, L)
    sc = eng.encode_sparse(pool)
    fc, ex = fcm.feature_examples(sc, None, L, K, K, seed=1)
    sets = A.feature_example_sets_from_codes(fc, ex, tokens, feature_chunk=100)
    for g, es in enumerate(sets):
        ds = A.feature_activation_dataset_from_sparse(sc, g, tokens)
        assert torch.equal(es.n_frags, (ds.maxes > 0).sum(0))
        top = torch.topk(ds.maxes.float(), K, dim=0).values.T            # [n, K]
        assert torch.equal(ex.top_max[g].cpu().half().float(), top)
        for f in range(0, N_DICT, 7):
            for table, acts in ((es.top_frag, es.top_acts), (es.rand_frag, es.rand_acts)):
                for k, fr in enumerate(table[f].tolist()):
                    want = ds.acts[fr, :, f] if fr >= 0 else torch.zeros(L, dtype=torch.float16)
                    assert torch.equal(acts[f, k], want), (g, f, k)
                    assert fr < 0 or float(ds.maxes[fr, f]) > 0
