"""Co-activation partners on the MI355X: the kernels of ``csrc/coactivation.hip`` against the torch oracle on the
crafted inputs of ``coactivation_cases.py`` (list and row lengths around 64, ties, negative and zero scores,
both instantiations, several windows per model, the skip rule, the widest target), and ``coactivation`` of the
engines and the trainer.  Every comparison is ``torch.equal``; every kernel case runs twice."""

import pytest
import torch

import coactivation_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = C.G
SENTINELS = (-7, -3.0, -9, -5.0)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_coding__amd.ops import _lib as L

    L.lib()  # must load: no silent fallback on a GPU box
    yield


def _twice(fn):
    runs = [fn(), fn()]
    torch.cuda.synchronize()
    return runs


# ----------------------------------------------------------------------------- the two kernels
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "N%d-na%d-nb%d" % s)
def test_list_moments_and_the_shift_scale_vectors_match_oracle(shape):
    from sparse_coding__amd.engine import coactivation as co
    from sparse_coding__amd.engine.feature_codes import feature_codes_reference
    from sparse_coding__amd.ops import coactivation as co_ops

    sc_a, sc_b, _ = C.case(*shape)
    for sc in (sc_a, sc_b):
        ref = feature_codes_reference(sc)
        want = co.list_moments_reference(ref)
        fc = ref.to(DEV)
        for got in _twice(lambda: co_ops.list_moments(fc.col_ptr, fc.row, fc.val)):
            for a, b in zip(got, want):
                assert a.dtype == b.dtype and torch.equal(a.cpu(), b)
            for score in C.SCORES:   # fp64 torch ops on the device round as on the host
                for name, a, b in zip(("shift", "scale"), co.shift_scale(*got, sc.n_rows, score),
                                      co.shift_scale(*want, sc.n_rows, score)):
                    assert a.dtype == torch.float32 and torch.equal(a.cpu(), b), (score, name, int((a.cpu() != b).sum()))


@pytest.mark.parametrize("score", C.SCORES)
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "N%d-na%d-nb%d" % s)
def test_coactivation_matches_oracle(shape, score):
    from sparse_coding__amd.engine import coactivation as co

    N = shape[0]
    sc_a, sc_b, sums = C.case(*shape)
    a, b = sc_a.to(DEV), sc_b.to(DEV)
    for m, min_both in ((32, 1), (4, 2), (1, 1), (4, N + 1), (0, 1)):
        want = co.coactivation_reference(sc_a, sc_b, m=m, score=score, min_both=min_both, sums=sums)
        for got in _twice(lambda: co.coactivation(a, b, m=m, score=score, min_both=min_both)):
            assert got.partner.is_cuda and got.partner.shape == (G, G, shape[1], m)
            C.same(got, want)
    assert torch.equal(a.coactivation(b, m=4, score=score, exclude_self=False).partner.cpu(),
                       co.coactivation_reference(sc_a, sc_b, m=4, score=score, sums=sums).partner)


def _launch(sc_a, sc_b, score, m, min_both=1, exclude_self=False, nactive_b=None, **kw):
    """One ``coactivation_topm`` launch on the oracle's own lists and vectors, into sentinel-filled outputs."""
    from sparse_coding__amd.engine import coactivation as co
    from sparse_coding__amd.engine.feature_codes import feature_codes_reference
    from sparse_coding__amd.ops import coactivation as co_ops

    fa, fb = feature_codes_reference(sc_a), feature_codes_reference(sc_b, nactive_b)
    ca, s1, s2 = co.list_moments_reference(fa)
    sha, sca = co.shift_scale(ca, s1, s2, sc_a.n_rows, score)
    cb, s1, s2 = co.list_moments_reference(fb)
    shb, scb = co.shift_scale(cb, s1, s2, sc_a.n_rows, score)
    shape = (fa.n_models, fb.n_models, fa.n, m)
    pad = 64
    flat = [torch.full((fa.n_models * fb.n_models * fa.n * m + pad,), v, device=DEV,
                       dtype=torch.int32 if isinstance(v, int) else torch.float32) for v in SENTINELS]
    out = tuple(t[:t.numel() - pad].view(shape) for t in flat)
    d = lambda t: t.to(DEV)
    live = None if nactive_b is None else torch.tensor(nactive_b, dtype=torch.int32, device=DEV)
    got = co_ops.coactivation_topm(d(fa.col_ptr), d(fa.row), d(fa.val), d(sc_b.row_ptr), d(sc_b.col), d(sc_b.val),
                                   sc_b.n, d(sha), d(sca), d(ca), d(shb), d(scb), d(cb), m, score, min_both,
                                   exclude_self, live, out=out, **kw)
    torch.cuda.synchronize()
    for t, v in zip(flat, SENTINELS):
        assert bool((t[t.numel() - pad:] == v).all())      # nothing is written past the outputs
    return got


@pytest.mark.parametrize("geometry", [{"window": 64, "waves": 1}, {"window": 64, "waves": 4}, {"waves": 1},
                                      {"window": 37, "waves": 2}], ids=lambda g: "-".join(f"{k}{v}" for k, v in g.items()))
@pytest.mark.parametrize("score", ["pearson", "jaccard"])
def test_every_slot_is_written_under_any_geometry(score, geometry):
    """n_b = 100 in windows of 64 and 37 columns (two and three walks per list), one to four waves per block."""
    from sparse_coding__amd.engine import coactivation as co

    sc_a, sc_b, sums = C.case(*C.SHAPES[0])
    for m, min_both in ((32, 1), (4, 2)):
        want = co.coactivation_reference(sc_a, sc_b, m=m, score=score, min_both=min_both, sums=sums)
        for _ in range(2):
            got = _launch(sc_a, sc_b, score, m, min_both, **geometry)
            for t, k in zip(got, ("partner", "score", "both", "dot")):
                assert torch.equal(t.cpu(), getattr(want, k)), k


@pytest.mark.parametrize("score", C.SCORES)
def test_self_comparison_excludes_only_the_own_column(score):
    from sparse_coding__amd.engine import coactivation as co

    sc, sums = C.self_case()
    dev = sc.to(DEV)
    other = sc.to(DEV)
    for m in (4, 32):
        want_on = co.coactivation_reference(sc, m=m, score=score, sums=sums)
        want_off = co.coactivation_reference(sc, m=m, score=score, exclude_self=False, sums=sums)
        for got in _twice(lambda: dev.coactivation(m=m, score=score)):
            C.same(got, want_on)
        for got in _twice(lambda: dev.coactivation(m=m, score=score, exclude_self=False)):
            C.same(got, want_off)
        for got in _twice(lambda: dev.coactivation(other, m=m, score=score)):     # another object: nothing excluded
            C.same(got, want_off)
    if score == "pearson":   # the constant feature: scale 0, every score +0.0, partners by column
        got = dev.coactivation(m=32, score=score)
        s = got.score[0, 0, C.B_CONST].cpu()
        assert not s.any() and not (torch.copysign(torch.ones(32), s) < 0).any()
        assert got.partner[0, 0, C.B_CONST].tolist() == [j for j in range(33) if j != C.B_CONST]


@pytest.mark.parametrize("score", ["cosine", "jaccard"])
def test_a_column_past_nactive_leaves_its_row_out(score):
    from sparse_coding__amd.engine import coactivation as co

    sc_a, sc_b, nactive = C.nactive_case()
    want = co.coactivation_reference(sc_a, sc_b, m=4, score=score, nactive_b=nactive)
    assert want.skipped_b.tolist() == [0, 0, 1]
    for got in _twice(lambda: co.coactivation(sc_a.to(DEV), sc_b.to(DEV), m=4, score=score, nactive_b=nactive)):
        C.same(got, want)
        with pytest.raises(co.CoActivationSkipped):
            got.check()


@pytest.mark.parametrize("score", ["pearson", "jaccard"])
@pytest.mark.parametrize("name", ["decreasing_pointer", "column_at_n", "column_at_nactive", "overflowed_budget"])
def test_skip_rule_on_the_device(name, score):
    from sparse_coding__amd.engine import coactivation as co

    sc_a, sc_b, nactive, lost = C.skip_targets()[name]
    want = co.coactivation_reference(sc_a, sc_b, m=4, score=score, nactive_b=nactive)
    assert want.skipped_b.tolist() == [len(lost.get(g, ())) for g in range(G)]
    for got in _twice(lambda: co.coactivation(sc_a.to(DEV), sc_b.to(DEV), m=4, score=score, nactive_b=nactive)):
        C.same(got, want)
    # the skip input on both sides
    want = co.coactivation_reference(sc_b, m=4, score=score, nactive_a=nactive)
    for got in _twice(lambda: sc_b.to(DEV).coactivation(m=4, score=score, nactive_a=nactive)):
        C.same(got, want)
        assert torch.equal(got.skipped_a, got.skipped_b)


@pytest.mark.parametrize("score", C.SCORES)
def test_the_widest_target_runs_one_wave_per_block(score):
    from sparse_coding__amd.engine import coactivation as co
    from sparse_coding__amd.ops import coactivation as co_ops

    sc_a, sc_b = C.wide_case()
    assert co_ops.geometry(sc_b.n, score != "jaccard")[1] == 1
    want = co.coactivation_reference(sc_a, sc_b, m=8, score=score)
    assert sorted(set(want.partner.flatten().tolist())) != [-1] and int(want.partner.max()) == sc_b.n - 1
    for got in _twice(lambda: co.coactivation(sc_a.to(DEV), sc_b.to(DEV), m=8, score=score)):
        C.same(got, want)
    got = _launch(sc_a, sc_b, score, 8)
    for t, k in zip(got, ("partner", "score", "both", "dot")):
        assert torch.equal(t.cpu(), getattr(want, k)), k
    from sparse_coding__amd.engine.sparse_codes import SparseCodes

    too_wide = SparseCodes(sc_b.n_rows, sc_b.n + 1, sc_b.row_ptr, sc_b.col, sc_b.val).to(DEV)
    with pytest.raises(ValueError, match="16384"):
        co.coactivation(sc_a.to(DEV), too_wide)


def test_coactivation_is_graph_capturable():
    from sparse_coding__amd.engine import coactivation as co

    sc, sums = C.self_case()
    dev = sc.to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dev.coactivation(m=4)  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = dev.coactivation(m=4)
    graph.replay()
    torch.cuda.synchronize()
    C.same(out, co.coactivation_reference(sc, m=4, sums=sums))


# ----------------------------------------------------------------------------- engines
from test_sparse_codes_gpu import (B_ENG, N_DICT, N_POOL, TK_B, TK_N, _data, _engine, _models, _state_tensors,  # noqa: E402
                                   _topk_case, _topk_models)


def _check_engine(codes, nactive, got, **kw):
    """``got`` equals the oracle run on the engine's own sparse codes, which are bf16-valued."""
    from sparse_coding__amd.engine import coactivation as co

    host = codes.to("cpu")
    assert torch.equal(host.val, host.val.to(torch.bfloat16).float())
    want = co.coactivation_reference(host, nactive_a=nactive, **kw)
    C.same(got, want)
    return want


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_sae_engine_coactivation(masked):
    from sparse_coding__amd.engine import coactivation as co

    sizes = [128, 256, 256] if masked else None
    sig, models = _models("untied", sizes)
    eng = _engine(sig, models)
    eng.step_batch(_data(seed=2, batches=1))
    pool = _data(seed=1)
    codes = eng.encode_sparse(pool)
    got = eng.coactivation(pool, m=4, score="pearson")
    torch.cuda.synchronize()
    assert got.partner.is_cuda and got.partner.shape == (G, G, N_DICT, 4) and got.n_rows == N_POOL
    want = _check_engine(codes, sizes, got, m=4, score="pearson")
    got.check()
    assert int(want.partner.max()) >= 0 and float(got.mean_best().min()) > 0
    if masked:
        assert bool((got.partner[0, :, 128:] == -1).all()) and int(got.partner[:, 0].max()) < 128
        assert bool((got.partner[1, 1, 128:] >= 0).any())
    _check_engine(codes, sizes, eng.coactivation(pool, m=2, score="jaccard", min_both=2), m=2, score="jaccard",
                  min_both=2)
    # a budget that is too small: whole rows are skipped and counted, check() raises, nothing faults
    budget = max(1, int(codes.nnz().min()) // N_POOL // 2)
    tight = eng.encode_sparse(pool, budget=budget)
    got = eng.coactivation(pool, m=4, score="cosine", budget=budget)
    torch.cuda.synchronize()
    _check_engine(tight, sizes, got, m=4, score="cosine")
    assert bool((got.skipped_a > 0).all()) and torch.equal(got.skipped_a, got.skipped_b)
    with pytest.raises(co.CoActivationSkipped):
        got.check()
    with pytest.raises(ValueError):
        eng.coactivation(pool, m=33)


def test_coactivation_leaves_training_state_alone():
    sig, models = _models("untied")
    a, b = _engine(sig, models).enable_graph(), _engine(sig, models).enable_graph()
    xs = _data(seed=3, batches=2)
    pool = _data(seed=4)
    for e in (a, b):
        e.step_batch(xs[:B_ENG])
    graphs = dict(a._graph)
    a.coactivation(pool)
    a.coactivation(pool, m=2, score="jaccard", budget=4)
    for e in (a, b):
        e.step_batch(xs[B_ENG:])
    torch.cuda.synchronize()
    assert set(a._graph) == set(graphs) and all(a._graph[k] is g for k, g in graphs.items())
    assert a.step_count == b.step_count == 2 and a.rows_seen == b.rows_seen
    sa, sb = _state_tensors(a), _state_tensors(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_topk_engine_coactivation():
    from sparse_coding__amd.engine.topk import FusedTopKEnsemble

    W, x = _topk_case(n_batches=1)
    eng = FusedTopKEnsemble(_topk_models(W), batch_size=TK_B, device=DEV, lr=1e-3)
    pool = x.to(DEV)
    codes = eng.encode_sparse(pool)
    got = eng.coactivation(pool, m=4, score="pearson")
    torch.cuda.synchronize()
    assert got.partner.shape == (G, G, TK_N, 4) and got.n_rows == pool.shape[0]
    _check_engine(codes, None, got, m=4, score="pearson")
    got.check()


def test_trainer_routes_coactivation():
    from sparse_coding__amd.engine import coactivation as co
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.topk import TopKEncoder

    sig, models = _models("untied")
    pool = _data(seed=5)
    tr = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV)
    assert tr.kind == "fused-sae"
    got = tr.coactivation(pool.cpu(), m=3, score="cosine", budget=N_DICT // 2)
    got2 = tr.impl.coactivation(pool, m=3, score="cosine", budget=N_DICT // 2)
    assert isinstance(got, co.CoActivation) and got.partner.is_cuda
    C.same(got, got2)
    W, x = _topk_case(n_batches=1, zero_rows=0, seed=102)
    tk = EnsembleTrainer(_topk_models(W), TopKEncoder, lr=1e-3, batch_size=TK_B, device="cuda:0")
    assert tk.kind == "fused-topk"
    _check_engine(tk.encode_sparse(x), None, tk.coactivation(x, m=2, score="jaccard"), m=2, score="jaccard")
    # an eager SAE: the oracle on its torch codes
    eager = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV, engine="eager")
    assert eager.kind == "eager"
    rows = pool.float()
    got = eager.coactivation(rows, m=2)
    C.same(got, co.coactivation_reference(eager.encode_sparse(rows), m=2))


def test_data_parallel_trainer_refuses():
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.signatures import FunctionalSAE

    models = [FunctionalSAE.init(16, 32, 1e-3) for _ in range(2)]
    tr = EnsembleTrainer(models, FunctionalSAE, batch_size=16, device="cpu", engine="eager", parallel="dp")
    with pytest.raises(NotImplementedError, match="data-parallel"):
        tr.coactivation(torch.randn(64, 16))
