"""Value-ordered feature lists on the MI355X: the kernels of ``csrc/value_order.hip`` against the torch oracles on
the crafted lists of ``value_order_cases.py`` (list lengths around 64 and 128, a 1000-entry list, every value
set, ties across chunks, 32 concepts), the same bits under every geometry, the guards, graph capture, and
``value_order`` / ``feature_auroc`` of the engines and the trainer.  Every comparison is ``torch.equal``."""

import pytest
import torch

import value_order_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 64
ROW_MARK, VAL_MARK = -77, -123.0          # what the sort's outputs hold before the launch
POS_MARK, U2_MARK = -7, -9                # no count is negative


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_coding__amd.ops import _lib as L

    L.lib()  # must load: no silent fallback on a GPU box
    yield


def _padded(shape, mark, dtype):
    """A ``mark``-filled buffer of ``shape`` cut from a flat one with PAD spare words on either side."""
    flat = torch.full((torch.Size(shape).numel() + 2 * PAD,), mark, device=DEV, dtype=dtype)
    return flat, flat[PAD:flat.numel() - PAD].view(shape)


def _canaries_intact(flat, mark):
    return bool((flat[:PAD] == mark).all()) and bool((flat[-PAD:] == mark).all())


def _sort(cp, row, val, cap_out=None, waves=4):
    """One launch into marked outputs: (vrow, vval) on the host, canaries checked, inputs unchanged."""
    from sparse_coding__amd.ops import value_order as vo_ops

    Gm, cap = row.shape
    cap_out = cap if cap_out is None else cap_out
    frow, orow = _padded((Gm, cap_out), ROW_MARK, torch.int32)
    fval, oval = _padded((Gm, cap_out), VAL_MARK, torch.float32)
    drow, dval = row.to(DEV), val.to(DEV)
    vo_ops.sort_lists(cp.to(DEV), drow, dval, out=(orow, oval), waves=waves)
    torch.cuda.synchronize()
    assert _canaries_intact(frow, ROW_MARK) and _canaries_intact(fval, VAL_MARK)
    assert torch.equal(drow.cpu(), row) and torch.equal(C.bits(dval.cpu()), C.bits(val))
    return orow.cpu(), oval.cpu()


def _sort_want(cp, row, val, cap_out=None):
    from sparse_coding__amd.engine.value_order import sort_lists_reference

    cap_out = row.shape[1] if cap_out is None else cap_out
    out = (torch.full((row.shape[0], cap_out), ROW_MARK, dtype=torch.int32),
           torch.full((row.shape[0], cap_out), VAL_MARK, dtype=torch.float32))
    return sort_lists_reference(cp, row, val, out=out)


# ----------------------------------------------------------------------------- the sort
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "N%d-n%d" % s)
def test_sort_matches_oracle_under_every_geometry(shape, kind):
    fc = C.lists(*shape, kind)
    want = _sort_want(fc.col_ptr, fc.row, fc.val)
    assert bool((want[0][:, -C.TAIL:] == ROW_MARK).all())            # the tail is not the kernel's to write
    for waves in (1, 4, 2, 4):
        C.same_lists(_sort(fc.col_ptr, fc.row, fc.val, waves=waves), want)


def test_by_value_on_device_lists():
    from sparse_coding__amd.engine import value_order as vo

    for kind in ("bf16", "fp32"):
        fc = C.lists(1024, 70, kind)
        got = fc.to(DEV).by_value()
        assert isinstance(got, vo.ValueOrdered) and got.row.is_cuda and got.n_rows == 1024
        want = fc.by_value()
        C.same_lists((got.row, got.val), (want.row, want.val))       # the default outputs: a zero tail
        for Q in (1, 10):
            a, b = got.quantiles(Q).cpu(), want.quantiles(Q)
            assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())
        edges = torch.tensor([0.0, 0.5, 1.0, 2.0, 400.0])
        assert torch.equal(got.histogram(edges.to(DEV)).cpu(), want.histogram(edges))
        for a, b in zip(got.strata(4, 3), want.strata(4, 3)):
            assert torch.equal(a.cpu(), b)


def test_sort_guards_keep_every_access_in_bounds():
    """Pointers past ``cap``, negative and non-monotone ones, and outputs shorter than the inputs: the oracle's
    stated lists, everything else untouched."""
    fc = C.lists(1024, 70, "three")
    cp = C.guard_pointers(fc)
    for cap_out in (fc.cap, fc.cap - 700, 100):
        want = _sort_want(cp, fc.row, fc.val, cap_out)
        for waves in (1, 4):
            C.same_lists(_sort(cp, fc.row, fc.val, cap_out, waves), want)
    want = _sort_want(fc.col_ptr, fc.row, fc.val, fc.cap - 700)
    C.same_lists(_sort(fc.col_ptr, fc.row, fc.val, fc.cap - 700), want)
    from sparse_coding__amd.ops import value_order as vo_ops

    dev = fc.to(DEV)
    with pytest.raises(ValueError, match="in place"):
        vo_ops.sort_lists(dev.col_ptr, dev.row, dev.val, out=(dev.row, dev.val))
    with pytest.raises(ValueError, match="waves"):
        vo_ops.sort_lists(dev.col_ptr, dev.row, dev.val, waves=3)


# ----------------------------------------------------------------------------- the AUROC walk
def _auroc(cp, vrow, vval, fl, K, waves=4):
    """One launch into marked outputs: (pos_in, u2) on the host; every slot written, nothing past them."""
    from sparse_coding__amd.ops import value_order as vo_ops

    Gm, n = cp.shape[0], cp.shape[1] - 1
    fpos, pos = _padded((Gm, n, K), POS_MARK, torch.int32)
    fu2, u2 = _padded((Gm, n, K), U2_MARK, torch.int64)
    vo_ops.list_auroc(cp.to(DEV), vrow.to(DEV), vval.to(DEV), fl.to(DEV), K, out=(pos, u2), waves=waves)
    torch.cuda.synchronize()
    assert _canaries_intact(fpos, POS_MARK) and _canaries_intact(fu2, U2_MARK)
    assert not bool((pos == POS_MARK).any()) and not bool((u2 == U2_MARK).any())
    return pos.cpu(), u2.cpu()


@pytest.mark.parametrize("kind", C.POSITIVE)
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "N%d-n%d" % s)
def test_auroc_matches_oracle_under_every_geometry(shape, kind):
    from sparse_coding__amd.engine import value_order as vo

    fc = C.lists(*shape, kind)
    ordered = fc.by_value()
    for K in (1, 3, 32):
        fl = C.flags(shape[0], K)
        want = vo.list_auroc_reference(ordered.col_ptr, ordered.row, ordered.val, fl, K)
        for waves in (1, 4, 2, 4):
            got = _auroc(ordered.col_ptr, ordered.row, ordered.val, fl, K, waves)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (K, waves)
        res = ordered.to(DEV).auroc(fl.to(DEV), K)
        assert res.u2.is_cuda and res.auroc().dtype == torch.float64
        C.same_auroc(res, ordered.auroc(fl, K))
    if shape[1] == 70:
        a = res.auroc().cpu()
        assert bool((a[0, 0, [0, 31]] == 0.5).all()) and bool(a[..., 1].isnan().all()) and bool(a[..., 2].isnan().all())
        assert res.cnt[1, C.F_ALL].item() == shape[0]


def test_auroc_guards_keep_every_access_in_bounds():
    """Rows outside [0, N) in the busiest lists and broken pointers: the oracle's stated behaviour."""
    from sparse_coding__amd.engine import value_order as vo

    fc = C.lists(512, 70, "three")
    ordered = fc.by_value()
    row = ordered.row.clone()
    for g, f, at, bad in ((0, 9, 0, 512), (0, 9, 64, -1), (0, 9, 65, 2 ** 31 - 1), (1, C.F_ALL, 63, 600),
                          (1, C.F_200, 128, -2 ** 31)):
        row[g, fc.host_ptr()[g][f] + at] = bad
    fl = C.flags(512, 32)
    for cp in (fc.col_ptr, C.guard_pointers(fc)):
        want = vo.list_auroc_reference(cp, row, ordered.val, fl, 32)
        for waves in (1, 4):
            got = _auroc(cp, row, ordered.val, fl, 32, waves)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        broken = vo.ValueOrdered(512, 70, cp, row, ordered.val, fc.skipped)
        C.same_auroc(broken.to(DEV).auroc(fl.to(DEV)), broken.auroc(fl))

def test_by_feature_by_value_and_auroc_are_graph_capturable():
    import feature_codes_cases as FC
    from sparse_coding__amd.engine import value_order as vo

    sc = FC.codes(FC.crafted_dense(384, 640, seed=3))
    fl = C.flags(384, 32)
    dev, dfl = sc.to(DEV), fl.to(DEV)

    def run():
        ordered = dev.by_feature().by_value()
        return ordered, ordered.auroc(dfl, 32)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ordered, res = run()
    graph.replay()
    torch.cuda.synchronize()
    want = vo.value_order(sc, kernels=False)
    C.same_lists((ordered.row, ordered.val), (want.row, want.val))
    C.same_auroc(res, want.auroc(fl, 32))


# ----------------------------------------------------------------------------- engines
from test_sparse_codes_gpu import (B_ENG, N_DICT, N_POOL, TK_B, TK_N, _data, _engine, _models, _state_tensors,  # noqa: E402
                                   _topk_case, _topk_models)


def _check_engine(codes, nactive, ordered, res, fl, K):
    """``ordered`` / ``res`` equal the oracles run on the engine's own sparse codes, which are bf16-valued."""
    from sparse_coding__amd.engine import value_order as vo

    host = codes.to("cpu")
    assert torch.equal(host.val, host.val.to(torch.bfloat16).float())
    want = vo.value_order(host, nactive, kernels=False)
    assert ordered.row.is_cuda and torch.equal(ordered.col_ptr.cpu(), want.col_ptr)
    C.same_lists((ordered.row, ordered.val), (want.row, want.val))
    C.same_auroc(res, vo.feature_auroc(host, fl.cpu(), K, nactive, kernels=False))
    return want


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_sae_engine_value_order_and_auroc(masked):
    from sparse_coding__amd.engine.sparse_codes import SparseCodesOverflow

    sizes = [128, 256, 256] if masked else None
    sig, models = _models("untied", sizes)
    eng = _engine(sig, models)
    eng.step_batch(_data(seed=2, batches=1))
    pool = _data(seed=1)
    fl = C.flags(N_POOL, 32)
    codes = eng.encode_sparse(pool)
    ordered = eng.value_order(pool)
    res = eng.feature_auroc(pool, fl.to(DEV))
    torch.cuda.synchronize()
    assert res.u2.shape == (len(models), N_DICT, 32) and res.n_rows == N_POOL
    want = _check_engine(codes, sizes, ordered, res, fl, 32)
    assert int(want.col_ptr[:, -1].min()) > 0 and want.skipped.tolist() == [0] * len(models)
    a = res.auroc()
    live = ~a.isnan()
    assert bool(((a[live] >= 0) & (a[live] <= 1)).all()) and bool((a[live] != 0.5).any())
    if masked:
        assert bool(ordered.quantiles(4)[0, 128:].isnan().all()) and bool((a[0, 128:, 0] == 0.5).all())
        assert not bool(ordered.quantiles(4)[1, 128:].isnan().all())
    budget = max(1, int(codes.nnz().min()) // N_POOL // 2)
    with pytest.raises(SparseCodesOverflow):
        eng.feature_auroc(pool, fl, budget=budget)
    assert int(eng.value_order(pool, budget=budget).skipped.sum()) > 0


def test_value_order_leaves_training_state_alone():
    sig, models = _models("untied")
    a, b = _engine(sig, models).enable_graph(), _engine(sig, models).enable_graph()
    xs = _data(seed=3, batches=2)
    pool = _data(seed=4)
    fl = C.flags(N_POOL, 3)
    for e in (a, b):
        e.step_batch(xs[:B_ENG])
    graphs = dict(a._graph)
    a.value_order(pool)
    a.feature_auroc(pool, fl, n_concepts=3)
    for e in (a, b):
        e.step_batch(xs[B_ENG:])
    torch.cuda.synchronize()
    assert set(a._graph) == set(graphs) and all(a._graph[k] is g for k, g in graphs.items())
    assert a.step_count == b.step_count == 2 and a.rows_seen == b.rows_seen
    sa, sb = _state_tensors(a), _state_tensors(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_topk_engine_value_order_and_auroc():
    from sparse_coding__amd.engine.topk import FusedTopKEnsemble

    W, x = _topk_case(n_batches=1)
    eng = FusedTopKEnsemble(_topk_models(W), batch_size=TK_B, device=DEV, lr=1e-3)
    pool = x.to(DEV)
    fl = C.flags(pool.shape[0], 3)
    codes = eng.encode_sparse(pool)
    ordered, res = eng.value_order(pool), eng.feature_auroc(pool, fl, n_concepts=3)
    torch.cuda.synchronize()
    assert res.u2.shape[1:] == (TK_N, 3)
    want = _check_engine(codes, None, ordered, res, fl, 3)
    assert int(want.counts()[:, 0].min()) > 64                       # atom 0 fires on every non-zero row


def test_trainer_routes_value_order_and_auroc():
    from sparse_coding__amd.engine import value_order as vo
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.topk import TopKEncoder

    sig, models = _models("untied")
    pool = _data(seed=5)
    fl = C.flags(N_POOL, 3)
    tr = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV)
    assert tr.kind == "fused-sae"
    ordered, res = tr.value_order(pool.cpu()), tr.feature_auroc(pool.cpu(), fl, n_concepts=3)
    assert isinstance(ordered, vo.ValueOrdered) and isinstance(res, vo.FeatureAuroc) and res.u2.is_cuda
    _check_engine(tr.encode_sparse(pool), None, ordered, res, fl, 3)
    W, x = _topk_case(n_batches=1, zero_rows=0, seed=102)
    tk = EnsembleTrainer(_topk_models(W), TopKEncoder, lr=1e-3, batch_size=TK_B, device="cuda:0")
    assert tk.kind == "fused-topk"
    fl = C.flags(x.shape[0], 3)
    _check_engine(tk.encode_sparse(x), None, tk.value_order(x), tk.feature_auroc(x, fl, n_concepts=3), fl, 3)
    # an eager SAE: the oracles on its torch codes, on the device
    eager = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV, engine="eager")
    assert eager.kind == "eager"
    rows = pool.float()
    fl = C.flags(N_POOL, 3)
    host = eager.encode_sparse(rows).to("cpu")
    want = vo.value_order(host, kernels=False)
    got = eager.value_order(rows)
    C.same_lists((got.row, got.val), (want.row, want.val))
    C.same_auroc(eager.feature_auroc(rows, fl, n_concepts=3), want.auroc(fl, 3))


def test_data_parallel_trainer_refuses():
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.signatures import FunctionalSAE

    models = [FunctionalSAE.init(16, 32, 1e-3) for _ in range(2)]
    tr = EnsembleTrainer(models, FunctionalSAE, batch_size=16, device="cpu", engine="eager", parallel="dp")
    with pytest.raises(NotImplementedError, match="data-parallel"):
        tr.value_order(torch.randn(64, 16))
    with pytest.raises(NotImplementedError, match="data-parallel"):
        tr.feature_auroc(torch.randn(64, 16), torch.zeros(64, dtype=torch.int32))
