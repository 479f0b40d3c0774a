"""Label profiles on the MI355X: the kernels of ``csrc/label_profile.hip`` against the torch oracle on the crafted
inputs of ``label_profile_cases.py`` (list lengths around 64, 64 runs in a pass, runs across passes, ties, the
order-sensitive sums, labels up to 2^31 - 2), the guards, and ``label_profile`` of the engines and the trainer.
Every comparison is ``torch.equal``."""

import pytest
import torch

import feature_codes_cases as FC
import label_profile_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = C.G
CASE_IDS = ["N%d-n%d-%s" % c for c in C.CASES]
SENTINELS = (-7, -9, -11, -3.0, -13, -15, -5.0, -17.0)       # one per output, none a value the kernel writes


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_coding__amd.ops import _lib as L

    L.lib()  # must load: no silent fallback on a GPU box
    yield


# ----------------------------------------------------------------------------- take_rows
def _rows_case():
    """Codes with rows of 0, 1, 64 and 65 entries (and the crafted full row of model 1) and an index with
    duplicates, the crafted rows first."""
    dense = FC.crafted_dense(128, 128, seed=21)
    gen = torch.Generator().manual_seed(22)
    for r, k in ((10, 0), (11, 1), (12, 64), (13, 65)):
        dense[:, r] = 0
        for g in range(G):
            dense[g, r, torch.randperm(128, generator=gen)[:k]] = 1.5
    index = torch.cat([torch.tensor([13, 10, 11, 12, 13, 13, FC.FULL_ROW, FC.EMPTY_ROW, 0, 127]),
                       torch.randint(0, 128, (290,), generator=gen)])
    return FC.codes(dense), index


def test_take_rows_matches_oracle():
    from sparse_coding__amd.engine.sparse_codes import take_rows_reference

    sc, index = _rows_case()
    want = take_rows_reference(sc, index)
    assert sorted(set((want.row_ptr[0, 1:5] - want.row_ptr[0, 0:4]).tolist())) == [0, 1, 64, 65]
    dev = sc.to(DEV)
    for waves in (1, 2, 4):
        got = dev.take_rows(index.to(DEV), waves=waves)
        assert got.col.is_cuda and got.n_rows == index.numel() and got.cap == want.cap
        for k in ("row_ptr", "col", "val"):
            assert torch.equal(getattr(got, k).cpu(), getattr(want, k)), (waves, k)
    a, b = dev.narrow_rows(17, 90), dev.take_rows(torch.arange(17, 90, device=DEV))
    for k in ("row_ptr", "col", "val"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert dev.take_rows(torch.zeros(0, dtype=torch.int64)).n_rows == 0
    with pytest.raises(IndexError):
        dev.take_rows(torch.tensor([128]))


def test_take_rows_kernel_rechecks_its_bounds():
    """A row whose pointers decrease and an index past the rows are written as empty; a ``cap_out`` that ends
    inside a row cuts it there; the words behind the buffers keep their value."""
    from sparse_coding__amd.ops import sparse_codes as sc_ops

    sc, _ = _rows_case()
    rp = sc.row_ptr.clone()
    rp[1, 13] = rp[1, 12] - 1                       # row 12 of model 1 ends before it starts; row 13 starts there
    index = torch.tensor([12, 13, 500, -3, 11, 14])
    lens = torch.stack([(sc.row_ptr[g, 1:] - sc.row_ptr[g, :-1])[index.clamp(0, 127)] for g in range(G)])
    out_ptr = torch.zeros(G, 7, dtype=torch.int64)
    out_ptr[:, 1:] = torch.cumsum(lens, 1)
    cap_out = int(out_ptr[:, 5].max()) + 1         # ends one entry into the last row of the fullest model
    col, val = sc_ops.take_rows(rp.to(DEV), sc.col.to(DEV), sc.val.to(DEV), index.to(DEV), out_ptr.to(DEV), cap_out)
    torch.cuda.synchronize()
    col, val = col.cpu(), val.cpu()
    for g in range(G):
        for i, r in enumerate(index.tolist()):
            lo, hi = int(out_ptr[g, i]), min(int(out_ptr[g, i + 1]), cap_out)
            if 0 <= r < 128 and rp[g, r] <= rp[g, r + 1]:
                s = int(rp[g, r])                   # (row 13 of model 1 starts early: cut at the next row's start)
                assert torch.equal(col[g, lo:hi], sc.col[g, s:s + hi - lo]), (g, i)
                assert torch.equal(val[g, lo:hi], sc.val[g, s:s + hi - lo]), (g, i)
            else:
                assert not col[g, lo:hi].any() and not val[g, lo:hi].any(), (g, i)


# ----------------------------------------------------------------------------- the kernel against the oracle
@pytest.mark.parametrize("rank_by", C.RANKS)
@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_label_profile_matches_oracle(case, rank_by):
    from sparse_coding__amd.engine import label_profile as lp

    sc, labels, n_classes, _, _ = C.case(*case)
    dev, lab = sc.to(DEV), labels.to(DEV)
    for m in (1, 8, 64):
        want = C.reference(*case, m, rank_by)
        got = lp.label_profile(dev, lab, m=m, rank_by=rank_by, n_classes=n_classes)
        assert got.top_label.is_cuda and got.top_label.shape == (G, case[1], m)
        C.same(got, want)
    got = dev.label_profile(labels.to(torch.int32), m=8, rank_by=rank_by, n_classes=n_classes)   # int32, on the host
    C.same(got, C.reference(*case, 8, rank_by))
    if rank_by == "sum":
        assert got.top_sum[:, C.F_ORDER_A, 0].tolist() == [C.ORDER_SUM_A] * G
        assert got.top_sum[:, C.F_ORDER_B, 0].tolist() == [C.ORDER_SUM_B] * G


def _lists(case):
    """The label-ordered feature lists of a case and their labels, built by the oracles on the host."""
    from sparse_coding__amd.engine.feature_codes import feature_codes_reference
    from sparse_coding__amd.engine.sparse_codes import take_rows_reference

    sc, labels, _, _, _ = C.case(*case)
    kept = torch.nonzero(labels >= 0).flatten()
    lab, order = torch.sort(labels[kept], stable=True)
    return feature_codes_reference(take_rows_reference(sc, kept[order])), lab.to(torch.int32)


def _launch(col_ptr, row, val, lab, m, rank_by, waves=4):
    """One kernel launch into sentinel-filled outputs cut from flat buffers with spare words behind them."""
    from sparse_coding__amd.ops import label_profile as lp_ops

    Gm, n = col_ptr.shape[0], col_ptr.shape[1] - 1
    dts = (torch.int64, torch.int32, torch.int64, torch.float64, torch.int32, torch.int32, torch.float64, torch.float32)
    shapes = [(Gm, n)] * 4 + [(Gm, n, m)] * 4
    pad = 64
    flat = [torch.full((torch.Size(s).numel() + pad,), v, device=DEV, dtype=dt) for s, v, dt in zip(shapes, SENTINELS, dts)]
    out = tuple(t[:t.numel() - pad].view(s) for t, s in zip(flat, shapes))
    d = lambda t: t.to(DEV)
    got = lp_ops.label_profile(d(col_ptr), d(row), d(val), d(lab), m, rank_by, waves=waves, out=out)
    torch.cuda.synchronize()
    for t, v, o in zip(flat, SENTINELS, got):
        assert bool((t[t.numel() - pad:] == v).all())        # nothing is written past the outputs
        assert not bool((o == v).any())                       # every element is written
    return tuple(t.cpu() for t in got)


@pytest.mark.parametrize("case", [(128, 128, "sparse"), (384, 640, "L5")], ids=["N128-sparse", "N384-L5"])
def test_same_bits_twice_and_under_any_geometry_and_every_slot_written(case):
    from sparse_coding__amd.engine import label_profile as lp

    fc, lab = _lists(case)
    for rank_by in C.RANKS:
        for m in (1, 64):
            ref = C.reference(*case, m, rank_by)
            want = tuple(getattr(ref, k) for k in C.FIELDS)
            C.same_tuple(want, lp.profile_lists_reference(fc.col_ptr, fc.row, fc.val, lab, m, rank_by))
            for waves in (1, 2, 4, 4):
                C.same_tuple(_launch(fc.col_ptr, fc.row, fc.val, lab, m, rank_by, waves), want)


def test_guards_keep_every_access_in_bounds():
    """A decreasing ``col_ptr``, pointers outside [0, cap], rows outside [0, M) in a list: the oracle's stated
    behaviour (clipped lists, skipped entries).  An unsorted ``lab``: more runs, the totals of the entries."""
    from sparse_coding__amd.engine import label_profile as lp

    fc, lab = _lists((128, 128, "L70"))
    M = lab.numel()
    cp, row = fc.col_ptr.clone(), fc.row.clone()
    cp[0, 40] = cp[0, 39] - 3                  # list 39 ends before it starts: empty; list 40 starts earlier
    cp[1, 0] = -5
    cp[1, -1] = fc.cap + 1000
    cp[2, 7] = fc.cap + 9
    for g in range(G):                          # rows >= M, negative rows and INT32_MAX in the busiest lists
        lo = int(fc.col_ptr[g, C.F_EVERY])
        row[g, lo + 3], row[g, lo + 64], row[g, lo + 65] = M, -1, 2 ** 31 - 1
        lo = int(fc.col_ptr[g, C.F_65])
        row[g, lo], row[g, lo + 64] = M + 7, M
    for rank_by in C.RANKS:
        want = lp.profile_lists_reference(cp, row, fc.val, lab, 8, rank_by)
        assert want[0][0, C.F_EVERY].item() == M - 3 and want[0][0, 39].item() == 0
        for waves in (1, 4):
            C.same_tuple(_launch(cp, row, fc.val, lab, 8, rank_by, waves), want)
    shuffled = lab[torch.randperm(M, generator=torch.Generator().manual_seed(6))].contiguous()
    ref = lp.profile_lists_reference(fc.col_ptr, fc.row, fc.val, lab, 64, "count")
    got = _launch(fc.col_ptr, fc.row, fc.val, shuffled, 64, "count")
    assert torch.equal(got[0], ref[0]) and bool((got[1] <= got[0]).all())
    for g in range(G):                          # at least as many runs as the list has distinct labels, here more
        for f in (C.F_EVERY, C.F_65, C.F_64):
            lo, hi = int(fc.col_ptr[g, f]), int(fc.col_ptr[g, f + 1])
            distinct = shuffled[fc.row[g, lo:hi].long()].unique().numel()
            assert got[1][g, f].item() >= distinct
        assert got[1][g, C.F_EVERY].item() > 70
    assert int(got[4].max()) <= int(lab.max()) and int(got[4].min()) >= -1
    assert torch.equal(got[5].sum(-1).long().clamp(max=got[0]), got[5].sum(-1).long())
    C.same_tuple(got, lp.profile_lists_reference(fc.col_ptr, fc.row, fc.val, shuffled, 64, "count"))


def test_masked_model_on_the_device():
    from sparse_coding__amd.engine import label_profile as lp

    sc, labels, nactive = C.masked_case()
    want = lp.label_profile_reference(sc, labels, m=8, nactive=nactive, n_classes=5)
    assert want.skipped.tolist() == [0, 0, 1]
    C.same(lp.label_profile(sc.to(DEV), labels.to(DEV), m=8, nactive=nactive, n_classes=5), want)


def test_by_feature_and_the_kernel_are_graph_capturable():
    from sparse_coding__amd.engine.sparse_codes import take_rows_reference
    from sparse_coding__amd.ops import label_profile as lp_ops

    case = (128, 128, "L70")
    sc, labels, _, _, _ = C.case(*case)
    kept = torch.nonzero(labels >= 0).flatten()
    lab, order = torch.sort(labels[kept], stable=True)
    taken = take_rows_reference(sc, kept[order]).to(DEV)      # complete codes: nothing below synchronises
    lab = lab.to(DEV, torch.int32)

    def run():
        fc = taken.by_feature()
        return lp_ops.label_profile(fc.col_ptr, fc.row, fc.val, lab, 8, "sum")

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    torch.cuda.synchronize()
    ref = C.reference(*case, 8, "sum")
    C.same_tuple(out, tuple(getattr(ref, k) for k in C.FIELDS))


# ----------------------------------------------------------------------------- engines
from test_sparse_codes_gpu import (B_ENG, N_DICT, N_POOL, TK_B, TK_N, _data, _engine, _models, _state_tensors,  # noqa: E402
                                   _topk_case, _topk_models)


def _pool_labels(N, L=40, seed=9):
    lab = torch.randint(0, L, (N,), generator=torch.Generator().manual_seed(seed))
    lab[::17] = -1
    lab[0] = lab[N - 1] = -1
    return lab


def _check_engine(codes, nactive, got, labels, **kw):
    """``got`` equals the oracle run on the engine's own sparse codes, which are bf16-valued."""
    from sparse_coding__amd.engine import label_profile as lp

    host = codes.to("cpu")
    assert torch.equal(host.val, host.val.to(torch.bfloat16).float())
    want = lp.label_profile_reference(host, labels, nactive=nactive, **kw)
    C.same(got, want)
    return want


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_sae_engine_label_profile(masked):
    from sparse_coding__amd.engine.sparse_codes import SparseCodesOverflow

    sizes = [128, 256, 256] if masked else None
    sig, models = _models("untied", sizes)
    eng = _engine(sig, models)
    eng.step_batch(_data(seed=2, batches=1))
    pool = _data(seed=1)
    labels = _pool_labels(N_POOL)
    codes = eng.encode_sparse(pool)
    got = eng.label_profile(pool, labels.to(DEV), m=8, n_classes=40)
    torch.cuda.synchronize()
    assert got.top_label.is_cuda and got.top_label.shape == (G, N_DICT, 8) and got.n_rows == int((labels >= 0).sum())
    want = _check_engine(codes, sizes, got, labels, m=8, n_classes=40)
    assert int(want.top_label.max()) >= 0 and int(want.n_entries.sum()) > 0 and want.skipped.tolist() == [0] * G
    assert float(got.recall().max()) <= 1.0 and float(got.share().sum(-1).max()) <= 1.0 + 1e-12
    if masked:
        assert not got.n_entries[0, 128:].any() and bool((got.top_label[0, 128:] == -1).all())
        assert bool(got.n_entries[1, 128:].any())
    _check_engine(codes, sizes, eng.label_profile(pool, labels, m=2, rank_by="count"), labels, m=2, rank_by="count")
    budget = max(1, int(codes.nnz().min()) // N_POOL // 2)
    with pytest.raises(SparseCodesOverflow):
        eng.label_profile(pool, labels, budget=budget)
    with pytest.raises(ValueError):
        eng.label_profile(pool, labels, m=65)


def test_label_profile_leaves_training_state_alone():
    sig, models = _models("untied")
    a, b = _engine(sig, models).enable_graph(), _engine(sig, models).enable_graph()
    xs = _data(seed=3, batches=2)
    pool = _data(seed=4)
    labels = _pool_labels(N_POOL)
    for e in (a, b):
        e.step_batch(xs[:B_ENG])
    graphs = dict(a._graph)
    a.label_profile(pool, labels)
    a.label_profile(pool, labels, m=2, rank_by="count", n_classes=40)
    for e in (a, b):
        e.step_batch(xs[B_ENG:])
    torch.cuda.synchronize()
    assert set(a._graph) == set(graphs) and all(a._graph[k] is g for k, g in graphs.items())
    assert a.step_count == b.step_count == 2 and a.rows_seen == b.rows_seen
    sa, sb = _state_tensors(a), _state_tensors(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_topk_engine_label_profile():
    from sparse_coding__amd.engine.topk import FusedTopKEnsemble

    W, x = _topk_case(n_batches=1)
    eng = FusedTopKEnsemble(_topk_models(W), batch_size=TK_B, device=DEV, lr=1e-3)
    pool = x.to(DEV)
    labels = _pool_labels(pool.shape[0])
    codes = eng.encode_sparse(pool)
    got = eng.label_profile(pool, labels, m=4, n_classes=40)
    torch.cuda.synchronize()
    assert got.top_label.shape == (G, TK_N, 4)
    want = _check_engine(codes, None, got, labels, m=4, n_classes=40)
    assert int(want.n_entries[:, 0].min()) > 0 and int(want.n_labels.max()) > 1   # atom 0 fires on every non-zero row


def test_trainer_routes_label_profile():
    from sparse_coding__amd.engine import label_profile as lp
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.topk import TopKEncoder

    sig, models = _models("untied")
    pool = _data(seed=5)
    labels = _pool_labels(N_POOL)
    tr = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV)
    assert tr.kind == "fused-sae"
    got = tr.label_profile(pool.cpu(), labels, m=3, rank_by="count")
    got2 = tr.impl.label_profile(pool, labels.to(DEV), m=3, rank_by="count")
    assert isinstance(got, lp.LabelProfile) and got.top_label.is_cuda
    C.same(got, got2)
    W, x = _topk_case(n_batches=1, zero_rows=0, seed=102)
    tk = EnsembleTrainer(_topk_models(W), TopKEncoder, lr=1e-3, batch_size=TK_B, device="cuda:0")
    assert tk.kind == "fused-topk"
    lab = _pool_labels(x.shape[0])
    _check_engine(tk.encode_sparse(x), None, tk.label_profile(x, lab, m=2), lab, m=2)
    # an eager SAE: the oracle on its torch codes
    eager = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV, engine="eager")
    assert eager.kind == "eager"
    rows = pool.float()
    got = eager.label_profile(rows, labels, m=2, n_classes=40)
    C.same(got, lp.label_profile_reference(eager.encode_sparse(rows), labels, m=2, n_classes=40))


def test_data_parallel_trainer_refuses():
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.signatures import FunctionalSAE

    models = [FunctionalSAE.init(16, 32, 1e-3) for _ in range(2)]
    tr = EnsembleTrainer(models, FunctionalSAE, batch_size=16, device="cpu", engine="eager", parallel="dp")
    with pytest.raises(NotImplementedError, match="data-parallel"):
        tr.label_profile(torch.randn(64, 16), torch.zeros(64, dtype=torch.int64))
