"""Sparse codes on the MI355X: the two kernels of ``csrc/sparse_codes.hip`` against the torch oracle, and
``encode_sparse`` of the fused SAE and top-k engines end to end (oracle parity on the engine's own codes,
budgets and overflow, masked ensembles, untouched training state, the trainer facade, consistency with
``feature_stats``).  All outputs are exact: every comparison is ``torch.equal``."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = 3
COL_SENTINEL, VAL_SENTINEL = -7, -1.0
SHAPES = [(128, 128), (128, 640), (384, 128), (384, 640), (128, 1152)]  # 1152: two full passes and a tail


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_coding__amd.ops import _lib as L

    L.lib()  # must load: no silent fallback on a GPU box
    yield


def _codes(B, n, seed):
    """bf16 codes [G, B, n] of about 5 % positive density (negatives and -0.0 sprinkled in) with crafted rows:
    0 all zero, 1 all n positive, 2 only column 0, 3 only column n - 1, 4 positives at the lane boundary
    (7 / 8) and the pass boundaries (511 / 512, 1023 / 1024 where n allows), 5 negatives and -0.0 only,
    B - 1 (the last row of the batch) never empty."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    c = torch.rand(G, B, n, device=DEV, generator=gen) * 4 + 0.01
    u = torch.rand(G, B, n, device=DEV, generator=gen)
    c = torch.where(u < 0.05, c, torch.where(u < 0.10, -c, torch.zeros_like(c)))
    c = torch.where((u >= 0.10) & (u < 0.15), torch.full_like(c, -0.0), c)
    c[:, 0] = 0
    c[:, 1] = torch.rand(G, n, device=DEV, generator=gen) + 0.5
    c[:, 2] = 0
    c[:, 2, 0] = 1.5
    c[:, 3] = 0
    c[:, 3, n - 1] = 2.5
    c[:, 4] = 0
    for j in (7, 8, 511, 512, 1023, 1024):
        if j < n:
            c[:, 4, j] = j + 1.0
    c[:, 5] = -0.0
    c[:, 5, ::3] = -1.0
    c[:, B - 1, 3] = 3.0
    return c.to(torch.bfloat16).contiguous()


def _buffers(cap, pad=64):
    """Sentinel-filled col / val [G, cap] cut from flat buffers with ``pad`` spare elements behind them: a write
    past a model's ``cap`` would land in the next model's entries or in the spare elements."""
    fc = torch.full((G * cap + pad,), COL_SENTINEL, device=DEV, dtype=torch.int32)
    fv = torch.full((G * cap + pad,), VAL_SENTINEL, device=DEV, dtype=torch.float32)
    return fc, fv, fc[: G * cap].view(G, cap), fv[: G * cap].view(G, cap)


def _row_ptr(c, base=None, row0=0, total_rows=None):
    from sparse_coding__amd.ops import sparse_codes as sc_ops

    B = c.shape[1]
    rp = torch.zeros(G, (total_rows or row0 + B) + 1, device=DEV, dtype=torch.int64)
    if base is not None:
        rp[:, row0] = base
    nnz = torch.full((G, B), -1, device=DEV, dtype=torch.int32)
    sc_ops.code_row_counts(c, nnz)
    sc_ops.extend_row_ptr(rp, nnz, row0)
    return rp, nnz


def _assert_prefix(col, val, ref, cap, fc, fv):
    """``col`` / ``val`` [G, cap] hold the oracle's first ``min(nnz, cap)`` entries and the sentinel behind them;
    the spare elements behind the buffers are untouched."""
    nnz = ref.nnz().tolist()
    for g in range(G):
        k = min(nnz[g], cap)
        assert torch.equal(col[g, :k], ref.col[g, :k]), g
        assert torch.equal(val[g, :k], ref.val[g, :k]), g
        assert bool((col[g, k:] == COL_SENTINEL).all()) and bool((val[g, k:] == VAL_SENTINEL).all()), g
    assert bool((fc[G * cap:] == COL_SENTINEL).all()) and bool((fv[G * cap:] == VAL_SENTINEL).all())


# ----------------------------------------------------------------------------- sc_code_row_counts
@pytest.mark.parametrize("B,n", SHAPES)
def test_row_counts_match_torch(B, n):
    c = _codes(B, n, seed=B + n)
    _, nnz = _row_ptr(c)
    torch.cuda.synchronize()
    want = (c > 0).sum(-1)
    assert torch.equal(nnz.long(), want)
    # the crafted rows did what they were made for
    assert not want[:, 0].any() and bool((want[:, 1] == n).all()) and bool((want[:, 2] == 1).all())
    assert bool((want[:, 3] == 1).all()) and not want[:, 5].any() and bool((want[:, B - 1] > 0).all())
    assert bool((want[:, 4] == sum(j < n for j in (7, 8, 511, 512, 1023, 1024))).all())


# ----------------------------------------------------------------------------- sc_code_compact
@pytest.mark.parametrize("B,n", SHAPES)
def test_compact_with_exact_cap_matches_oracle(B, n):
    from sparse_coding__amd.engine import sparse_codes as sc
    from sparse_coding__amd.ops import sparse_codes as sc_ops

    c = _codes(B, n, seed=B + n + 1)
    ref = sc.sparse_codes_reference([c])
    cap = ref.cap  # the largest model's count: the other models leave a tail
    rp, _ = _row_ptr(c)
    runs = []
    for _ in range(2):
        fc, fv, col, val = _buffers(cap)
        sc_ops.code_compact(c, rp, col, val, 0)
        runs.append((fc, fv, col, val))
    torch.cuda.synchronize()
    assert torch.equal(rp, ref.row_ptr)
    fc, fv, col, val = runs[0]
    _assert_prefix(col, val, ref, cap, fc, fv)  # nothing written past row_ptr[:, -1]
    assert torch.equal(runs[1][0], fc) and torch.equal(runs[1][1], fv)  # the same bits every run
    assert int(ref.nnz().min()) < cap or G == 1
    # the result type on the kernels' output reads back the dense codes
    got = sc.SparseCodes(B, n, rp, torch.where(col == COL_SENTINEL, 0, col).contiguous(),
                         torch.where(val == VAL_SENTINEL, 0.0, val).contiguous())
    for g in range(G):
        assert torch.equal(got.to_dense(g, dtype=torch.bfloat16), torch.relu(c[g]))


@pytest.mark.parametrize("B,n", [(128, 640), (384, 128)])
def test_compact_second_batch_of_a_stream(B, n):
    """``row0 > 0`` with a non-zero base pointer: two batches into one set of buffers equal the oracle on both,
    and the second batch alone writes only from its base on."""
    from sparse_coding__amd.engine import sparse_codes as sc
    from sparse_coding__amd.ops import sparse_codes as sc_ops

    c = _codes(2 * B, n, seed=B + n + 2)
    c1, c2 = c[:, :B].contiguous(), c[:, B:].contiguous()
    ref = sc.sparse_codes_reference([c1, c2])
    cap = ref.cap
    rp = torch.zeros(G, 2 * B + 1, device=DEV, dtype=torch.int64)
    nnz = torch.empty(G, B, device=DEV, dtype=torch.int32)
    fc, fv, col, val = _buffers(cap)
    for i, cb in enumerate((c1, c2)):
        sc_ops.code_row_counts(cb, nnz)
        sc_ops.extend_row_ptr(rp, nnz, i * B)
        sc_ops.code_compact(cb, rp, col, val, i * B)
    torch.cuda.synchronize()
    assert torch.equal(rp, ref.row_ptr)
    _assert_prefix(col, val, ref, cap, fc, fv)
    # the second batch alone, from a base of its own per model
    base = torch.tensor([11, 0, 5], device=DEV)
    only = sc.sparse_codes_reference([c2])
    rp2, _ = _row_ptr(c2, base=base, row0=B)
    cap2 = int((only.nnz() + base).max())
    fc, fv, col, val = _buffers(cap2)
    sc_ops.code_compact(c2, rp2, col, val, B)
    torch.cuda.synchronize()
    assert torch.equal(rp2[:, B:] - base.unsqueeze(1), only.row_ptr)
    for g in range(G):
        b, k = int(base[g]), int(only.nnz()[g])
        assert torch.equal(col[g, b:b + k], only.col[g, :k]) and torch.equal(val[g, b:b + k], only.val[g, :k])
        assert bool((col[g, :b] == COL_SENTINEL).all()) and bool((col[g, b + k:] == COL_SENTINEL).all())
        assert bool((val[g, :b] == VAL_SENTINEL).all()) and bool((val[g, b + k:] == VAL_SENTINEL).all())
    assert bool((fc[G * cap2:] == COL_SENTINEL).all()) and bool((fv[G * cap2:] == VAL_SENTINEL).all())


@pytest.mark.parametrize("where", ["mid_row", "row_boundary", "first_entry"])
@pytest.mark.parametrize("B,n", [(128, 128), (384, 640), (128, 1152)])
def test_compact_overflow_keeps_the_oracle_prefix(B, n, where):
    """A ``cap`` that ends inside a row, exactly on a row boundary, or after one entry: the kept prefix is the
    oracle's and nothing is written at or past ``cap`` (a bounds test in the kernel, not an out-of-range
    write: the buffers' neighbours keep their sentinel)."""
    from sparse_coding__amd.engine import sparse_codes as sc
    from sparse_coding__amd.ops import sparse_codes as sc_ops

    c = _codes(B, n, seed=B + n + 3)
    full = sc.sparse_codes_reference([c])
    rp, _ = _row_ptr(c)
    if where == "mid_row":
        cap = n // 2 + 3          # inside row 1 (row 0 is empty, row 1 holds n entries), off any lane boundary
    elif where == "row_boundary":
        cap = int(full.row_ptr[0, B // 2])  # model 0's rows 0 .. B/2 - 1 fit exactly
    else:
        cap = 1
    assert 0 < cap < int(full.nnz().min())
    ref = sc.sparse_codes_reference([c], cap=cap)
    fc, fv, col, val = _buffers(cap)
    sc_ops.code_compact(c, rp, col, val, 0)
    torch.cuda.synchronize()
    assert torch.equal(rp, full.row_ptr)  # the true counts
    assert torch.equal(col, ref.col) and torch.equal(val, ref.val)
    _assert_prefix(col, val, ref, cap, fc, fv)


# ----------------------------------------------------------------------------- SAE engine end to end
B_ENG, N_DICT, D = 128, 256, 256
N_POOL = 3 * B_ENG


def _models(kind, dict_size=None):
    from sparse_coding__amd.models import signatures as S

    l1s = [1e-4, 1e-3, 1e-2]
    if dict_size is not None:
        sig = S.FunctionalMaskedSAE if kind == "untied" else S.FunctionalMaskedTiedSAE
        return sig, [sig.init(D, k, N_DICT, l1, device=DEV) for k, l1 in zip(dict_size, l1s)]
    sig = S.FunctionalSAE if kind == "untied" else S.FunctionalTiedSAE
    return sig, [sig.init(D, N_DICT, l1, device=DEV) for l1 in l1s]


def _engine(sig, models, **kw):
    from sparse_coding__amd.engine.fused import FusedSAEEnsemble

    models = [({k: t.clone() for k, t in p.items()}, b) for p, b in models]
    return FusedSAEEnsemble(models, sig, lr=1e-3, batch_size=B_ENG, device=DEV, count_every=1, **kw)


def _data(seed=0, batches=3):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    feats = torch.nn.functional.normalize(torch.randn(1024, D, device=DEV, generator=gen), dim=-1)
    codes = torch.relu(torch.randn(batches * B_ENG, 1024, device=DEV, generator=gen) - 2.0)
    return (codes @ feats).to(torch.bfloat16)


def _own_codes(eng, pool):
    """The engine's own bf16 codes, batch by batch."""
    copies = []
    for i in range(0, pool.shape[0], B_ENG):
        eng.evaluate(pool[i:i + B_ENG])
        copies.append(eng.c.clone())
    return copies


def _same(a, b):
    assert a.n_rows == b.n_rows and a.n == b.n and a.cap == b.cap
    for k in ("row_ptr", "col", "val"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and torch.equal(x, y), k


def _state_tensors(eng):
    out = {f"p.{k}": t for k, t in eng.params.items()}
    out.update({f"m.{k}": t for k, t in eng.m.items()})
    out.update({f"v.{k}": t for k, t in eng.v.items()})
    out["enc_shadow"], out["norms"], out["out"], out["step_dev"] = eng.enc_shadow, eng.norms, eng.out, eng.step_dev
    out["feature_counts"] = eng.feature_counts
    if eng.dec_shadow is not eng.enc_shadow:
        out["dec_shadow"] = eng.dec_shadow
    return out


@pytest.mark.parametrize("kind", ["untied", "tied"])
def test_engine_encode_sparse_matches_oracle_on_its_own_codes(kind):
    from sparse_coding__amd.engine import sparse_codes as sc

    sig, models = _models(kind)
    eng = _engine(sig, models)
    eng.step_batch(_data(seed=2, batches=1))  # biases and moments away from their initial values
    pool = _data(seed=1)
    copies = _own_codes(eng, pool)
    ref = sc.sparse_codes_reference(copies)
    got = eng.encode_sparse(pool)  # budget=None: sized exactly
    torch.cuda.synchronize()
    assert got.n_rows == N_POOL and got.n == N_DICT and got.col.device.type == "cuda"
    _same(got, ref)
    allc = torch.cat(copies, dim=1)
    for g in range(G):
        assert torch.equal(got.to_dense(g, dtype=torch.bfloat16), allc[g])
    l0 = got.nnz().double() / N_POOL
    print(f"engine {kind}: mean L0 per model = {[round(float(v), 1) for v in l0]}, cap = {got.cap}")
    # a generous budget: the same entries in larger buffers, nothing reported
    roomy = eng.encode_sparse(pool, budget=N_DICT)
    assert roomy.cap == N_POOL * N_DICT and not bool(roomy.overflow().any())
    assert torch.equal(roomy.row_ptr, got.row_ptr)
    assert torch.equal(roomy.col[:, :got.cap], got.col) and torch.equal(roomy.val[:, :got.cap], got.val)
    assert not roomy.col[:, got.cap:].any() and not roomy.val[:, got.cap:].any()  # the tail holds (0, 0.0)
    # a tight budget: overflow is reported, the kept prefix is the oracle's, row_ptr keeps the true counts
    budget = max(1, int(got.nnz().min()) // N_POOL // 2)
    tight = eng.encode_sparse(pool, budget=budget)
    assert tight.cap == N_POOL * budget and bool(tight.overflow().all())
    _same(tight, sc.sparse_codes_reference(copies, cap=tight.cap))
    with pytest.raises(sc.SparseCodesOverflow):
        tight.check()
    for bad in (pool[: B_ENG + 64], pool[:0], pool[:, :128]):
        with pytest.raises(ValueError):
            eng.encode_sparse(bad)
    with pytest.raises(ValueError):
        eng.encode_sparse(pool, budget=-1)


def test_engine_encode_sparse_with_fixed_affine_centering():
    """Tied models with a non-identity centering: each batch goes through ``prepare`` as in ``evaluate``."""
    from sparse_coding__amd.engine import sparse_codes as sc
    from sparse_coding__amd.models.signatures import FunctionalTiedSAE

    gen = torch.Generator(device=DEV).manual_seed(11)
    models = []
    for l1 in (1e-4, 1e-3, 1e-2):
        rot = torch.linalg.qr(torch.randn(D, D, device=DEV, generator=gen)).Q.contiguous()
        models.append(FunctionalTiedSAE.init(D, N_DICT, l1, device=DEV, rotation=rot,
                                             translation=torch.randn(D, device=DEV, generator=gen) * 0.1,
                                             scaling=torch.rand(D, device=DEV, generator=gen) + 0.5))
    eng = _engine(FunctionalTiedSAE, models)
    assert eng.centering is not None
    pool = _data(seed=6)
    _same(eng.encode_sparse(pool), sc.sparse_codes_reference(_own_codes(eng, pool)))


@pytest.mark.parametrize("kind", ["untied", "tied"])
def test_masked_ensemble_never_lists_a_masked_column(kind):
    from sparse_coding__amd.engine import sparse_codes as sc

    sizes = [128, 256, 256]
    sig, models = _models(kind, sizes)
    eng = _engine(sig, models)
    pool = _data(seed=7)
    got = eng.encode_sparse(pool)
    _same(got, sc.sparse_codes_reference(_own_codes(eng, pool)))
    nnz = got.nnz().tolist()
    for g in range(G):
        assert nnz[g] > 0 and int(got.col[g, :nnz[g]].max()) < sizes[g]
    assert int(got.col[1, :nnz[1]].max()) >= 128  # (the unmasked models do use the upper half)


@pytest.mark.parametrize("kind", ["untied", "tied"])
def test_encode_sparse_leaves_training_state_alone(kind):
    """Step, ``encode_sparse`` (both modes), step on a graph-replaying engine against two plain steps: every
    bit of the training state equal, the captured graphs still the ones in use."""
    sig, models = _models(kind)
    a, b = _engine(sig, models).enable_graph(), _engine(sig, models).enable_graph()
    xs = _data(seed=3, batches=2)
    pool = _data(seed=4)
    for e in (a, b):
        e.step_batch(xs[:B_ENG])
    graphs = dict(a._graph)
    a.encode_sparse(pool)
    a.encode_sparse(pool, budget=4)
    for e in (a, b):
        e.step_batch(xs[B_ENG:])
    torch.cuda.synchronize()
    assert set(a._graph) == set(graphs) and all(a._graph[k] is g for k, g in graphs.items())
    assert a.step_count == b.step_count == 2 and a.rows_seen == b.rows_seen
    sa, sb = _state_tensors(a), _state_tensors(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_kernels_are_graph_capturable():
    """Counts, row pointers and the fill of one batch captured into a graph and replayed on new codes."""
    from sparse_coding__amd.engine import sparse_codes as sc
    from sparse_coding__amd.ops import sparse_codes as sc_ops

    B, n = 128, 640
    c = _codes(B, n, seed=21)
    ref0 = sc.sparse_codes_reference([c])
    cap = ref0.cap + 64
    rp = torch.zeros(G, B + 1, device=DEV, dtype=torch.int64)
    nnz = torch.zeros(G, B, device=DEV, dtype=torch.int32)
    col = torch.zeros(G, cap, device=DEV, dtype=torch.int32)
    val = torch.zeros(G, cap, device=DEV)

    def run():
        sc_ops.code_row_counts(c, nnz)
        sc_ops.extend_row_ptr(rp, nnz, 0)
        sc_ops.code_compact(c, rp, col, val, 0)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    c.copy_(_codes(B, n, seed=22))
    ref = sc.sparse_codes_reference([c], cap=cap)
    assert not torch.equal(ref.row_ptr, ref0.row_ptr)
    col.zero_()
    val.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(rp, ref.row_ptr)
    for g in range(G):  # (entries of the warm-up run past this run's count were zeroed above)
        k = int(ref.nnz()[g])
        assert torch.equal(col[g, :k], ref.col[g, :k]) and torch.equal(val[g, :k], ref.val[g, :k])
        assert not col[g, k:].any() and not val[g, k:].any()


def test_column_counts_equal_feature_stats():
    sig, models = _models("untied")
    eng = _engine(sig, models)
    pool = _data(seed=8)
    got = eng.encode_sparse(pool)
    st = eng.feature_stats(pool)
    nnz = got.nnz().tolist()
    for g in range(G):
        assert torch.equal(torch.bincount(got.col[g, :nnz[g]].long(), minlength=N_DICT), st.count[g])
        f = int(st.count[g].argmax())
        rows, vals = got.feature_entries(g, f)
        assert rows.numel() == int(st.count[g, f]) and float(vals.max()) == float(st.max[g, f])


def test_trainer_runs_the_sae_engine_method():
    from sparse_coding__amd.engine.sparse_codes import SparseCodes
    from sparse_coding__amd.engine.trainer import EnsembleTrainer

    sig, models = _models("untied")
    tr = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV)
    assert tr.kind == "fused-sae"
    pool = _data(seed=5)
    got = tr.encode_sparse(pool.cpu(), budget=N_DICT // 2)
    assert isinstance(got, SparseCodes) and got.col.device.type == "cuda" and got.n_rows == N_POOL
    _same(got, tr.impl.encode_sparse(pool, budget=N_DICT // 2))


# ----------------------------------------------------------------------------- top-k engine
TK_B, TK_N, TK_D = 256, 512, 256
KS = (4, 64, 256)  # kmax = 256 = n / 2: the k = 256 model is bound to pick non-positive scores (val == 0 slots)


def _topk_case(n_batches=2, zero_rows=32, seed=101):
    """Masters [G, n, d] and a bf16 pool, built on the CPU from a fixed seed: atom 0 fires on every non-zero
    row, the last ``zero_rows`` rows of batch 0 are all zero (every pick of theirs has val == 0)."""
    gen = torch.Generator().manual_seed(seed)
    unit = lambda v: v / v.norm(dim=-1, keepdim=True)
    e = unit(torch.randn(TK_D, generator=gen))
    W = torch.randn(G, TK_N, TK_D, generator=gen)
    W = unit(W - (W @ e).unsqueeze(-1) * e)
    W[:, 0] = e
    W = W * (0.5 + 1.5 * torch.rand(G, TK_N, 1, generator=gen))
    a = 4.0 + 4.0 * torch.rand(n_batches * TK_B, 1, generator=gen)
    x = (a * e + 0.3 * torch.randn(n_batches * TK_B, TK_D, generator=gen)).to(torch.bfloat16)
    x[TK_B - zero_rows:TK_B] = 0
    return W, x


def _topk_models(W):
    from sparse_coding__amd.models.topk import TopKEncoder

    out = []
    for g, k in enumerate(KS):
        p, b = TopKEncoder.init(W.shape[2], W.shape[1], k, device=DEV)
        p["dict"] = W[g].to(DEV).clone()
        out.append((p, b))
    return out


def test_topk_engine_encode_sparse_matches_oracle_on_its_picks():
    from sparse_coding__amd.engine import sparse_codes as sc
    from sparse_coding__amd.engine.topk import FusedTopKEnsemble
    from sparse_coding__amd.engine.topk_stats import dense_codes_from_picks

    W, x = _topk_case()
    eng = FusedTopKEnsemble(_topk_models(W), batch_size=TK_B, device=DEV, lr=1e-3)
    pool = x.to(DEV)
    dense, clamped = [], False
    for i in range(0, pool.shape[0], TK_B):
        idx, val = eng._forward_only(pool[i:i + TK_B], decode=False)
        dense.append(dense_codes_from_picks(idx, val, eng.k, TK_N))
        clamped |= bool((val[2] == 0).any())  # picks inside k the ReLU clamped to 0
    assert clamped
    ref = sc.sparse_codes_reference(dense)
    got = eng.encode_sparse(pool)
    torch.cuda.synchronize()
    _same(got, ref)
    rp = got.row_ptr
    assert not (rp[:, TK_B - 31:TK_B + 1] - rp[:, TK_B - 32:TK_B]).any()  # the all-zero rows are empty rows
    assert bool((got.nnz() > 0).all())
    for g in range(G):
        assert torch.equal(got.to_dense(g), torch.cat(dense, dim=1)[g])
    roomy = eng.encode_sparse(pool, budget=max(KS))
    assert torch.equal(roomy.row_ptr, got.row_ptr) and not bool(roomy.overflow().any())
    assert torch.equal(roomy.col[:, :got.cap], got.col) and torch.equal(roomy.val[:, :got.cap], got.val)
    tight = eng.encode_sparse(pool, budget=2)
    assert bool(tight.overflow().any())
    _same(tight, sc.sparse_codes_reference(dense, cap=2 * pool.shape[0]))
    with pytest.raises(ValueError):
        eng.encode_sparse(pool[:100])


def test_trainer_runs_the_topk_engine_method():
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.topk import TopKEncoder

    W, x = _topk_case(n_batches=1, zero_rows=0, seed=102)
    tr = EnsembleTrainer(_topk_models(W), TopKEncoder, lr=1e-3, batch_size=TK_B, device="cuda:0")
    assert tr.kind == "fused-topk"
    got = tr.encode_sparse(x)
    assert got.n_rows == TK_B and got.col.device.type == "cuda"
    _same(got, tr.impl.encode_sparse(x.to(DEV)))
