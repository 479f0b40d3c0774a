"""Top-k ensembles on the MI355X: fire counts, statistics and dead-atom resampling from the picks.

The kernels of ``csrc/topk_stats.hip`` and ``sc_resample_dict_rows`` against the torch oracles of
``engine/topk_stats.py``, and ``FusedTopKEnsemble`` end to end (window counts, ``evaluate``,
``resample_dead``, ``feature_stats``, the trainer).  Shapes are the smallest the engine admits; ks =
(4, 64, 256) makes kmax = 256 = n / 2, so the k = 256 model is bound to pick non-positive scores
(``val == 0`` slots).  Every pool is built on the CPU from a fixed seed."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
G, B, N_DICT, D = 3, 256, 512, 256
KS = (4, 64, 256)
KMAX = max(KS)
NEVER = (5, 6, 7)  # atoms along -e: never a positive score


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_coding__amd.ops import _lib as L

    L.lib()  # must load: no silent fallback on a GPU box
    yield


# ----------------------------------------------------------------------------- constructions (CPU, seeded)
def _unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def _direction(gen, d=D):
    return _unit(torch.randn(d, generator=gen))


def _atoms(gen, e, hot, never, n=N_DICT, d=D):
    """[G, n, d] masters: random atoms orthogonal to the unit direction ``e`` (their scores on a e + noise
    are the noise's alone), atom 0 = e when ``hot`` (every row picks it), atoms ``never[g]`` = -e + tiny
    noise (negative score on every row).  Row norms are spread over [0.5, 2]."""
    W = torch.randn(G, n, d, generator=gen)
    W = _unit(W - (W @ e).unsqueeze(-1) * e)
    if hot:
        W[:, 0] = e
    for g in range(G):
        for f in never[g]:
            W[g, f] = _unit(-e + 1e-3 * torch.randn(d, generator=gen))
    return W * (0.5 + 1.5 * torch.rand(G, n, 1, generator=gen))


def _rows(gen, e, n_rows, lo, hi, d=D):
    """bf16 rows a e + 0.3 noise with a uniform in [lo, hi]."""
    a = lo + (hi - lo) * torch.rand(n_rows, 1, generator=gen)
    return (a * e + 0.3 * torch.randn(n_rows, d, generator=gen)).to(torch.bfloat16)


def _models(W):
    from sparse_coding__amd.models.topk import TopKEncoder

    out = []
    for g, k in enumerate(KS):
        p, b = TopKEncoder.init(W.shape[2], W.shape[1], k, device=DEV)
        p["dict"] = W[g].to(DEV).clone()
        out.append((p, b))
    return out


def _engine(W, **kw):
    from sparse_coding__amd.engine.topk import FusedTopKEnsemble

    return FusedTopKEnsemble(_models(W), batch_size=kw.pop("batch_size", B), device=DEV, lr=1e-3, **kw)


def _stats_case(n_batches=3, batch=B, zero_rows=32, dup=True, seed=101):
    """Masters and a pool for the counting / statistics tests: (a) atom 0 is picked with a positive value
    by every non-zero row, (b) the atoms NEVER are picked positively by no row, (c) the last ``zero_rows``
    rows of batch 0 are all zero (all scores 0: picks with val == 0); ``dup``: rows repeated within batch
    0 and across the batches (equal values in different rows)."""
    gen = torch.Generator().manual_seed(seed)
    e = _direction(gen)
    W = _atoms(gen, e, hot=True, never=[NEVER] * G)
    x = _rows(gen, e, n_batches * batch, 4.0, 8.0)
    if dup:
        x[10:20] = x[0:10]
        for i in range(1, n_batches):
            x[i * batch + 50:i * batch + 60] = x[0:10]
    if zero_rows:
        x[batch - zero_rows:batch] = 0
    return W, x


def _select(x, shadow, k, kmax):
    """The training step's scores GEMM + select on one bf16 batch: fresh (idx, val)."""
    from sparse_coding__amd.ops import gemm as gemm_ops
    from sparse_coding__amd.ops import topk as T

    scores = torch.empty(shadow.shape[0], x.shape[0], shadow.shape[1], device=DEV, dtype=torch.bfloat16)
    gemm_ops.matmul_nt(x, shadow, scores)
    return T.topk_select(scores, k, kmax, x=x, D=shadow)


def _shadow(W):
    from sparse_coding__amd.ops import adam as adam_ops

    Wd = W.to(DEV).contiguous()
    shadow = torch.empty(*W.shape, device=DEV, dtype=torch.bfloat16)
    norms = torch.ones(W.shape[0], W.shape[1], device=DEV)
    adam_ops.shadow_rows(Wd, shadow, norms, normalize=True)
    return shadow


def _k():
    return torch.tensor(KS, dtype=torch.int32, device=DEV)


# ----------------------------------------------------------------------------- 1. pick_counts
def test_pick_counts_matches_reference():
    from sparse_coding__amd.engine import topk_stats as ts
    from sparse_coding__amd.ops import topk_stats as ts_ops

    W, x = _stats_case(n_batches=2, dup=False)
    shadow, k = _shadow(W), _k()
    counts = torch.zeros(G, N_DICT, dtype=torch.int64, device=DEV)
    refs = []
    for i in range(2):
        idx, val = _select(x[i * B:(i + 1) * B].to(DEV), shadow, k, KMAX)
        ts_ops.pick_counts(idx, val, k, counts)
        refs.append(ts.pick_counts_reference(idx, val, k, N_DICT))
        torch.cuda.synchronize()
        assert torch.equal(counts, sum(refs)), i  # accumulation over two calls == the sum
        if i == 0:
            # the construction: (a) every non-zero row fires atom 0, (b) nobody fires NEVER, (c) the zero rows
            # carry val == 0 picks inside k and fire nothing
            assert bool((refs[0][:, 0] == B - 32).all())
            assert not refs[0][:, list(NEVER)].any()
            assert not (val[:, B - 32:] != 0).any() and bool((val[2] == 0).any())
            assert int(refs[0].sum()) == int((val > 0).sum())
    # the device predicate: a non-counting step leaves the counts alone, a counting one adds
    before = counts.clone()
    step = torch.tensor([5], dtype=torch.int32, device=DEV)
    ts_ops.pick_counts(idx, val, k, counts, step, 2)
    torch.cuda.synchronize()
    assert torch.equal(counts, before)
    step.fill_(6)
    ts_ops.pick_counts(idx, val, k, counts, step, 2)
    torch.cuda.synchronize()
    assert torch.equal(counts, before + refs[1])
    with pytest.raises(ValueError):
        ts_ops.pick_counts(idx, val, k, counts.int())
    with pytest.raises(ValueError):
        ts_ops.pick_counts(idx, val[:, :, :8], k, counts)


def test_pick_counts_and_stats_long_batch():
    """B = 2176 (> 2048, a multiple of 128): the slot sort takes its other long-list instantiation, and
    atom 0's list is as long as the batch."""
    from sparse_coding__amd.engine import feature_stats as fs
    from sparse_coding__amd.engine import topk_stats as ts
    from sparse_coding__amd.ops import topk as T
    from sparse_coding__amd.ops import topk_stats as ts_ops

    BL = 2176
    W, x = _stats_case(n_batches=1, batch=BL, zero_rows=0, dup=False, seed=103)
    shadow, k = _shadow(W), _k()
    idx, val = _select(x.to(DEV), shadow, k, KMAX)
    counts = torch.zeros(G, N_DICT, dtype=torch.int64, device=DEV)
    ts_ops.pick_counts(idx, val, k, counts)
    ref = ts.pick_counts_reference(idx, val, k, N_DICT)
    torch.cuda.synchronize()
    assert bool((ref[:, 0] == BL).all())  # case (a): everyone fires atom 0
    assert torch.equal(counts, ref)
    lists = T.SlotLists(G, BL, N_DICT, KS, KMAX, DEV)
    T.slot_lists(idx, k, lists)
    acc = torch.zeros(G, 5, N_DICT, dtype=torch.float64, device=DEV)
    mx = torch.zeros(G, N_DICT, device=DEV)
    tv, tr = fs.empty_topk(G, N_DICT, 5, DEV)
    ts_ops.pick_stats(lists, val, acc, mx, tv, tr, 1000)
    want = fs.feature_stats_reference([ts.dense_codes_from_picks(idx, val, k, N_DICT)], topk=5, row_offset=1000)
    torch.cuda.synchronize()
    assert torch.equal(acc[:, 0].round().long(), ref) and torch.equal(acc[:, 0].round().long(), want.count)
    assert torch.equal(mx, want.max) and torch.equal(tv, want.top_vals) and torch.equal(tr, want.top_rows)


# ----------------------------------------------------------------------------- 2. pick_stats / feature_stats
@pytest.fixture(scope="module")
def stats_pool():
    """The 3-batch pool, an engine on it, and the dense codes of the engine's own picks per batch (the
    select re-run by the test: the kernels are deterministic)."""
    from sparse_coding__amd.engine import topk_stats as ts

    W, x = _stats_case()
    eng = _engine(W)
    xd = x.to(DEV)
    codes = []
    for i in range(3):
        idx, val = _select(xd[i * B:(i + 1) * B], eng.shadow, eng.k, KMAX)
        codes.append(ts.dense_codes_from_picks(idx, val, eng.k, N_DICT))
    torch.cuda.synchronize()
    return eng, xd, codes


def _same_stats(a, b):
    assert a.n_rows == b.n_rows
    for name in ("count", "sums", "max", "top_vals", "top_rows"):
        u, v = getattr(a, name), getattr(b, name)
        assert (u is None) == (v is None), name
        if u is not None:
            assert torch.equal(u, v), name


@pytest.mark.parametrize("K", [0, 1, 5, 32])
def test_feature_stats_matches_reference(stats_pool, K):
    """count / max / top lists exact; the power sums within N 2^-52 sum |c|^p per feature.  Derivation:
    a bf16-valued code to the 4th power has at most 32 significant bits, so every term c^p is exact in
    fp64 on both sides; a sum of N non-negative exact terms in ANY order errs by at most
    (N - 1) 2^-53 sum |c|^p (each of the N - 1 additions rounds a partial sum <= the total by half an ulp);
    two orderings therefore differ by at most 2 (N - 1) 2^-53 < N 2^-52 times sum |c|^p."""
    from sparse_coding__amd.engine import feature_stats as fs

    eng, x, codes = stats_pool
    N = 3 * B
    got = eng.feature_stats(x, topk=K, row_offset=40)
    want = fs.feature_stats_reference(codes, topk=K, row_offset=40)
    torch.cuda.synchronize()
    assert got.n_rows == want.n_rows == N
    assert torch.equal(got.count, want.count)
    assert torch.equal(got.max, want.max)
    if K:
        assert torch.equal(got.top_vals, want.top_vals)
        assert torch.equal(got.top_rows, want.top_rows)
    else:
        assert got.top_vals is None and got.top_rows is None
    bound = N * 2.0 ** -52 * want.sums.abs()  # (codes are >= 0: sum |c|^p is the sum itself)
    excess = (got.sums - want.sums).abs() - bound
    print("power sums: max |diff| / bound", float(((got.sums - want.sums).abs() / bound.clamp(min=1e-300)).max()))
    assert bool((excess <= 0).all())
    # the construction: the everyone-picks atom (list length B), the never-picked atoms, the zero rows
    assert bool((want.count[:, 0] == N - 32).all())
    nv = list(NEVER)
    assert not got.count[:, nv].any() and not got.max[:, nv].any() and not got.sums[:, :, nv].any()
    if K:
        assert bool((got.top_rows[:, nv] == -1).all()) and not got.top_vals[:, nv].any()
        # equal values in different rows (the duplicated rows) are listed in ascending row order
        tv, tr = got.top_vals, got.top_rows
        tie = (tv[..., 1:] == tv[..., :-1]) & (tr[..., 1:] >= 0)
        assert bool((tr[..., 1:][tie] > tr[..., :-1][tie]).all())
        if K >= 5:
            assert int(tie.sum()) > 0


@pytest.mark.parametrize("K", [0, 5])
def test_feature_stats_chunking_and_repeats_are_bitwise(stats_pool, K):
    eng, x, _ = stats_pool
    whole = eng.feature_stats(x, topk=K, row_offset=3)
    again = eng.feature_stats(x, topk=K, row_offset=3)
    st = None
    for i in range(3):
        st = eng.feature_stats(x[i * B:(i + 1) * B], topk=K, row_offset=3 + i * B, state=st)
    torch.cuda.synchronize()
    _same_stats(whole, again)
    _same_stats(whole, st)
    with pytest.raises(ValueError):
        eng.feature_stats(x[:B + 1])
    with pytest.raises(ValueError):
        eng.feature_stats(x[:B], topk=33)
    with pytest.raises(ValueError):
        eng.feature_stats(x[:B], topk=K + 1, state=whole)


# ----------------------------------------------------------------------------- 3. sc_resample_dict_rows
def _pairs(n):
    """Explicit ragged pair lists: 5 / 0 / 3 pairs in use; every slot past cnt[g] holds poison (valid
    indices of rows that must not change)."""
    dead_idx = torch.tensor([[7, 0, 130, n - 1, 64, 200, 201, 202],
                             [10, 11, 12, 13, 14, 15, 16, 17],
                             [1, 129, n - 2, 100, 101, 102, 103, 104]], dtype=torch.int32, device=DEV)
    src_idx = torch.tensor([[3, 255, 128, 0, 77, 9, 9, 9],
                            [5, 6, 7, 8, 9, 10, 11, 12],
                            [200, 1, 127, 40, 41, 42, 43, 44]], dtype=torch.int64, device=DEV)
    cnt = torch.tensor([5, 0, 3], dtype=torch.int32, device=DEV)
    touched = torch.zeros(G, n, dtype=torch.bool, device=DEV)
    for g in range(G):
        touched[g, dead_idx[g, :int(cnt[g])].long()] = True
    return dead_idx, src_idx, cnt, touched


@pytest.mark.parametrize("d", [256, 768])
def test_resample_dict_rows_matches_reference(d):
    from sparse_coding__amd.engine import topk_stats as ts
    from sparse_coding__amd.ops import adam as adam_ops
    from sparse_coding__amd.ops import resample as rs_ops

    n = 256
    gen = torch.Generator(device=DEV).manual_seed(d)
    Dm = torch.randn(G, n, d, device=DEV, generator=gen) * 0.1
    m = torch.randn(G, n, d, device=DEV, generator=gen) * 1e-3
    v = torch.randn(G, n, d, device=DEV, generator=gen).abs() * 1e-3 + 1e-9
    shadow = torch.empty(G, n, d, device=DEV, dtype=torch.bfloat16)
    norms = torch.ones(G, n, device=DEV)
    adam_ops.shadow_rows(Dm, shadow, norms, normalize=True)
    rows = torch.randn(256, d, device=DEV, generator=gen).to(torch.bfloat16)
    dead_idx, src_idx, cnt, t = _pairs(n)
    u = ~t
    scale = torch.tensor([0.21, 3.0, 0.0173], device=DEV)
    before = [a.clone() for a in (Dm, m, v, shadow, norms)]
    rD, rm, rv = Dm.clone(), m.clone(), v.clone()
    rs_ops.resample_dict_rows(dead_idx, src_idx, cnt, rows, scale, Dm, m, v, shadow, norms)
    torch.cuda.synchronize()
    ts.resample_dict_reference(rD, rm, rv, dead_idx, src_idx, cnt, rows, scale)
    assert int(t.sum()) == 8
    torch.testing.assert_close(Dm[t], rD[t], rtol=1e-6, atol=0)  # (only the reduction order of |x| differs)
    assert not m[t].any() and not v[t].any()
    assert torch.equal(m, rm) and torch.equal(v, rv)
    # every row not in the lists (the poison slots past cnt included), in every state tensor
    for now, was in zip((Dm, m, v, shadow, norms), before):
        assert torch.equal(now[u], was[u])
    # shadows and norms of the rewritten rows: the bits of a shadow_rows(normalize=True) pass over the new masters
    want_sh, want_nr = torch.empty_like(shadow), torch.ones_like(norms)
    adam_ops.shadow_rows(Dm, want_sh, want_nr, normalize=True)
    assert torch.equal(shadow[t], want_sh[t]) and torch.equal(norms[t], want_nr[t])
    with pytest.raises(ValueError):
        rs_ops.resample_dict_rows(dead_idx, src_idx, cnt, rows.float(), scale, Dm, m, v, shadow, norms)
    with pytest.raises(ValueError):
        rs_ops.resample_dict_rows(dead_idx, src_idx, cnt, rows, scale, Dm, m, v, shadow, norms[:, :-1])


# ----------------------------------------------------------------------------- 4. resample_dead end to end
# (one atom for the k = 4 model: a reseeded atom carries the pool's common direction e, so every row
# picks it afterwards and it takes one of that model's four slots per row; with three such atoms the
# remaining slot no longer reaches every other atom over the pool and the second event finds new dead ones)
DEAD_SETS = ((100,), (0, 7), (5, 6, 7, 200, 300))


def _dead_case(seed=211, pool_batches=8):
    gen = torch.Generator().manual_seed(seed)
    e = _direction(gen)
    W = _atoms(gen, e, hot=False, never=DEAD_SETS)
    return W, _rows(gen, e, pool_batches * B, 2.0, 4.0)


def _oracle_codes(x, shadow):
    """Dense codes [G, N, n] of the torch oracle on the bf16-rounded operands, on the CPU."""
    from sparse_coding__amd.models.topk import TopKEncoder

    xf, S = x.float().cpu(), shadow.float().cpu()
    return torch.stack([TopKEncoder.encode(xf, KS[g], S[g]) for g in range(G)])


def test_resample_dead_end_to_end():
    from sparse_coding__amd.engine import topk_stats as ts

    W, pool = _dead_case()
    eng = _engine(W, sparse_k=8)
    N = pool.shape[0]
    # the torch oracle alone, on the CPU, finds exactly the chosen atoms dead
    codes = _oracle_codes(pool, eng.shadow)
    dead = ~(codes > 0).any(dim=1)
    for g in range(G):
        assert dead[g].nonzero().flatten().tolist() == sorted(DEAD_SETS[g]), g
    err_ref = (torch.bmm(codes, eng.shadow.float().cpu()) - pool.float().unsqueeze(0)).pow(2).sum(-1)
    before = {k: t.clone() for k, t in (("p", eng.params["dict"]), ("sh", eng.shadow), ("nr", eng.norms))}
    poold = pool.to(DEV)
    # the per-row errors the engine ranks the pool by (its own forward-only pass, deterministic)
    err = torch.empty(G, N, device=DEV)
    for i in range(0, N, B):
        eng._forward_only(poold[i:i + B])
        err[:, i:i + B].copy_(eng.row_se)
    torch.testing.assert_close(err.sum(1).cpu(), err_ref.sum(1), rtol=2e-2, atol=0)
    scale = ts.resample_dict_scales(before["p"], dead.to(DEV), 1.0)
    nrm = before["p"].norm(dim=-1)
    for g in range(G):
        alive = [f for f in range(N_DICT) if f not in DEAD_SETS[g]]
        torch.testing.assert_close(scale[g], nrm[g, alive].mean(), rtol=1e-5, atol=0)

    cnt = eng.resample_dead(poold)
    torch.cuda.synchronize()
    assert cnt.tolist() == [len(s) for s in DEAD_SETS]
    changed = (eng.params["dict"] != before["p"]).any(-1)
    assert torch.equal(changed.cpu(), dead)  # exactly those rows
    assert torch.equal(eng.shadow[~changed], before["sh"][~changed])
    assert torch.equal(eng.norms[~changed], before["nr"][~changed])
    assert not eng.m["dict"].any() and not eng.v["dict"].any()
    unit_pool = poold.float() / poold.float().norm(dim=-1, keepdim=True)
    for g in range(G):
        new = eng.params["dict"][g, sorted(DEAD_SETS[g])]
        src = (new @ unit_pool.T).argmax(-1)
        assert len(set(src.tolist())) == len(DEAD_SETS[g])  # distinct pool rows
        torch.testing.assert_close(new, unit_pool[src] * scale[g], rtol=1e-5, atol=1e-7)
        worst = torch.sort(err[g], descending=True, stable=True).indices[:len(DEAD_SETS[g])]
        assert src.tolist() == worst.tolist()  # pick="worst": the worst rows, paired in order
    # shadows and norms are consistent with the masters: a fresh engine built from the resampled state
    # has the same bits, and one training step on the same batch agrees bitwise
    fresh = _engine(eng.params["dict"].detach().cpu(), sparse_k=8)
    assert torch.equal(fresh.shadow, eng.shadow) and torch.equal(fresh.norms, eng.norms)
    # a second event on the same pool: the reseeded atoms now fire on their source rows
    eng2 = _engine(eng.params["dict"].detach().cpu(), sparse_k=8)
    cnt2 = eng2.resample_dead(poold)
    xb = poold[:B]
    mse = [e_.step_batch(xb).clone() for e_ in (eng, fresh)]
    torch.cuda.synchronize()
    assert bool((cnt2 < cnt).all()), (cnt2.tolist(), cnt.tolist())
    assert torch.equal(mse[0], mse[1])
    for a, b in ((eng.params["dict"], fresh.params["dict"]), (eng.m["dict"], fresh.m["dict"]),
                 (eng.v["dict"], fresh.v["dict"]), (eng.shadow, fresh.shadow), (eng.norms, fresh.norms)):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        eng.resample_dead(poold[:B + 3])
    with pytest.raises(ValueError):
        eng.resample_dead(poold[:B], pick="best")
    with pytest.raises(ValueError):
        eng.resample_dead(poold[:B, :128])


def test_resample_dead_loss_sq_pick():
    W, pool = _dead_case()
    eng = _engine(W)
    gen = torch.Generator(device=DEV).manual_seed(1)
    cnt = eng.resample_dead(pool.to(DEV), pick="loss_sq", generator=gen, rule="anthropic")  # (rule: ignored)
    torch.cuda.synchronize()
    assert cnt.tolist() == [len(s) for s in DEAD_SETS]


# ----------------------------------------------------------------------------- 5. window counts
def _train_case(seed=307, steps=4):
    gen = torch.Generator().manual_seed(seed)
    W = torch.randn(G, N_DICT, D, generator=gen)
    xs = [torch.randn(B, D, generator=gen).to(torch.bfloat16).to(DEV) for _ in range(steps)]
    return W, xs


def _state(e):
    return [e.params["dict"], e.m["dict"], e.v["dict"], e.shadow, e.norms, e.mse]


@pytest.mark.parametrize("graph", [False, True])
def test_window_counts_do_not_perturb_the_step(graph):
    from sparse_coding__amd.engine import topk_stats as ts

    W, xs = _train_case()
    on, off = _engine(W, sparse_k=8, count_every=1), _engine(W, sparse_k=8)
    assert on.sparse_g == 1 and off.feature_counts is None and off.rows_seen == 0
    if graph:
        on.enable_graph()
        off.enable_graph()
    want = torch.zeros(G, N_DICT, dtype=torch.int64, device=DEV)
    for x in xs:
        on.step_batch(x)
        off.step_batch(x)
        want += ts.pick_counts_reference(on.idx, on.val, on.k, N_DICT)
    torch.cuda.synchronize()
    for a, b in zip(_state(on), _state(off)):
        assert torch.equal(a, b)
    assert torch.equal(on.feature_counts, want) and int(want.sum()) > 0
    assert on.rows_seen == 4 * B
    torch.testing.assert_close(on.feature_frequency(), want / (4 * B))
    with pytest.raises(RuntimeError):
        off.feature_frequency()


def test_count_every_two_counts_steps_0_and_2():
    """``run_source(steps=4)`` (one graph, batches fetched inside it) and graphed ``step_batch``: with
    ``count_every=2`` only steps 0 and 2 count, on the device and in ``rows_seen``."""
    from sparse_coding__amd.data.ring import DeviceRing
    from sparse_coding__amd.engine import topk_stats as ts

    W, xs = _train_case(seed=311)
    ring = DeviceRing(4 * B, D, device=DEV, seed=7)
    ring.push(torch.cat(xs))
    src = ring.graph_source(B)
    eng = _engine(W, count_every=2)
    eng.run_source(src, 4)
    torch.cuda.synchronize()
    batches = [ring.buf.index_select(0, src.perm[t * B:(t + 1) * B]) for t in range(4)]
    ref = _engine(W, count_every=2).enable_graph()
    want = torch.zeros(G, N_DICT, dtype=torch.int64, device=DEV)
    for t, x in enumerate(batches):
        ref.step_batch(x)
        if t % 2 == 0:
            want += ts.pick_counts_reference(ref.idx, ref.val, ref.k, N_DICT)
    torch.cuda.synchronize()
    assert torch.equal(eng.params["dict"], ref.params["dict"])
    assert torch.equal(eng.feature_counts, want) and torch.equal(ref.feature_counts, want)
    assert eng.rows_seen == ref.rows_seen == 2 * B and eng.step_count == 4


def test_window_counts_gate_resampling_and_checkpoints():
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.topk import TopKEncoder

    W, pool = _dead_case()
    poold = pool.to(DEV)
    eng = _engine(W, count_every=1)
    # a window in which one of the dead-on-the-pool atoms of model 2 has fired
    eng.feature_counts[2, 200] = 3
    eng.rows_seen = B
    sd = copy.deepcopy(eng.state_dict())
    assert torch.equal(sd["feature_counts"], eng.feature_counts) and sd["rows_seen"] == B
    row = eng.params["dict"][2, 200].clone()
    cnt = eng.resample_dead(poold)
    torch.cuda.synchronize()
    assert cnt.tolist() == [1, 2, 4]
    assert torch.equal(eng.params["dict"][2, 200], row)  # dead on the pool, alive in the window: kept
    assert not eng.feature_counts.any() and eng.rows_seen == 0  # reset after the event
    # without the window it goes too
    eng_b = _engine(W, count_every=1)
    eng_b.feature_counts[2, 200] = 3
    eng_b.rows_seen = B
    assert eng_b.resample_dead(poold, use_window_counts=False).tolist() == [1, 2, 5]
    # the counts round-trip through a checkpoint; one without them loads
    other = _engine(torch.randn(G, N_DICT, D), count_every=1)
    other.load_state_dict(sd)
    assert torch.equal(other.feature_counts, sd["feature_counts"]) and other.rows_seen == B
    assert torch.equal(other.params["dict"], sd["params"]["dict"])
    old = {k: v for k, v in sd.items() if k not in ("feature_counts", "rows_seen")}
    other.load_state_dict(old)
    assert not other.feature_counts.any() and other.rows_seen == 0
    tr = EnsembleTrainer(_models(W), TopKEncoder, lr=1e-3, batch_size=B, device="cuda:0")
    st = tr.state_dict()
    assert "feature_counts" not in st["impl"]
    tr.load_state_dict(st)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 6. evaluate
def test_evaluate_matches_torch():
    from sparse_coding__amd.engine import topk_stats as ts

    W, xs = _train_case(seed=401, steps=2)
    eng = _engine(W)
    x = torch.cat(xs + [xs[0][:17]])  # (trimmed to a multiple of the batch size)
    fvu, l0 = eng.evaluate(x)
    N = 2 * B
    se = torch.zeros(G, device=DEV)
    nz = torch.zeros(G, device=DEV, dtype=torch.float64)
    S = eng.shadow.float()
    for i in range(2):
        idx, val = _select(xs[i], eng.shadow, eng.k, KMAX)
        c = ts.dense_codes_from_picks(idx, val, eng.k, N_DICT)
        se += (torch.bmm(c, S) - xs[i].float().unsqueeze(0)).pow(2).sum((1, 2))
        nz += (c > 0).sum((1, 2))
    xf = x[:N].float()
    var = (xf - xf.mean(0)).pow(2).sum()
    torch.cuda.synchronize()
    assert torch.equal(l0, (nz / N).float())
    assert bool((l0 <= torch.tensor(KS, device=DEV)).all())
    torch.testing.assert_close(fvu, se / var, rtol=2e-2, atol=0)
    with pytest.raises(ValueError):
        eng.evaluate(x[:B - 1])


def test_forward_only_calls_leave_training_alone():
    """After evaluate, feature_stats and resample_dead (a pool with no dead atoms) a captured-graph step
    matches an engine that made none of these calls, bitwise: the forward-only path leaves the pick
    buffers, the dense code / code-gradient buffers and the parity alone."""
    W, xs = _train_case(seed=409, steps=4)
    gen = torch.Generator().manual_seed(5)
    pool = torch.randn(8 * B, D, generator=gen).to(torch.bfloat16).to(DEV)
    a, b = _engine(W, sparse_k=8).enable_graph(), _engine(W, sparse_k=8).enable_graph()
    for x in xs[:2]:
        a.step_batch(x)
        b.step_batch(x)
    a.step_batch(xs[2])  # an odd number of steps: the parity is 1 when the calls come
    b.step_batch(xs[2])
    a.evaluate(pool[:2 * B])
    a.feature_stats(pool[:2 * B], topk=4)
    cnt = a.resample_dead(pool)
    torch.cuda.synchronize()
    assert cnt.tolist() == [0, 0, 0]
    assert a._cur == b._cur and int(a.step_dev) == int(b.step_dev) == 3
    for x in (xs[3], xs[0]):
        a.step_batch(x)
        b.step_batch(x)
    torch.cuda.synchronize()
    for u, v in zip(_state(a) + [a.codebuf, a.dscbuf, a.idx_buf, a.g],
                    _state(b) + [b.codebuf, b.dscbuf, b.idx_buf, b.g]):
        assert torch.equal(u, v)


# ----------------------------------------------------------------------------- 7. trainer
def test_trainer_routes_topk():
    from sparse_coding__amd.engine.feature_stats import FeatureStats
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.topk import TopKEncoder

    W, pool = _dead_case()
    tr = EnsembleTrainer(_models(W), TopKEncoder, lr=1e-3, batch_size=B, device="cuda:0")
    assert tr.kind == "fused-topk"
    st = tr.feature_stats(pool[:2 * B], topk=3)
    assert isinstance(st, FeatureStats) and st.n_rows == 2 * B and st.topk == 3
    for g in range(G):
        times_active = st.per_model(g)[0]
        assert torch.equal(times_active, st.count[g].float())
        assert torch.equal(st.frequency[g], (st.count[g].double() / st.n_rows).float())
    counts = tr.resample_dead(pool, rule="reference", pick="worst")  # (the keywords the sweep driver passes)
    assert counts == [len(s) for s in DEAD_SETS] and all(isinstance(c, int) for c in counts)
    tr.step(pool[:B].to(DEV))
    torch.cuda.synchronize()
