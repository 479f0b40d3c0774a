"""Expected interference on the MI355X: the kernels of ``csrc/interference.hip`` against the fp64 torch oracle
on the inputs of ``interference_cases.py`` -- bit-exact on the planted powers of two, within the fp32 bound on
random overlapping atoms -- reproducibility and row windows, the guards of the gathering kernel, and
``interference`` of the fused SAE and top-k engines and of the trainer end to end."""

import pytest
import torch

import interference_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = C.G
CAP_SENTINEL, INT_SENTINEL = -3.0, -99


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_coding__amd.ops import _lib as L

    L.lib()  # must load: no silent fallback on a GPU box
    yield


_CASES = {}


def _case(kind, n, d):
    """(D bf16 on the device, SparseCodes on the device, SparseCodes on the CPU, D on the CPU, fp64 oracle):
    built once per (kind, shape) and shared; nothing here is modified by a test."""
    from sparse_coding__amd.engine import interference as ic
    from sparse_coding__amd.engine.sparse_codes import sparse_codes_reference

    key = (kind, n, d)
    if key not in _CASES:
        if kind == "planted":
            D, codes, _ = C.planted(n, d)
        else:
            D, codes = C.random_case(n, d)
        sc = sparse_codes_reference([codes])
        _CASES[key] = (D.to(DEV), sc.to(DEV), sc, D, ic.active_capacity_reference(sc, D))
    return _CASES[key]


def _flat(shape, dtype, fill, pad=64):
    """A sentinel-filled tensor of ``shape`` cut from a flat buffer with ``pad`` spare elements behind it."""
    numel = 1
    for s in shape:
        numel *= s
    flat = torch.full((numel + pad,), fill, device=DEV, dtype=dtype)
    return flat, flat[:numel].view(*shape)


def _run(sc, D, nactive=None, windows=None, entry=True):
    """One ``active_capacity`` call per row window into zeroed sums; returns (entry_cap, qsum, count, skipped)."""
    from sparse_coding__amd.ops import interference as ic_ops

    n = D.shape[1]
    qsum = torch.zeros(G, n, device=DEV, dtype=torch.int64)
    count = torch.zeros(G, n, device=DEV, dtype=torch.int64)
    skipped = torch.zeros(G, device=DEV, dtype=torch.int64)
    ecap = torch.zeros(G, sc.cap, device=DEV) if entry else None
    norm2 = ic_ops.row_norm2(D)
    for row0, rows in (windows or [(0, sc.n_rows)]):
        ic_ops.active_capacity(sc.row_ptr, sc.col, sc.val, D, norm2, qsum, count, skipped, row0=row0, n_rows=rows,
                               nactive=nactive, entry_cap=ecap)
    torch.cuda.synchronize()
    return ecap, qsum, count, skipped


# ----------------------------------------------------------------------------- sc_row_norm2
@pytest.mark.parametrize("n,d", C.SHAPES + [(130, 544)])
def test_row_norm2(n, d):
    from sparse_coding__amd.ops import interference as ic_ops

    gen = torch.Generator().manual_seed(n + d)
    D = torch.randn(G, n, d, generator=gen).to(torch.bfloat16)
    flat, out = _flat((G, n), torch.float32, CAP_SENTINEL)
    ic_ops.row_norm2(D.to(DEV), out)
    again = ic_ops.row_norm2(D.to(DEV))
    torch.cuda.synchronize()
    want = (D.double() ** 2).sum(-1)
    # d products exact in fp32 up to one rounding each, d - 1 additions: (d + 1) 2^-24 relative on positive terms
    assert float(((out.cpu().double() - want).abs() / want).max()) <= (d + 1) * 2.0 ** -24
    assert torch.equal(out, again) and bool((flat[G * n:] == CAP_SENTINEL).all())
    # integers: exact
    Di = torch.randint(-3, 4, (G, n, d), generator=gen).to(torch.bfloat16)
    assert torch.equal(ic_ops.row_norm2(Di.to(DEV)).cpu().double(), (Di.double() ** 2).sum(-1))


# ----------------------------------------------------------------------------- 1. planted, bit-exact
@pytest.mark.parametrize("n,d", C.SHAPES)
def test_planted_is_bit_exact(n, d):
    D, sc, _, _, ref = _case("planted", n, d)
    ecap, qsum, count, skipped = _run(sc, D)
    assert torch.equal(ecap.cpu().double(), ref.entry_cap)
    assert torch.equal(qsum.cpu(), ref.qsum) and torch.equal(count.cpu(), ref.count)
    assert torch.equal(skipped.cpu(), ref.skipped) and not skipped.any()
    assert int(count.sum()) == int(sc.nnz().sum())
    # the public entry point takes the kernel route for a bf16 dictionary on the device
    from sparse_coding__amd.eval import metrics

    res = metrics.expected_interference(sc, D)
    assert res.qsum.device.type == "cuda" and res.n_rows == C.B and res.check() is res
    assert torch.equal(res.qsum, qsum) and torch.equal(res.count, count)
    want = ref.qsum.double() * 2.0 ** -32 / ref.count.clamp(min=1).double()
    assert torch.equal(res.expected.cpu(), want)
    assert float((res.capacity.cpu() - metrics.capacity_per_feature_lowrank(D.cpu())).abs().max()) <= 1e-12


# ----------------------------------------------------------------------------- 2. random, bounded
@pytest.mark.parametrize("n,d", C.SHAPES)
def test_random_is_inside_the_fp32_bound(n, d):
    D, sc, _, _, ref = _case("random", n, d)
    ecap, qsum, count, skipped = _run(sc, D)
    bound = C.entry_bound(ref, d)
    err = (ecap.cpu().double() - ref.entry_cap).abs()
    stored = ref.entry_len > 0
    ratio = float((err[stored] / bound[stored]).max())
    print(f"random n = {n}, d = {d}: largest |cap - cap_ref| / bound = {ratio:.3g}")
    assert torch.equal(count.cpu(), ref.count) and not skipped.any()
    assert ratio <= 1.0
    assert not err[~stored].any()
    # the sums: every entry within its bound, plus the two roundings to a multiple of 2^-32
    per_feature = torch.zeros(G, n, dtype=torch.float64)
    for g in range(G):
        k = int(sc.nnz()[g])
        per_feature[g].index_add_(0, sc.col[g, :k].long().cpu(), bound[g, :k] * 2.0 ** 32 + 0.5)
    assert bool(((qsum.cpu() - ref.qsum).abs().double() <= per_feature).all())


# ----------------------------------------------------------------------------- 3. reproducible, chunk-invariant
@pytest.mark.parametrize("n,d", [(640, 160), (128, 32)])
def test_same_bits_every_run_and_under_any_row_windows(n, d):
    D, sc, _, _, _ = _case("random", n, d)
    a = _run(sc, D)
    b = _run(sc, D)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    w = _run(sc, D, windows=[(0, 37), (37, 1), (38, 0), (38, C.B - 38)])
    for x, y in zip(a, w):
        assert torch.equal(x, y)
    rev = _run(sc, D, windows=[(64, 64), (0, 64)])
    for x, y in zip(a, rev):
        assert torch.equal(x, y)
    # a window alone touches only its own rows' entries
    part = _run(sc, D, windows=[(5, 20)])
    lo, hi = sc.row_ptr[:, 5].tolist(), sc.row_ptr[:, 25].tolist()
    for g in range(G):
        assert torch.equal(part[0][g, lo[g]:hi[g]], a[0][g, lo[g]:hi[g]])
        assert not part[0][g, :lo[g]].any() and not part[0][g, hi[g]:].any()
    no_entry = _run(sc, D, entry=False)
    assert no_entry[0] is None and torch.equal(no_entry[1], a[1]) and torch.equal(no_entry[2], a[2])


# ----------------------------------------------------------------------------- 4. guards
def test_outputs_stay_inside_their_buffers():
    from sparse_coding__amd.ops import interference as ic_ops

    n, d = 640, 160
    D, sc, _, _, ref = _case("planted", n, d)
    cap = sc.cap
    nnz = sc.nnz().tolist()
    assert min(nnz) < cap  # (a model with an unused tail)
    fe, ecap = _flat((G, cap), torch.float32, CAP_SENTINEL)
    fq, qsum = _flat((G, n), torch.int64, INT_SENTINEL)
    fc, count = _flat((G, n), torch.int64, INT_SENTINEL)
    fs, skipped = _flat((G,), torch.int64, INT_SENTINEL)
    ic_ops.active_capacity(sc.row_ptr, sc.col, sc.val, D, ic_ops.row_norm2(D), qsum, count, skipped, entry_cap=ecap)
    torch.cuda.synchronize()
    for g in range(G):
        assert torch.equal(ecap[g, :nnz[g]].cpu().double(), ref.entry_cap[g, :nnz[g]])
        assert bool((ecap[g, nnz[g]:] == CAP_SENTINEL).all())  # the unused tail
    assert torch.equal(qsum.cpu() - INT_SENTINEL, ref.qsum) and torch.equal(count.cpu() - INT_SENTINEL, ref.count)
    assert bool((skipped == INT_SENTINEL).all())
    assert bool((fe[G * cap:] == CAP_SENTINEL).all()) and bool((fq[G * n:] == INT_SENTINEL).all())
    assert bool((fc[G * n:] == INT_SENTINEL).all()) and bool((fs[G:] == INT_SENTINEL).all())


def test_rows_that_were_not_stored_are_skipped_and_counted():
    from sparse_coding__amd.engine import interference as ic
    from sparse_coding__amd.engine.sparse_codes import SparseCodes

    n, d = 128, 128
    D, sc, sc_cpu, D_cpu, full = _case("planted", n, d)
    cap = int(sc_cpu.row_ptr[:, 60].min()) + 3  # every model loses its last rows, at least one from mid-row on
    short_cpu = SparseCodes(sc_cpu.n_rows, n, sc_cpu.row_ptr, sc_cpu.col[:, :cap].contiguous(),
                            sc_cpu.val[:, :cap].contiguous())
    ref = ic.active_capacity_reference(short_cpu, D_cpu)
    assert bool((ref.skipped > 0).all()) and int(ref.count.sum()) > 0
    ecap, qsum, count, skipped = _run(short_cpu.to(DEV), D)
    assert torch.equal(skipped.cpu(), ref.skipped)
    assert torch.equal(ecap.cpu().double(), ref.entry_cap)
    assert torch.equal(qsum.cpu(), ref.qsum) and torch.equal(count.cpu(), ref.count)
    for g in range(G):  # the rows that fit are the full run's
        k = int(short_cpu.row_ptr[g][short_cpu.row_ptr[g] <= cap].max())
        assert torch.equal(ref.entry_cap[g, :k], full.entry_cap[g, :k])
    res = ic.Interference(sc.n_rows, qsum, count, skipped, torch.zeros(G, n, dtype=torch.float64))
    with pytest.raises(ic.InterferenceSkipped):
        res.check()
    # negative and decreasing pointers: skipped too
    rp = sc_cpu.row_ptr.clone()
    rp[0, 3] = -1   # rows 2 and 3 of model 0
    rp[1, 0] = 1    # row 0 of model 1 (empty) runs from 1 to 0
    odd = SparseCodes(sc_cpu.n_rows, n, rp, sc_cpu.col, sc_cpu.val)
    ref = ic.active_capacity_reference(odd, D_cpu)
    assert ref.skipped.tolist() == [2, 1, 0]
    ecap, qsum, count, skipped = _run(odd.to(DEV), D)
    assert torch.equal(skipped.cpu(), ref.skipped) and torch.equal(qsum.cpu(), ref.qsum)
    assert torch.equal(count.cpu(), ref.count)


@pytest.mark.parametrize("bad", [640, 2 ** 31 - 1, -1, -(2 ** 31)])
def test_an_invalid_column_skips_its_row_only(bad):
    """A hand-corrupted copy: one column of one row outside [0, n).  The kernel checks every column of a row
    before it gathers anything, so the row is left out and nothing is read out of bounds."""
    from sparse_coding__amd.engine import interference as ic
    from sparse_coding__amd.engine.sparse_codes import SparseCodes

    n, d = 640, 32
    D, sc, sc_cpu, D_cpu, full = _case("planted", n, d)
    col = sc_cpu.col.clone()
    lo, hi = int(sc_cpu.row_ptr[1, 9]), int(sc_cpu.row_ptr[1, 10])  # the all-active row of model 1
    assert hi - lo == n
    col[1, hi - 1] = bad  # (the last entry: every other column of the row is valid)
    hurt = SparseCodes(sc_cpu.n_rows, n, sc_cpu.row_ptr, col, sc_cpu.val)
    ref = ic.active_capacity_reference(hurt, D_cpu)
    assert ref.skipped.tolist() == [0, 1, 0]
    ecap, qsum, count, skipped = _run(hurt.to(DEV), D)
    assert torch.equal(skipped.cpu(), ref.skipped)
    assert torch.equal(ecap.cpu().double(), ref.entry_cap) and not ecap[1, lo:hi].any()
    assert torch.equal(qsum.cpu(), ref.qsum) and torch.equal(count.cpu(), ref.count)
    assert torch.equal(ecap[1, :lo].cpu().double(), full.entry_cap[1, :lo])
    assert torch.equal(ecap[1, hi:].cpu().double(), full.entry_cap[1, hi:])


def test_a_masked_run_never_touches_a_dead_column():
    from sparse_coding__amd.engine import interference as ic

    n, d = 128, 128
    D, sc, sc_cpu, D_cpu, _ = _case("random", n, d)
    live = [128, 120, 0]
    ref = ic.active_capacity_reference(sc_cpu, D_cpu, nactive=live)
    assert 0 < int(ref.skipped[1]) < C.B and int(ref.skipped[2]) == C.B - 1  # (row 0 is empty: nothing to skip)
    Dm = D.clone()
    Dm[1, 120:] = float("nan")  # a gathered dead atom would poison its row
    Dm[2] = float("nan")
    ecap, qsum, count, skipped = _run(sc, Dm, nactive=torch.tensor(live, device=DEV, dtype=torch.int32))
    assert torch.equal(skipped.cpu(), ref.skipped) and torch.equal(count.cpu(), ref.count)
    assert int(count[1].sum()) > 0 and not count[1, 120:].any() and not qsum[1, 120:].any()
    assert not count[2].any() and not qsum[2].any()
    assert bool(torch.isfinite(ecap).all())
    bound = C.entry_bound(ref, d)
    assert bool(((ecap.cpu().double() - ref.entry_cap).abs() <= bound).all())


def test_launch_is_graph_capturable():
    from sparse_coding__amd.ops import interference as ic_ops

    n, d = 128, 128
    D, sc, _, _, ref = _case("planted", n, d)
    qsum = torch.zeros(G, n, device=DEV, dtype=torch.int64)
    count, skipped = torch.zeros_like(qsum), torch.zeros(G, device=DEV, dtype=torch.int64)
    norm2 = torch.empty(G, n, device=DEV)

    def run():
        ic_ops.row_norm2(D, norm2)
        ic_ops.active_capacity(sc.row_ptr, sc.col, sc.val, D, norm2, qsum, count, skipped)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for t in (qsum, count, skipped):
        t.zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(qsum.cpu(), 2 * ref.qsum) and torch.equal(count.cpu(), 2 * ref.count) and not skipped.any()


# ----------------------------------------------------------------------------- 5. engines
B_ENG, N_DICT, D_ACT = 128, 256, 256
N_POOL = 3 * B_ENG


def _models(kind, dict_size=None):
    from sparse_coding__amd.models import signatures as S

    l1s = [1e-4, 1e-3, 1e-2]
    if dict_size is not None:
        sig = S.FunctionalMaskedSAE if kind == "untied" else S.FunctionalMaskedTiedSAE
        return sig, [sig.init(D_ACT, k, N_DICT, l1, device=DEV) for k, l1 in zip(dict_size, l1s)]
    sig = S.FunctionalSAE if kind == "untied" else S.FunctionalTiedSAE
    return sig, [sig.init(D_ACT, N_DICT, l1, device=DEV) for l1 in l1s]


def _engine(sig, models, **kw):
    from sparse_coding__amd.engine.fused import FusedSAEEnsemble

    models = [({k: t.clone() for k, t in p.items()}, b) for p, b in models]
    return FusedSAEEnsemble(models, sig, lr=1e-3, batch_size=B_ENG, device=DEV, count_every=1, **kw)


def _data(seed=0, batches=3):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    feats = torch.nn.functional.normalize(torch.randn(1024, D_ACT, device=DEV, generator=gen), dim=-1)
    codes = torch.relu(torch.randn(batches * B_ENG, 1024, device=DEV, generator=gen) - 2.0)
    return (codes @ feats).to(torch.bfloat16)


def _state_tensors(eng):
    out = {f"p.{k}": t for k, t in eng.params.items()}
    out.update({f"m.{k}": t for k, t in eng.m.items()})
    out.update({f"v.{k}": t for k, t in eng.v.items()})
    out.update(enc_shadow=eng.enc_shadow, dec_shadow=eng.dec_shadow, norms=eng.norms, out=eng.out,
               step_dev=eng.step_dev, feature_counts=eng.feature_counts)
    return out


def _square_capacity(D, live=None):
    out = torch.zeros(D.shape[0], D.shape[1], dtype=torch.float64)
    for g in range(D.shape[0]):
        k = D.shape[1] if live is None else live[g]
        sq = (D[g, :k].double() @ D[g, :k].double().T) ** 2
        out[g, :k] = torch.diagonal(sq) / sq.sum(-1)
    return out


def _assert_engine_result(got, codes, shadow, live=None, n_rows=N_POOL):
    """``got`` against the fp64 oracle on the engine's own sparse codes and bf16 shadow."""
    from sparse_coding__amd.engine import interference as ic

    torch.cuda.synchronize()
    sc, Dc = codes.to("cpu"), shadow.cpu()
    ref = ic.active_capacity_reference(sc, Dc, nactive=live)
    n, d = Dc.shape[1:]
    assert got.n_rows == n_rows and got.qsum.device.type == "cuda"
    assert torch.equal(got.count.cpu(), ref.count) and torch.equal(got.skipped.cpu(), ref.skipped)
    bound = C.entry_bound(ref, d)
    per_feature = torch.zeros(G, n, dtype=torch.float64)
    for g in range(G):
        k = min(int(sc.nnz()[g]), sc.cap)
        per_feature[g].index_add_(0, sc.col[g, :k].long(), bound[g, :k] * 2.0 ** 32 + 0.5)
    assert bool(((got.qsum.cpu() - ref.qsum).abs().double() <= per_feature).all())
    assert float((got.capacity.cpu() - _square_capacity(Dc, live)).abs().max()) <= 1e-10
    want = ref.qsum.double() * 2.0 ** -32 / ref.count.clamp(min=1).double()
    assert float((got.expected.cpu() - want).abs().max()) < 1e-4 and float(got.expected.max()) <= 1.0 + 1e-6
    return ref


@pytest.mark.parametrize("kind", ["untied", "tied"])
def test_sae_engine_interference_matches_oracle(kind):
    from sparse_coding__amd.engine import interference as ic

    sig, models = _models(kind)
    eng = _engine(sig, models)
    eng.step_batch(_data(seed=2, batches=1))  # biases and moments away from their initial values
    pool = _data(seed=1)
    got = eng.interference(pool)
    codes = eng.encode_sparse(pool)
    ref = _assert_engine_result(got, codes, eng.dec_shadow)
    assert not ref.skipped.any() and got.check() is got and int(got.count.sum()) > 0
    # the same bits again, and chunk by chunk through state=
    again = eng.interference(pool)
    part = eng.interference(pool[B_ENG:], state=eng.interference(pool[:B_ENG]))
    torch.cuda.synchronize()
    for other in (again, part):
        assert other.n_rows == N_POOL
        for k in ("qsum", "count", "skipped", "capacity"):
            assert torch.equal(getattr(other, k), getattr(got, k)), k
    # a budget that is too small: the rows that lost entries are skipped and counted, the others are exact
    budget = max(1, int(codes.nnz().min()) // N_POOL // 2)
    tight = eng.interference(pool, budget=budget)
    ref = _assert_engine_result(tight, eng.encode_sparse(pool, budget=budget), eng.dec_shadow)
    assert bool((ref.skipped > 0).all())
    with pytest.raises(ic.InterferenceSkipped):
        tight.check()
    for bad in (pool[: B_ENG + 64], pool[:0], pool[:, :128]):
        with pytest.raises(ValueError):
            eng.interference(bad)
    with pytest.raises(ValueError):
        eng.interference(pool, state="no state")


@pytest.mark.parametrize("kind", ["untied", "tied"])
def test_masked_sae_engine_interference(kind):
    sizes = [128, 256, 256]
    sig, models = _models(kind, sizes)
    eng = _engine(sig, models)
    pool = _data(seed=7)
    got = eng.interference(pool)
    ref = _assert_engine_result(got, eng.encode_sparse(pool), eng.dec_shadow, live=sizes)
    assert not ref.skipped.any()
    for g, k in enumerate(sizes):
        assert not got.count[g, k:].any() and not got.qsum[g, k:].any() and not got.capacity[g, k:].any()


@pytest.mark.parametrize("kind", ["untied", "tied"])
def test_interference_leaves_training_state_alone(kind):
    """Step, ``interference`` (both budget modes), step on a graph-replaying engine against two plain steps:
    every bit of the training state equal, the captured graphs still the ones in use."""
    sig, models = _models(kind)
    a, b = _engine(sig, models).enable_graph(), _engine(sig, models).enable_graph()
    xs = _data(seed=3, batches=2)
    pool = _data(seed=4)
    for e in (a, b):
        e.step_batch(xs[:B_ENG])
    graphs = dict(a._graph)
    a.interference(pool)
    a.interference(pool, budget=4)
    for e in (a, b):
        e.step_batch(xs[B_ENG:])
    torch.cuda.synchronize()
    assert set(a._graph) == set(graphs) and all(a._graph[k] is g for k, g in graphs.items())
    assert a.step_count == b.step_count == 2 and a.rows_seen == b.rows_seen
    sa, sb = _state_tensors(a), _state_tensors(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


TK_B, TK_N, TK_D = 256, 512, 256
KS = (4, 24, 64)


def _topk_engine(seed=101, n_batches=2):
    from sparse_coding__amd.engine.topk import FusedTopKEnsemble
    from sparse_coding__amd.models.topk import TopKEncoder

    gen = torch.Generator().manual_seed(seed)
    W = torch.randn(G, TK_N, TK_D, generator=gen)
    x = torch.randn(n_batches * TK_B, TK_D, generator=gen).to(torch.bfloat16)
    models = []
    for g, k in enumerate(KS):
        p, b = TopKEncoder.init(TK_D, TK_N, k, device=DEV)
        p["dict"] = W[g].to(DEV).clone()
        models.append((p, b))
    return FusedTopKEnsemble(models, batch_size=TK_B, device=DEV, lr=1e-3), models, x.to(DEV)


def test_topk_engine_interference_matches_oracle():
    eng, _, pool = _topk_engine()
    got = eng.interference(pool)
    codes = eng.encode_sparse(pool)
    ref = _assert_engine_result(got, codes, eng.shadow, n_rows=2 * TK_B)
    assert not ref.skipped.any() and int(got.count.sum()) == int(codes.nnz().sum())
    part = eng.interference(pool[TK_B:], state=eng.interference(pool[:TK_B]))
    torch.cuda.synchronize()
    for k in ("qsum", "count", "skipped"):
        assert torch.equal(getattr(part, k), getattr(got, k)), k
    tight = eng.interference(pool, budget=8)
    ref = _assert_engine_result(tight, eng.encode_sparse(pool, budget=8), eng.shadow, n_rows=2 * TK_B)
    assert ref.skipped.tolist()[0] == 0 and ref.skipped.tolist()[2] > 0
    with pytest.raises(ValueError):
        eng.interference(pool[:100])


def test_topk_step_after_interference_is_bit_identical():
    """A captured-graph step after ``interference`` (called after an odd number of steps, both budget modes)
    matches an engine that never made the call, bitwise."""
    a, _, pool = _topk_engine(seed=103)
    b, _, _ = _topk_engine(seed=103)
    a.enable_graph()
    b.enable_graph()
    for e in (a, b):
        e.step_batch(pool[:TK_B])
    a.interference(pool)
    a.interference(pool, budget=16)
    for x in (pool[TK_B:], pool[:TK_B]):
        for e in (a, b):
            e.step_batch(x)
    torch.cuda.synchronize()
    assert a.step_count == b.step_count == 3
    for k in a.params:
        assert torch.equal(a.params[k], b.params[k]) and torch.equal(a.m[k], b.m[k]) and torch.equal(a.v[k], b.v[k])
    assert torch.equal(a.shadow, b.shadow) and torch.equal(a.norms, b.norms)


def test_trainer_routes_to_the_engines():
    from sparse_coding__amd.engine.interference import Interference
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.topk import TopKEncoder

    sig, models = _models("untied")
    tr = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV)
    assert tr.kind == "fused-sae"
    pool = _data(seed=5)
    got = tr.interference(pool.cpu(), budget=N_DICT)
    want = tr.impl.interference(pool, budget=N_DICT)
    torch.cuda.synchronize()
    assert isinstance(got, Interference) and got.qsum.device.type == "cuda" and got.n_rows == N_POOL
    for k in ("qsum", "count", "skipped", "capacity"):
        assert torch.equal(getattr(got, k), getattr(want, k)), k
    _, tk_models, x = _topk_engine(seed=102, n_batches=1)
    tr = EnsembleTrainer(tk_models, TopKEncoder, lr=1e-3, batch_size=TK_B, device="cuda:0")
    assert tr.kind == "fused-topk"
    got, want = tr.interference(x.cpu()), tr.impl.interference(x)
    torch.cuda.synchronize()
    assert torch.equal(got.qsum, want.qsum) and torch.equal(got.count, want.count) and got.n_rows == TK_B
    # the torch path on the device (analytic engine), and the refusals
    an = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV, engine="analytic")
    res = an.interference(pool[:B_ENG])
    assert res.n_rows == B_ENG and not res.skipped.any() and int(res.count.sum()) > 0
    for par in ("dp", "zero1"):
        cpu_models = [sig.init(D_ACT, N_DICT, l1) for l1 in (1e-4, 1e-3)]
        dp = EnsembleTrainer(cpu_models, sig, batch_size=B_ENG, device="cpu", engine="eager", parallel=par)
        try:
            with pytest.raises(NotImplementedError, match="data-parallel"):
                dp.interference(pool[:B_ENG].cpu())
        finally:
            dp.close()
