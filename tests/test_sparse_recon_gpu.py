"""Truncated and ablated reconstruction error on the MI355X: the kernels of ``csrc/sparse_recon.hip`` against
the fp64 torch oracle on the inputs of ``sparse_recon_cases.py`` -- bit-exact on the planted dyadic rows, within
the fp32 bound on random rows -- shared against per-model rows, row windows and reproducibility, the guards of
the gathering kernels, and ``recon_profile`` / ``fvu_top_activating`` of the fused SAE and top-k engines and of
the trainer end to end."""

import pytest
import torch

import sparse_recon_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL, INT_SENTINEL = -3.0, -99


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_coding__amd.ops import _lib as L

    L.lib()  # must load: no silent fallback on a GPU box
    yield


_CASES = {}


def _case(kind, d):
    """dict(D, sc, x, keep, words on the device; sc_cpu, D_cpu, x_cpu, keep_cpu; ref: the fp64 oracle at J = 64):
    built once per (kind, d) and shared; nothing here is modified by a test.  The oracle's curve at a smaller J
    is its first J + 1 columns."""
    from sparse_coding__amd.engine import sparse_recon as sr
    from sparse_coding__amd.engine.sparse_codes import sparse_codes_reference

    key = (kind, d)
    if key not in _CASES:
        D, codes, x, keep = C.planted(d) if kind == "planted" else C.random_case(d)
        sc = sparse_codes_reference([codes])
        _CASES[key] = dict(D=D.to(DEV), sc=sc.to(DEV), x=x.to(DEV), keep=keep.to(DEV),
                           words=sr.keep_words(keep).to(DEV), sc_cpu=sc, D_cpu=D, x_cpu=x, keep_cpu=keep,
                           ref=sr.sparse_recon_reference(sc, D, x, 64, keep))
    return _CASES[key]


def _flat(shape, dtype, fill, pad=64):
    """A sentinel-filled tensor of ``shape`` cut from a flat buffer with ``pad`` spare elements behind it."""
    numel = 1
    for s in shape:
        numel *= s
    flat = torch.full((numel + pad,), fill, device=DEV, dtype=dtype)
    return flat, flat[:numel].view(*shape)


def _run(sc, D, x, J, words=None, nactive=None, row0=0):
    """(curve, split, skipped of the curve launch, skipped of the split launch) of one launch each."""
    from sparse_coding__amd.ops import sparse_recon as sr_ops

    G = D.shape[0]
    sk1 = torch.zeros(G, device=DEV, dtype=torch.int64)
    sk2 = torch.zeros(G, device=DEV, dtype=torch.int64)
    curve = sr_ops.recon_curve(sc.row_ptr, sc.col, sc.val, D, x, J, sk1, row0=row0, nactive=nactive)
    split = sr_ops.recon_split(sc.row_ptr, sc.col, sc.val, D, x, sk2, keep=words, row0=row0, nactive=nactive)
    torch.cuda.synchronize()
    return curve, split, sk1, sk2


# ----------------------------------------------------------------------------- 1. planted, bit-exact
@pytest.mark.parametrize("d", C.DS)
def test_planted_is_bit_exact(d):
    k = _case("planted", d)
    ref = k["ref"]
    assert C.planted_is_exact(ref) and not ref.skipped.any()
    for J in C.PLANTED_J:
        curve, split, sk1, sk2 = _run(k["sc"], k["D"], k["x"], J, k["words"])
        assert torch.equal(curve.cpu(), ref.curve[..., :J + 1].float()), J
        assert torch.equal(split.cpu(), ref.split.float()), J
        assert not sk1.any() and not sk2.any()
    bare = _run(k["sc"], k["D"], k["x"], 8)[1]
    assert torch.equal(bare[..., 0].cpu(), ref.split[..., 0].float()) and not bare[..., 1:].any()
    # the public entry point takes the kernel route for bf16 inputs on the device
    from sparse_coding__amd.eval import metrics

    res = metrics.truncated_fvu(k["sc"], k["D"], k["x"], 8, k["keep"])
    assert res.sse_prefix.device.type == "cuda" and res.n_rows == C.PLANTED_ROWS and res.check() is res
    assert torch.equal(res.sse_prefix.cpu(), ref.curve[..., :9].sum(1))  # (sums of multiples of 1/16: exact)
    assert torch.equal(res.sse_keep.cpu(), ref.split[..., 1].sum(1))
    assert torch.equal(res.sse_rest.cpu(), ref.split[..., 2].sum(1))


# ----------------------------------------------------------------------------- 2. random, bounded
@pytest.mark.parametrize("d", C.DS)
def test_random_is_inside_the_fp32_bound(d):
    """Every per-row value within ``value_bound`` of the oracle.  Largest observed fraction of the bound (one
    MI355X): 0.228 at d = 64, 0.137 at 512, 0.096 at 768, 0.083 at 1024."""
    k = _case("random", d)
    ref = k["ref"]
    curve, split, sk1, sk2 = _run(k["sc"], k["D"], k["x"], 64, k["words"])
    assert not sk1.any() and not sk2.any()
    worst = 0.0
    for got, want, rm, mm, cnt in ((curve, ref.curve, ref.curve_rm, ref.curve_mm, ref.curve_cnt),
                                   (split, ref.split, ref.split_rm, ref.split_mm, ref.split_cnt)):
        bound = C.value_bound(want, rm, mm, cnt, d)
        err = (got.cpu().double() - want).abs()
        ratio = float((err / bound.clamp(min=1e-300)).max())
        worst = max(worst, ratio)
        assert bool((err <= bound).all()), ratio
    print(f"random d = {d}: largest |value - oracle| / bound = {worst:.3g}")
    assert worst <= 1.0


# ----------------------------------------------------------------------------- 3. structure
@pytest.mark.parametrize("d", [64, 768])
def test_shared_rows_windows_and_reruns_give_the_same_bits(d):
    k = _case("random", d)
    sc, D, x, words = k["sc"], k["D"], k["x"], k["words"]
    G, N = C.RANDOM_G, C.RANDOM_ROWS
    a = _run(sc, D, x, 32, words)
    b = _run(sc, D, x, 32, words)
    per = _run(sc, D, x.expand(G, N, d).contiguous(), 32, words)
    for other in (b, per):
        for s, t in zip(a, other):
            assert torch.equal(s, t)
    # a row window equals slicing (per-model rows too: the stride is the window's)
    for lo, rows in ((0, 37), (37, 1), (38, 0), (77, 179)):
        w = _run(sc, D, x[lo:lo + rows], 32, words, row0=lo)
        assert torch.equal(w[0], a[0][:, lo:lo + rows]) and torch.equal(w[1], a[1][:, lo:lo + rows])
    xg = x.expand(G, N, d)[:, 40:90].contiguous()
    w = _run(sc, D, xg, 32, words, row0=40)
    assert torch.equal(w[0], a[0][:, 40:90]) and torch.equal(w[1], a[1][:, 40:90])
    # a shorter curve is a prefix of a longer one
    assert torch.equal(_run(sc, D, x, 5, words)[0], a[0][..., :6])


# ----------------------------------------------------------------------------- 4. guards
def test_outputs_stay_inside_their_buffers():
    from sparse_coding__amd.ops import sparse_recon as sr_ops

    k = _case("planted", 64)
    sc, D, x, ref = k["sc"], k["D"], k["x"], k["ref"]
    G, N, J = C.PLANTED_G, C.PLANTED_ROWS, 8
    fc, curve = _flat((G, N, J + 1), torch.float32, SENTINEL)
    fs, split = _flat((G, N, 3), torch.float32, SENTINEL)
    fk, sk = _flat((G,), torch.int64, INT_SENTINEL)
    sr_ops.recon_curve(sc.row_ptr, sc.col, sc.val, D, x, J, sk, out=curve)
    sr_ops.recon_split(sc.row_ptr, sc.col, sc.val, D, x, sk, keep=k["words"], out=split)
    # a window writes only its own rows
    fw, win = _flat((G, 10, J + 1), torch.float32, SENTINEL)
    sr_ops.recon_curve(sc.row_ptr, sc.col, sc.val, D, x[:, 20:30].contiguous(), J, sk, row0=20, out=win)
    torch.cuda.synchronize()
    assert torch.equal(curve.cpu(), ref.curve[..., :J + 1].float()) and torch.equal(split.cpu(), ref.split.float())
    assert torch.equal(win, curve[:, 20:30])
    assert bool((sk == INT_SENTINEL).all())
    assert bool((fc[G * N * (J + 1):] == SENTINEL).all()) and bool((fs[G * N * 3:] == SENTINEL).all())
    assert bool((fw[G * 10 * (J + 1):] == SENTINEL).all()) and bool((fk[G:] == INT_SENTINEL).all())


def test_rows_that_were_not_stored_are_skipped_and_zeroed():
    from sparse_coding__amd.engine import sparse_recon as sr
    from sparse_coding__amd.engine.sparse_codes import SparseCodes

    k = _case("random", 64)
    sc, D, x, keep = k["sc_cpu"], k["D_cpu"], k["x_cpu"], k["keep_cpu"]
    N = C.RANDOM_ROWS
    cap = int(sc.row_ptr[:, 200].min()) + 3  # every model loses its last rows, at least one from mid-row on
    short = SparseCodes(N, sc.n, sc.row_ptr, sc.col[:, :cap].contiguous(), sc.val[:, :cap].contiguous())
    rp = sc.row_ptr.clone()
    rp[0, 3] = -1   # rows 2 and 3 of model 0
    rp[1, 0] = 1    # row 0 of model 1 (empty) runs from 1 to 0
    odd = SparseCodes(N, sc.n, rp, sc.col, sc.val)
    empty = SparseCodes(N, sc.n, sc.row_ptr, sc.col[:, :0].contiguous(), sc.val[:, :0].contiguous())
    for codes, want in ((short, None), (odd, [2, 1, 0]), (empty, None)):
        ref = sr.sparse_recon_reference(codes, D, x, 8, keep)
        assert bool(ref.skipped.any()) and (want is None or ref.skipped.tolist() == want)
        curve, split, sk1, sk2 = _run(codes.to(DEV), k["D"], k["x"], 8, k["words"])
        assert torch.equal(sk1.cpu(), ref.skipped) and torch.equal(sk2.cpu(), ref.skipped)
        left = (ref.curve == 0).all(-1)  # (no kept row of this fixture has |x|^2 = 0)
        assert int(left.sum()) == int(ref.skipped.sum())
        assert not curve.cpu()[left].any() and not split.cpu()[left].any()
        for got, want_v, rm, mm, cnt in ((curve, ref.curve, ref.curve_rm, ref.curve_mm, ref.curve_cnt),
                                         (split, ref.split, ref.split_rm, ref.split_mm, ref.split_cnt)):
            assert bool(((got.cpu().double() - want_v).abs() <= C.value_bound(want_v, rm, mm, cnt, 64)).all())
    # only the rows with no entry survive buffers that hold nothing
    assert int(sr.sparse_recon_reference(empty, D, x, 8).skipped[0]) == N - int(
        (sc.row_ptr[0, 1:] == 0).sum())


@pytest.mark.parametrize("bad", [512, 2 ** 31 - 1, -1, -(2 ** 31)])
def test_an_invalid_column_skips_its_row_only(bad):
    """A hand-corrupted copy: one column of one row outside [0, n).  The kernels check every column of a row
    before they gather anything, so the row is left out and nothing is read out of bounds."""
    from sparse_coding__amd.engine.sparse_codes import SparseCodes

    k = _case("random", 64)
    sc = k["sc_cpu"]
    col = sc.col.clone()
    col[1, int(sc.row_ptr[1, 78]) - 1] = bad  # the last entry of the 300-entry row: every other column is valid
    hurt = SparseCodes(sc.n_rows, sc.n, sc.row_ptr, col, sc.val).to(DEV)
    full = _run(k["sc"], k["D"], k["x"], 16, k["words"])
    curve, split, sk1, sk2 = _run(hurt, k["D"], k["x"], 16, k["words"])
    assert sk1.tolist() == [0, 1, 0] and sk2.tolist() == [0, 1, 0]
    assert not curve[1, 77].any() and not split[1, 77].any()
    rest = torch.ones(C.RANDOM_G, C.RANDOM_ROWS, dtype=torch.bool, device=DEV)
    rest[1, 77] = False
    assert torch.equal(curve[rest], full[0][rest]) and torch.equal(split[rest], full[1][rest])


def test_a_masked_run_never_touches_a_dead_column():
    from sparse_coding__amd.engine import sparse_recon as sr

    k = _case("random", 64)
    live = [512, 400, 0]
    ref = sr.sparse_recon_reference(k["sc_cpu"], k["D_cpu"], k["x_cpu"], 8, k["keep_cpu"], nactive=live)
    assert 0 < int(ref.skipped[1]) < C.RANDOM_ROWS and int(ref.skipped[2]) > 0
    Dm = k["D"].clone()
    Dm[1, 400:] = float("nan")  # a gathered dead atom would poison its row
    Dm[2] = float("nan")
    curve, split, sk1, sk2 = _run(k["sc"], Dm, k["x"], 8, k["words"],
                                  nactive=torch.tensor(live, device=DEV, dtype=torch.int32))
    assert torch.equal(sk1.cpu(), ref.skipped) and torch.equal(sk2.cpu(), ref.skipped)
    assert bool(torch.isfinite(curve).all()) and bool(torch.isfinite(split).all())
    assert bool(((curve.cpu().double() - ref.curve).abs()
                 <= C.value_bound(ref.curve, ref.curve_rm, ref.curve_mm, ref.curve_cnt, 64)).all())


def test_host_refusals_and_graph_capture():
    from sparse_coding__amd.ops import sparse_recon as sr_ops

    k = _case("planted", 64)
    sc, D, x, ref = k["sc"], k["D"], k["x"], k["ref"]
    G = C.PLANTED_G
    sk = torch.zeros(G, device=DEV, dtype=torch.int64)
    for d in (32, 96, 1088):
        with pytest.raises(ValueError, match="d % 64"):
            sr_ops.recon_curve(sc.row_ptr, sc.col, sc.val, torch.zeros(G, sc.n, d, device=DEV, dtype=torch.bfloat16),
                               torch.zeros(G, sc.n_rows, d, device=DEV, dtype=torch.bfloat16), 8, sk)
    for J in (-1, 65):
        with pytest.raises(ValueError, match="max_kept"):
            sr_ops.recon_curve(sc.row_ptr, sc.col, sc.val, D, x, J, sk)
    with pytest.raises(ValueError, match="keep must be"):
        sr_ops.recon_split(sc.row_ptr, sc.col, sc.val, D, x, sk, keep=k["words"][:, :-1].contiguous())
    with pytest.raises(ValueError, match="x must be"):
        sr_ops.recon_split(sc.row_ptr, sc.col, sc.val, D, x.cpu(), sk)
    assert not sk.any()
    # both launches inside one captured graph
    curve = torch.empty(G, sc.n_rows, 9, device=DEV)
    split = torch.empty(G, sc.n_rows, 3, device=DEV)

    def run():
        sr_ops.recon_curve(sc.row_ptr, sc.col, sc.val, D, x, 8, sk, out=curve)
        sr_ops.recon_split(sc.row_ptr, sc.col, sc.val, D, x, sk, keep=k["words"], out=split)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    curve.fill_(SENTINEL)
    split.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(curve.cpu(), ref.curve[..., :9].float()) and torch.equal(split.cpu(), ref.split.float())
    assert not sk.any()


# ----------------------------------------------------------------------------- 5. engines
B_ENG, N_DICT, D_ACT = 128, 256, 256      # (the shapes test_interference_gpu.py builds its engines at)
N_POOL = 3 * B_ENG
G = 3
J_ENG = 32


def _models(kind, dict_size=None):
    from sparse_coding__amd.models import signatures as S

    l1s = [1e-4, 1e-3, 1e-2]
    if dict_size is not None:
        sig = S.FunctionalMaskedSAE if kind == "untied" else S.FunctionalMaskedTiedSAE
        return sig, [sig.init(D_ACT, k, N_DICT, l1, device=DEV) for k, l1 in zip(dict_size, l1s)]
    sig = S.FunctionalSAE if kind == "untied" else S.FunctionalTiedSAE
    if kind == "centred":
        gen = torch.Generator(device=DEV).manual_seed(11)
        models = []
        for l1 in l1s:
            rot = torch.linalg.qr(torch.randn(D_ACT, D_ACT, device=DEV, generator=gen)).Q.contiguous()
            models.append(sig.init(D_ACT, N_DICT, l1, device=DEV, rotation=rot,
                                   translation=torch.randn(D_ACT, device=DEV, generator=gen) * 0.1,
                                   scaling=torch.rand(D_ACT, device=DEV, generator=gen) + 0.5))
        return sig, models
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


def _prepared(eng, pool):
    """The rows the engine's decoder sees, [N, d] or [G, N, d], batch by batch through ``prepare``."""
    B = eng.batch_size
    parts = [eng.prepare(pool[i:i + B]).clone() for i in range(0, pool.shape[0], B)]
    return torch.cat(parts, dim=-2)


def _assert_profile(got, codes, shadow, x, keep=None, live=None, J=J_ENG):
    """``got`` against the fp64 oracle on the engine's own sparse codes, bf16 shadow and prepared rows: every
    sum within the sum of its rows' bounds."""
    from sparse_coding__amd.engine import sparse_recon as sr

    torch.cuda.synchronize()
    sc, Dc, xc = codes.to("cpu"), shadow.cpu(), x.cpu()
    d = Dc.shape[2]
    ref = sr.sparse_recon_reference(sc, Dc, xc, J, None if keep is None else keep.cpu(), live)
    want = sr.recon_profile_reference(sc, Dc, xc, J, None if keep is None else keep.cpu(), live)
    assert got.n_rows == sc.n_rows and got.sse_prefix.device.type == "cuda" and got.max_kept == J
    assert torch.equal(got.skipped.cpu(), ref.skipped) and torch.equal(got.rows_within.cpu(), want.rows_within)
    slack = 1 + 1e-9  # (the fp64 sums over the rows)
    b = C.value_bound(ref.curve, ref.curve_rm, ref.curve_mm, ref.curve_cnt, d).sum(1)
    assert bool(((got.sse_prefix.cpu() - want.sse_prefix).abs() <= b * slack + 1e-9 * want.sse_prefix).all())
    b = C.value_bound(ref.split, ref.split_rm, ref.split_mm, ref.split_cnt, d).sum(1)
    assert bool(((got.sse_full.cpu() - want.sse_full).abs() <= b[:, 0] * slack + 1e-9 * want.sse_full).all())
    if keep is not None:
        assert bool(((got.sse_keep.cpu() - want.sse_keep).abs() <= b[:, 1] * slack + 1e-9 * want.sse_keep).all())
        assert bool(((got.sse_rest.cpu() - want.sse_rest).abs() <= b[:, 2] * slack + 1e-9 * want.sse_rest).all())
    else:
        assert got.sse_keep is None and got.sse_rest is None
    assert torch.allclose(got.s1.cpu(), want.s1, rtol=1e-12, atol=1e-9)
    assert torch.allclose(got.s2.cpu(), want.s2, rtol=1e-12, atol=0)
    return ref, want


def _equal_profiles(a, b):
    assert a.n_rows == b.n_rows
    for k in ("sse_prefix", "sse_full", "sse_keep", "sse_rest", "rows_within", "s1", "s2", "skipped"):
        s, t = getattr(a, k), getattr(b, k)
        assert (s is None and t is None) or torch.equal(s, t), k


@pytest.mark.parametrize("kind", ["untied", "tied", "centred"])
def test_sae_engine_recon_profile_matches_oracle(kind):
    from sparse_coding__amd.engine import sparse_recon as sr

    sig, models = _models(kind)
    eng = _engine(sig, models)
    assert (eng.centering is not None) == (kind == "centred")
    eng.step_batch(_data(seed=2, batches=1))  # biases and moments away from their initial values
    pool = _data(seed=1)
    before = {k: t.clone() for k, t in _state_tensors(eng).items()}
    steps, seen = eng.step_count, eng.rows_seen
    keep = torch.rand(G, N_DICT, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)) < 0.25
    got = eng.recon_profile(pool, max_kept=J_ENG, keep=keep)
    codes = eng.encode_sparse(pool)
    x = _prepared(eng, pool)
    assert x.dim() == (3 if kind == "centred" else 2)
    ref, want = _assert_profile(got, codes, eng.dec_shadow, x, keep)
    assert not ref.skipped.any() and got.check() is got
    assert bool((got.fvu_full > 0).all()) and bool(torch.isfinite(got.fvu_prefix).all())
    # the same bits again, chunk by chunk through state=, and with the packed words
    again = eng.recon_profile(pool, max_kept=J_ENG, keep=keep)
    part = eng.recon_profile(pool[B_ENG:], max_kept=J_ENG, keep=keep,
                             state=eng.recon_profile(pool[:B_ENG], max_kept=J_ENG, keep=keep))
    packed = eng.recon_profile(pool, max_kept=J_ENG, keep=sr.keep_words(keep))
    torch.cuda.synchronize()
    for other in (again, part, packed):
        _equal_profiles(other, got)
    bare = eng.recon_profile(pool, max_kept=4)
    assert bare.sse_keep is None and torch.equal(bare.sse_full, got.sse_full)
    # (a shorter curve holds the same per-row bits; the fp64 row sums of another shape may round differently)
    assert torch.allclose(bare.sse_prefix, got.sse_prefix[:, :5], rtol=1e-12, atol=0)
    # a budget that is too small: the rows that lost entries are skipped and counted
    budget = max(1, int(codes.nnz().min()) // N_POOL // 2)
    tight = eng.recon_profile(pool, max_kept=J_ENG, budget=budget)
    ref, _ = _assert_profile(tight, eng.encode_sparse(pool, budget=budget), eng.dec_shadow, x)
    assert bool((ref.skipped > 0).all())
    with pytest.raises(sr.ReconSkipped):
        tight.check()
    # parameters, moments, shadows, counts and the step counter are left alone
    torch.cuda.synchronize()
    assert eng.step_count == steps and eng.rows_seen == seen
    after = _state_tensors(eng)
    for k2 in before:
        assert torch.equal(before[k2], after[k2]), k2
    for bad in (pool[: B_ENG + 64], pool[:0], pool[:, :128]):
        with pytest.raises(ValueError):
            eng.recon_profile(bad)
    for J in (-1, 65):
        with pytest.raises(ValueError, match="max_kept"):
            eng.recon_profile(pool, max_kept=J)
    with pytest.raises(ValueError):
        eng.recon_profile(pool, state="no state")
    with pytest.raises(ValueError):
        eng.recon_profile(pool, max_kept=J_ENG, state=got)  # (a state with a keep mask, a call without)


@pytest.mark.parametrize("kind", ["untied", "tied"])
def test_masked_sae_engine_recon_profile(kind):
    sizes = [128, 256, 256]
    sig, models = _models(kind, sizes)
    eng = _engine(sig, models)
    pool = _data(seed=7)
    keep = torch.rand(G, N_DICT, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6)) < 0.5
    got = eng.recon_profile(pool, max_kept=J_ENG, keep=keep)
    ref, _ = _assert_profile(got, eng.encode_sparse(pool), eng.dec_shadow, _prepared(eng, pool), keep, live=sizes)
    assert not ref.skipped.any()
    top, rest = eng.fvu_top_activating(pool, 4)
    sums = eng.feature_stats(pool).sums[:, 0]
    from sparse_coding__amd.engine import sparse_recon as sr

    mask = sr.top_features(sums, 4, eng.nactive)
    assert mask.sum(1).tolist() == [4, 4, 4] and not mask[0, 128:].any()
    want = eng.recon_profile(pool, max_kept=0, keep=mask)
    assert torch.equal(top, want.fvu_keep) and torch.equal(rest, want.fvu_rest)


def test_unsupported_kinds_are_refused():
    from sparse_coding__amd.models.signatures import FunctionalReverseSAE

    models = [FunctionalReverseSAE.init(D_ACT, N_DICT, l1, device=DEV) for l1 in (1e-4, 1e-3, 1e-2)]
    eng = _engine(FunctionalReverseSAE, models)
    pool = _data(seed=1, batches=1)
    with pytest.raises(NotImplementedError, match="recon_profile: reverse"):
        eng.recon_profile(pool)
    with pytest.raises(NotImplementedError, match="reverse"):
        eng.fvu_top_activating(pool)


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


def test_topk_engine_recon_profile_matches_oracle():
    from sparse_coding__amd.engine import sparse_recon as sr

    eng, _, pool = _topk_engine()
    before = {k: t.clone() for k, t in eng.params.items()}
    shadow, steps = eng.shadow.clone(), eng.step_count
    keep = torch.rand(G, TK_N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8)) < 0.5
    got = eng.recon_profile(pool, max_kept=J_ENG, keep=keep)
    codes = eng.encode_sparse(pool)
    ref, _ = _assert_profile(got, codes, eng.shadow, pool, keep)
    assert not ref.skipped.any()
    # a k = 4 model is all there after four codes, a k = 64 model is not
    assert torch.equal(got.rows_within[0, 4:], torch.full((J_ENG - 3,), 2 * TK_B, device=DEV))
    assert int(got.rows_within[2, J_ENG]) < 2 * TK_B
    part = eng.recon_profile(pool[TK_B:], max_kept=J_ENG, keep=keep,
                             state=eng.recon_profile(pool[:TK_B], max_kept=J_ENG, keep=keep))
    torch.cuda.synchronize()
    _equal_profiles(part, got)
    tight = eng.recon_profile(pool, max_kept=J_ENG, budget=8)
    ref, _ = _assert_profile(tight, eng.encode_sparse(pool, budget=8), eng.shadow, pool)
    assert ref.skipped.tolist()[0] == 0 and ref.skipped.tolist()[2] > 0
    with pytest.raises(sr.ReconSkipped):
        tight.check()
    top, rest = eng.fvu_top_activating(pool, 3, stats=eng.feature_stats(pool))
    want = eng.recon_profile(pool, max_kept=0, keep=sr.top_features(eng.feature_stats(pool).sums[:, 0], 3))
    assert torch.equal(top, want.fvu_keep) and torch.equal(rest, want.fvu_rest)
    torch.cuda.synchronize()
    assert eng.step_count == steps and torch.equal(eng.shadow, shadow)
    for k in before:
        assert torch.equal(eng.params[k], before[k])
    with pytest.raises(ValueError):
        eng.recon_profile(pool[:100])


# ----------------------------------------------------------------------------- 6. agreement with evaluate()
@pytest.mark.parametrize("which", ["untied", "tied", "topk"])
def test_fvu_full_agrees_with_evaluate(which):
    """``evaluate()`` measures the same FVU from the GEMM epilogue's fp32 partials of bf16 codes.  The gap
    between it and the fp64 oracle's ``fvu_full`` involves no code under test; the kernel route must lie
    within 4x that gap of ``evaluate()`` (the margin covers the seed spread of a bf16 forward pass).
    Measured (one MI355X): gap 1.08e-7 untied, 2.46e-8 tied, 9.29e-9 top-k; the kernel route 1.08e-7, 2.27e-8,
    8.79e-9 (``evaluate()`` returns fp32: the gap is the rounding of its own result)."""
    from sparse_coding__amd.engine import sparse_recon as sr

    if which == "topk":
        eng, _, pool = _topk_engine(seed=104)
        shadow, x = eng.shadow, pool
    else:
        sig, models = _models(which)
        eng = _engine(sig, models)
        eng.step_batch(_data(seed=2, batches=1))
        pool = _data(seed=9)
        shadow, x = eng.dec_shadow, _prepared(eng, pool)
    fvu_eval = eng.evaluate(pool)[0].double().cpu()
    got = eng.recon_profile(pool, max_kept=0).fvu_full.cpu()
    codes = eng.encode_sparse(pool)
    torch.cuda.synchronize()
    oracle = sr.recon_profile_reference(codes.to("cpu"), shadow.cpu(), x.cpu(), 0).fvu_full
    gap = float((oracle - fvu_eval).abs().max())
    mine = float((got - fvu_eval).abs().max())
    print(f"{which}: |oracle fvu_full - evaluate| = {gap:.3g}, |kernel fvu_full - evaluate| = {mine:.3g}, "
          f"fvu = {fvu_eval.tolist()}")
    assert mine <= 4 * gap


# ----------------------------------------------------------------------------- 7. trainer
def test_trainer_routes_to_the_engines():
    from sparse_coding__amd.engine import sparse_recon as sr
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.eval import metrics
    from sparse_coding__amd.models.topk import TopKEncoder

    sig, models = _models("untied")
    tr = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV)
    assert tr.kind == "fused-sae"
    pool = _data(seed=5)
    got = tr.recon_profile(pool.cpu(), max_kept=8, budget=N_DICT)
    want = tr.impl.recon_profile(pool, max_kept=8, budget=N_DICT)
    torch.cuda.synchronize()
    assert isinstance(got, sr.ReconProfile) and got.sse_prefix.device.type == "cuda" and got.n_rows == N_POOL
    _equal_profiles(got, want)
    # fvu_top_activating against the oracle with the same mask
    top, rest = tr.fvu_top_activating(pool, 2)
    mask = sr.top_features(tr.impl.feature_stats(pool).sums[:, 0], 2)
    codes = tr.impl.encode_sparse(pool)
    torch.cuda.synchronize()
    prof = tr.impl.recon_profile(pool, max_kept=0, keep=mask)
    assert torch.equal(top, prof.fvu_keep) and torch.equal(rest, prof.fvu_rest)
    _assert_profile(prof, codes, tr.impl.dec_shadow, pool, mask, J=0)
    n_used, t2, r2 = metrics.ensemble_fvu_top_activating(tr, torch.cat([pool, pool[:7]]), 2)
    assert n_used == N_POOL and torch.equal(t2, top) and torch.equal(r2, rest)
    _, tk_models, x = _topk_engine(seed=102, n_batches=1)
    tr = EnsembleTrainer(tk_models, TopKEncoder, lr=1e-3, batch_size=TK_B, device="cuda:0")
    assert tr.kind == "fused-topk"
    got, want = tr.recon_profile(x.cpu(), max_kept=8), tr.impl.recon_profile(x, max_kept=8)
    torch.cuda.synchronize()
    _equal_profiles(got, want)
    top, rest = tr.fvu_top_activating(x, 2)
    assert tuple(top.shape) == (G,) and bool((rest < top).all())  # (two features of 512 explain less than the rest)
    # the torch path on the device (analytic engine)
    an = EnsembleTrainer(models, sig, batch_size=B_ENG, device=DEV, engine="analytic")
    res = an.recon_profile(pool[:B_ENG], max_kept=4)
    assert res.n_rows == B_ENG and not res.skipped.any() and bool((res.fvu_full > 0).all())
