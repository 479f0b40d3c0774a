"""Dead-feature resampling on the MI355X: the two kernels of ``csrc/resample.hip`` against torch, and
``FusedSAEEnsemble.resample_dead`` end to end (counts, masking, graphs, oracle parity, checkpoints)."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
G, B, N_DICT = 3, 128, 256
N_POOL = 2 * B


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_coding__amd.ops import _lib as L

    L.lib()  # must load: no silent fallback on a GPU box
    yield


# ----------------------------------------------------------------------------- sc_row_sqerr
@pytest.mark.parametrize("d", [256, 768])
def test_row_sqerr_matches_torch(d):
    from sparse_coding__amd.ops import resample as rs_ops

    torch.manual_seed(d)
    r = (torch.randn(G, B, d, device=DEV) * 0.3).to(torch.bfloat16)
    N, off = 2 * B + 64, B + 32  # a row stride larger than B, a slice that starts past 0
    err = torch.full((G, N), -1.0, device=DEV)
    rs_ops.row_sqerr(r, err, off)
    torch.cuda.synchronize()
    ref = r.float().pow(2).sum(-1)
    print("row_sqerr max rel err", float(((err[:, off:off + B] - ref).abs() / ref).max()))
    torch.testing.assert_close(err[:, off:off + B], ref, rtol=1e-5, atol=0)
    assert bool((err[:, :off] == -1).all()) and bool((err[:, off + B:] == -1).all())
    with pytest.raises(ValueError):
        rs_ops.row_sqerr(r, err, N - B + 1)


# ----------------------------------------------------------------------------- sc_resample_rows
def _engine_state(kind, d, seed):
    """Random engine-shaped state with consistent shadows / norms (as refresh_shadows builds them)."""
    from sparse_coding__amd.ops import adam as adam_ops

    gen = torch.Generator(device=DEV).manual_seed(seed)
    n = N_DICT

    def rnd(*shape, scale=1.0):
        return torch.randn(*shape, device=DEV, generator=gen) * scale

    keys = ["encoder", "decoder"] if kind == "untied" else ["encoder"]
    params = {k: rnd(G, n, d, scale=0.1) for k in keys}
    params["encoder_bias"] = rnd(G, n)
    m = {k: rnd(*t.shape, scale=1e-3) for k, t in params.items()}
    v = {k: rnd(*t.shape, scale=1e-3).abs() + 1e-9 for k, t in params.items()}
    enc_shadow = torch.empty(G, n, d, device=DEV, dtype=torch.bfloat16)
    norms = torch.ones(G, n, device=DEV)
    if kind == "untied":
        dec_shadow = torch.empty_like(enc_shadow)
        adam_ops.shadow_rows(params["encoder"], enc_shadow, normalize=False)
        adam_ops.shadow_rows(params["decoder"], dec_shadow, norms, normalize=True)
    else:
        dec_shadow = None
        adam_ops.shadow_rows(params["encoder"], enc_shadow, norms, normalize=True)
    return params, m, v, enc_shadow, dec_shadow, norms


def _pairs():
    """Explicit ragged pair lists: 5 / 0 / 3 pairs in use; every slot past cnt[g] holds poison (valid
    indices of rows that must not change)."""
    P = 8
    dead_idx = torch.tensor([[7, 0, 130, 255, 64, 200, 201, 202],
                             [10, 11, 12, 13, 14, 15, 16, 17],
                             [1, 129, 254, 100, 101, 102, 103, 104]], dtype=torch.int32, device=DEV)
    src_idx = torch.tensor([[3, 255, 128, 0, 77, 9, 9, 9],
                            [5, 6, 7, 8, 9, 10, 11, 12],
                            [200, 1, 127, 40, 41, 42, 43, 44]], dtype=torch.int64, device=DEV)
    cnt = torch.tensor([5, 0, 3], dtype=torch.int32, device=DEV)
    touched = torch.zeros(G, N_DICT, dtype=torch.bool, device=DEV)
    for g in range(G):
        touched[g, dead_idx[g, :int(cnt[g])].long()] = True
    assert P == dead_idx.shape[1]
    return dead_idx, src_idx, cnt, touched


@pytest.mark.parametrize("d", [256, 768])
@pytest.mark.parametrize("rule", ["reference", "anthropic"])
@pytest.mark.parametrize("kind", ["untied", "tied"])
def test_resample_rows_matches_reference(kind, rule, d):
    from sparse_coding__amd.engine import resample as rs
    from sparse_coding__amd.ops import adam as adam_ops
    from sparse_coding__amd.ops import resample as rs_ops

    params, m, v, enc_shadow, dec_shadow, norms = _engine_state(kind, d, seed=d + len(rule))
    gen = torch.Generator(device=DEV).manual_seed(5)
    rows = torch.randn(N_POOL, d, device=DEV, generator=gen).to(torch.bfloat16)
    dead_idx, src_idx, cnt, touched = _pairs()
    scale = torch.tensor([0.21, 3.0, 0.0173], device=DEV)
    flags = rs.RULES[rule]
    before = {"p": copy.deepcopy(params), "m": copy.deepcopy(m), "v": copy.deepcopy(v),
              "enc_shadow": enc_shadow.clone(), "dec_shadow": None if dec_shadow is None else dec_shadow.clone(),
              "norms": norms.clone()}
    rp, rm, rv = copy.deepcopy(params), copy.deepcopy(m), copy.deepcopy(v)
    untied = kind == "untied"
    rs_ops.resample_rows(dead_idx, src_idx, cnt, rows, scale, params["encoder"], m["encoder"], v["encoder"],
                         enc_shadow, params["encoder_bias"], m["encoder_bias"], v["encoder_bias"], norms,
                         dec=params.get("decoder"), dec_m=m.get("decoder"), dec_v=v.get("decoder"),
                         dec_shadow=dec_shadow, **flags)
    torch.cuda.synchronize()
    rs.resample_rows_reference(rp, rm, rv, dead_idx, src_idx, cnt, rows, scale, kind=kind, **flags)
    t, u = touched, ~touched
    assert int(t.sum()) == 8
    # ---- the rewritten rows against the oracle
    if flags["normalize_src"]:  # (only the reduction order of |v| differs)
        torch.testing.assert_close(params["encoder"][t], rp["encoder"][t], rtol=1e-6, atol=0)
    else:  # one fp32 multiply
        assert torch.equal(params["encoder"][t], rp["encoder"][t])
    if untied:
        if flags["set_decoder"]:
            torch.testing.assert_close(params["decoder"][t], rp["decoder"][t], rtol=1e-6, atol=0)
        else:
            assert torch.equal(params["decoder"], before["p"]["decoder"])
    assert torch.equal(params["encoder_bias"], rp["encoder_bias"])
    if flags["zero_bias"]:
        assert not params["encoder_bias"][t].any()
    for k in params:
        assert not m[k][t].any() and not v[k][t].any(), k
        assert torch.equal(m[k], rm[k]) and torch.equal(v[k], rv[k]), k
    # ---- every row not in the lists (poison slots past cnt included), in every state tensor
    for k in params:
        assert torch.equal(params[k][u], before["p"][k][u]), k
        assert torch.equal(m[k][u], before["m"][k][u]) and torch.equal(v[k][u], before["v"][k][u]), k
    assert torch.equal(enc_shadow[u], before["enc_shadow"][u])
    assert torch.equal(norms[u], before["norms"][u])
    if untied:
        assert torch.equal(dec_shadow[u], before["dec_shadow"][u])
    # ---- shadows and norms of the rewritten rows: the bits of a sc_shadow_rows pass over the new masters
    want_norms = torch.ones(G, N_DICT, device=DEV)
    want_enc = torch.empty_like(enc_shadow)
    if untied:
        want_dec = torch.empty_like(dec_shadow)
        adam_ops.shadow_rows(params["encoder"], want_enc, normalize=False)
        adam_ops.shadow_rows(params["decoder"], want_dec, want_norms, normalize=True)
        if flags["set_decoder"]:
            assert torch.equal(dec_shadow[t], want_dec[t])
            assert torch.equal(norms[t], want_norms[t])
        else:  # decoder rows did not change: neither did their shadow and norms
            assert torch.equal(dec_shadow, before["dec_shadow"]) and torch.equal(norms, before["norms"])
    else:
        adam_ops.shadow_rows(params["encoder"], want_enc, want_norms, normalize=True)
        assert torch.equal(norms[t], want_norms[t])
    assert torch.equal(enc_shadow[t], want_enc[t])


# ----------------------------------------------------------------------------- engine end to end
def _models(kind, d, dict_size=None):
    from sparse_coding__amd.models import signatures as S

    l1s = [1e-4, 1e-3, 1e-2]
    if dict_size is not None:
        sig = S.FunctionalMaskedSAE if kind == "untied" else S.FunctionalMaskedTiedSAE
        return sig, [sig.init(d, k, N_DICT, l1, device=DEV) for k, l1 in zip(dict_size, l1s)]
    sig = S.FunctionalSAE if kind == "untied" else S.FunctionalTiedSAE
    return sig, [sig.init(d, N_DICT, l1, device=DEV) for l1 in l1s]


def _engine(sig, models, **kw):
    from sparse_coding__amd.engine.fused import FusedSAEEnsemble

    models = [({k: t.clone() for k, t in p.items()}, b) for p, b in models]
    return FusedSAEEnsemble(models, sig, lr=1e-3, batch_size=B, device=DEV, count_every=1, **kw)


KILL = [[5, 17, 64, 127], [], [0, 3, 128, 200, 201, 254, 255]]  # per model; all below dict_size[0] = 128 for model 0


def _kill(eng, lists=KILL):
    for g, idx in enumerate(lists):
        eng.params["encoder_bias"][g, idx] = -1e4
    eng._bsq_dirty = True


def _data(d, seed=0, batches=2):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    feats = torch.nn.functional.normalize(torch.randn(1024, d, device=DEV, generator=gen), dim=-1)
    codes = torch.relu(torch.randn(batches * B, 1024, device=DEV, generator=gen) - 2.0)
    return (codes @ feats).to(torch.bfloat16)


def _state_tensors(eng):
    out = {f"p.{k}": t for k, t in eng.params.items()}
    out.update({f"m.{k}": t for k, t in eng.m.items()})
    out.update({f"v.{k}": t for k, t in eng.v.items()})
    out["enc_shadow"], out["norms"] = eng.enc_shadow, eng.norms
    if eng.dec_shadow is not eng.enc_shadow:
        out["dec_shadow"] = eng.dec_shadow
    return out


@pytest.mark.parametrize("d", [256, 768])
@pytest.mark.parametrize("kind,masked", [("untied", False), ("tied", False), ("untied", True), ("tied", True)])
def test_engine_resample_dead_end_to_end(kind, masked, d):
    dict_size = [128, 256, 256] if masked else None
    sig, models = _models(kind, d, dict_size)
    eng = _engine(sig, models)
    pool = _data(d, seed=1)
    _kill(eng)
    eng.step_batch(_data(d, seed=2, batches=1))  # a counted step: the window counts are in play
    assert eng.rows_seen == B
    before = {k: t.clone() for k, t in _state_tensors(eng).items()}
    cnt = eng.resample_dead(pool, rule="anthropic")
    assert cnt.device.type == "cuda" and cnt.tolist() == [len(x) for x in KILL]
    assert eng.rows_seen == 0 and not eng.feature_counts.any()
    after = _state_tensors(eng)
    touched = torch.zeros(G, N_DICT, dtype=torch.bool, device=DEV)
    for g, idx in enumerate(KILL):
        touched[g, idx] = True
    for k, t in after.items():  # only the forced rows changed
        assert torch.equal(t[~touched], before[k][~touched]), k
    assert not eng.params["encoder_bias"][touched].any()
    if masked:  # rows past a model's size are never listed: untouched, their moments still all-zero
        for k in ("encoder", "decoder"):
            if k in eng.m:
                assert not eng.m[k][0, 128:].any() and not eng.v[k][0, 128:].any()
    # each resampled feature fires on its source row in the next forward pass (the source row is the
    # pool row its new encoder row points along)
    enc = torch.nn.functional.normalize(eng.params["encoder"].float(), dim=-1)
    poolf = torch.nn.functional.normalize(pool.float(), dim=-1)
    codes = []
    for i in range(0, N_POOL, B):
        eng.evaluate(pool[i:i + B])
        codes.append(eng.c.clone())
    codes = torch.cat(codes, dim=1)  # [G, N, n]
    for g, idx in enumerate(KILL):
        for f in idx:
            cos, s = (poolf @ enc[g, f]).max(0)
            assert float(cos) > 0.999, (g, f, float(cos))
            assert float(codes[g, s, f]) > 0, (g, f)
    with pytest.raises(ValueError):
        eng.resample_dead(pool[: B + 64])


def test_engine_resample_window_counts_and_reference_rule():
    """A feature that fired in the counted window is not dead under ``use_window_counts`` even if it
    is silent on the pool; the reference rule rewrites encoder rows only."""
    d = 256
    sig, models = _models("untied", d)
    eng = _engine(sig, models)
    pool = _data(d, seed=1)
    eng.step_batch(_data(d, seed=2, batches=1))  # every feature fires somewhere in this window ...
    assert bool((eng.feature_counts > 0).all())
    _kill(eng)                                   # ... and the killed ones are silent on the pool
    dec0, bias0 = eng.params["decoder"].clone(), eng.params["encoder_bias"].clone()
    assert eng.resample_dead(pool).tolist() == [0, 0, 0]
    assert eng.rows_seen == 0
    cnt = eng.resample_dead(pool, use_window_counts=False)  # (rows_seen == 0 now: the pool decides anyway)
    assert cnt.tolist() == [len(x) for x in KILL]
    assert torch.equal(eng.params["decoder"], dec0) and torch.equal(eng.params["encoder_bias"], bias0)
    for g, idx in enumerate(KILL):
        assert not eng.m["decoder"][g, idx].any() and not eng.m["encoder_bias"][g, idx].any()


@pytest.mark.parametrize("kind", ["untied", "tied"])
def test_resample_is_graph_safe(kind):
    """An eager engine and a graph-replaying one: 3 steps, resample on the same pool, 3 steps --
    bit-identical state, with the graphs captured before the event still in use."""
    d = 256
    sig, models = _models(kind, d)
    eager, graph = _engine(sig, models), _engine(sig, models).enable_graph()
    xs = _data(d, seed=3, batches=6)
    pool = _data(d, seed=4)
    for e in (eager, graph):
        _kill(e)
    graphs = None
    for i in range(6):
        if i == 3:
            graphs = dict(graph._graph)
            ce = eager.resample_dead(pool, rule="anthropic", use_window_counts=False)
            cg = graph.resample_dead(pool, rule="anthropic", use_window_counts=False)
            assert ce.tolist() == cg.tolist() == [len(x) for x in KILL]
        for e in (eager, graph):
            e.step_batch(xs[i * B:(i + 1) * B])
    torch.cuda.synchronize()
    assert graph._graph is not None and set(graph._graph) == set(graphs)
    assert all(graph._graph[k] is g for k, g in graphs.items())  # no recapture
    a, b = _state_tensors(eager), _state_tensors(graph)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(eager.out, graph.out)


@pytest.mark.parametrize("kind", ["untied", "tied"])
def test_step_after_resample_matches_functional_oracle(kind, monkeypatch):
    """One fused step after ``resample_dead`` against a ``FunctionalEnsemble`` step after
    ``resample_rows_reference`` with the same pair lists (tolerances of
    ``test_fused_step_matches_functional_ensemble``)."""
    from sparse_coding__amd.engine import resample as rs
    from sparse_coding__amd.engine.ensemble import FunctionalEnsemble
    from sparse_coding__amd.engine.optim import adam

    d = 256
    sig, models = _models(kind, d)
    ref = FunctionalEnsemble([({k: v.clone() for k, v in p.items()}, b) for p, b in models], sig, adam,
                             {"lr": 1e-3}, device=DEV)
    fused = _engine(sig, models)
    _kill(fused)
    for g, idx in enumerate(KILL):
        ref.params["encoder_bias"][g, idx] = -1e4
    pool = _data(d, seed=6)
    plans = []
    plan = rs.plan_resample

    def spy(*a, **k):
        plans.append(plan(*a, **k))
        return plans[-1]

    monkeypatch.setattr(rs, "plan_resample", spy)
    cnt = fused.resample_dead(pool, rule="anthropic")
    assert cnt.tolist() == [len(x) for x in KILL] and len(plans) == 1
    dead_idx, src_idx, cnt2 = plans[0]
    dead = torch.zeros(G, N_DICT, dtype=torch.bool, device=DEV)
    for g, idx in enumerate(KILL):
        dead[g, idx] = True
    scale = rs.resample_scales(ref.params["encoder"], dead, None, rule="anthropic", ratio=0.2)
    mu, nu = ref.optim_states.mu, ref.optim_states.nu
    rs.resample_rows_reference(ref.params, mu, nu, dead_idx, src_idx, cnt2, pool, scale, kind=kind,
                               **rs.RULES["anthropic"])
    x = pool[:B]  # the resampled features fire on their source rows here
    loss_ref, _ = ref.step_batch(x.float())
    out = fused.step_batch(x)
    torch.cuda.synchronize()
    print("losses fused", out[:, :3].tolist(), "ref", {k: v.tolist() for k, v in loss_ref.items()})
    torch.testing.assert_close(out[:, 0], loss_ref["loss"], rtol=3e-2, atol=1e-4)
    torch.testing.assert_close(out[:, 1], loss_ref["l_reconstruction"], rtol=3e-2, atol=1e-4)
    torch.testing.assert_close(out[:, 2], loss_ref["l_l1"], rtol=3e-2, atol=1e-5)
    mu = ref.optim_states.mu
    for k in fused.m:
        for g in range(G):
            a, b = fused.m[k][g].float(), mu[k][g].float().reshape(fused.m[k][g].shape)
            e = float((a - b).norm() / b.norm().clamp_min(1e-30))
            print("first moment", k, g, e)
            assert e <= 5e-2, (k, g, e)


def test_checkpoint_after_resample_resumes_bit_identically():
    d = 256
    sig, models = _models("untied", d)
    a = _engine(sig, models)
    _kill(a)
    xs = _data(d, seed=7, batches=3)
    a.step_batch(xs[:B])
    a.resample_dead(_data(d, seed=8), rule="anthropic")
    sd = copy.deepcopy(a.state_dict())
    b = _engine(sig, models)
    b.load_state_dict(sd)
    for i in (1, 2):
        a.step_batch(xs[i * B:(i + 1) * B])
        b.step_batch(xs[i * B:(i + 1) * B])
    torch.cuda.synchronize()
    sa, sb = _state_tensors(a), _state_tensors(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.out, b.out)


def test_threshold_engine_is_not_implemented():
    from sparse_coding__amd.engine.fused import FusedSAEEnsemble
    from sparse_coding__amd.models.signatures import FunctionalThresholdingSAE as T

    d = 256
    eng = FusedSAEEnsemble([T.init(d, N_DICT, 1e-3, device=DEV) for _ in range(2)], T, batch_size=B, device=DEV)
    with pytest.raises(NotImplementedError, match="threshold"):
        eng.resample_dead(_data(d))


def test_trainer_fused_returns_host_counts():
    from sparse_coding__amd.engine.trainer import EnsembleTrainer

    d = 256
    sig, models = _models("untied", d)
    tr = EnsembleTrainer(models, sig, batch_size=B, device=DEV)
    assert tr.kind == "fused-sae"
    _kill(tr.impl)
    assert tr.resample_dead(_data(d, seed=9), rule="anthropic") == [len(x) for x in KILL]
