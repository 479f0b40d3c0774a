"""Launch policies of the row-Adam kernels (``ops.adam`` POLICY_*: streamed p / m / v loads and stores)
change cache hints only: every policy bit combination writes the bits of the plain policy.  The shapes are the smallest at which the index math can go wrong (a role offset that is no
multiple of 8, G below, at and above 8, one and two sets, every row width NV = d / 256 of the tail, a
compacted masked grid, a row shard with a partial last block)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
POLICIES = tuple(range(4))


@pytest.fixture(autouse=True)
def _restore_policy():
    from sparse_coding__amd.ops import adam as adam_ops

    before = adam_ops.policy()
    yield
    adam_ops.set_policy(before)


def _batches(B, d, steps=3, seed=5):
    g = torch.Generator(device=DEV).manual_seed(seed)
    feats = torch.nn.functional.normalize(torch.randn(1024, d, device=DEV, generator=g), dim=-1)
    return [(torch.relu(torch.randn(B, 1024, device=DEV, generator=g) - 2.0) @ feats).to(torch.bfloat16)
            for _ in range(steps)]


def _state(e):
    """Everything the end-of-step update writes: masters, both moments (the bias and its moments among
    them), bf16 shadows, row norms, the loss terms and the feature counts."""
    s = {f"p.{k}": v for k, v in e.params.items()}
    s.update({f"m.{k}": v for k, v in e.m.items()})
    s.update({f"v.{k}": v for k, v in e.v.items()})
    s["enc_shadow"], s["norms"], s["out"], s["counts"] = e.enc_shadow, e.norms, e.out, e.feature_counts
    if e.kind == "untied":
        s["dec_shadow"] = e.dec_shadow
    return {k: v.clone() for k, v in s.items()}


def _run(models, sig, B, xs, policy, fused_tail):
    """Steps an engine built from ``models`` over ``xs`` under ``policy``; its state after the first
    step and after the last (the latter with every step's loss terms as ``outs``)."""
    from sparse_coding__amd.engine.fused import FusedSAEEnsemble
    from sparse_coding__amd.ops import adam as adam_ops

    adam_ops.set_policy(policy)
    e = FusedSAEEnsemble(models, sig, lr=1e-3, batch_size=B, device=DEV, count_every=2, fused_tail=fused_tail)
    assert e._tail_ok == fused_tail
    outs, first = [], None
    for x in xs:
        outs.append(e.step_batch(x).clone())
        first = first or _state(e)
    torch.cuda.synchronize()
    assert int(e.step_dev.item()) == len(xs)
    assert not fused_tail or not e._ticket.any()
    last = _state(e)
    last["outs"] = torch.stack(outs)
    return first, last


def _case(name):
    from sparse_coding__amd.models.signatures import FunctionalMaskedTiedSAE, FunctionalSAE, FunctionalTiedSAE

    torch.manual_seed(31)
    if name == "masked":  # live sizes 100 / 256 / 37 of 256: the compacted grid, 25-, 64- and 10-block models
        sig, d = FunctionalMaskedTiedSAE, 512
        models = [sig.init(d, s, 256, 1e-3, device=DEV) for s in MASKED_SIZES]
    else:
        G, n, d, kind = name
        sig = FunctionalSAE if kind == "untied" else FunctionalTiedSAE
        models = [sig.init(d, n, l1, device=DEV) for l1 in torch.logspace(-4, -2, G).tolist()]
    return models, sig, 128, _batches(128, d)


MASKED_SIZES = (100, 256, 37)
CASES = [
    (3, 256, 256, "untied"),    # role offset 3 + 3 * 8 = 27; NV = 1
    (8, 128, 512, "untied"),    # 32 row blocks per set and model
    (5, 384, 512, "untied"),    # G does not divide 8
    (16, 128, 512, "tied"),     # one set; G > 8
    (2, 128, 1024, "untied"),   # NV = 4
    "masked",
]
_ids = [c if isinstance(c, str) else "-".join(map(str, c)) for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_every_policy_writes_the_plain_tails_bits(case):
    """``fused_tail=True`` under the default policy and under every policy bit combination against the
    plain policy (0: the kernels as they were before there was a policy), over three eager steps: bitwise
    on masters, moments, shadows, row norms, bias and its moments, every step's loss terms and the feature
    counts.  And against the separate kernels (``fused_tail=False``) after the first step, bitwise on the
    same list (after three: ``test_three_steps_match_separate_kernels``).  Masked: no row past a model's
    live size moves."""
    from sparse_coding__amd.ops import adam as adam_ops

    models, sig, B, xs = _case(case)
    sep_first, _ = _run(models, sig, B, xs[:1], 0, fused_tail=False)
    first0, last0 = _run(models, sig, B, xs, 0, fused_tail=True)
    for k, want in sep_first.items():
        assert torch.equal(first0[k], want), f"step 1, plain policy: {k} differs from the separate kernels"
    for pol in (adam_ops.DEFAULT_POLICY,) + POLICIES:
        first, last = _run(models, sig, B, xs, pol, fused_tail=True)
        for k, want in first0.items():
            assert torch.equal(first[k], want), f"policy {pol}, step 1: {k}"
        for k, want in last0.items():
            assert torch.equal(last[k], want), f"policy {pol}, step 3: {k}"
    if case == "masked":
        init = torch.stack([p["encoder"] for p, _ in models])
        for g, s in enumerate(MASKED_SIZES):
            assert torch.equal(last0["p.encoder"][g, s:], init[g, s:])
            assert not last0["m.encoder"][g, s:].any() and not last0["v.encoder"][g, s:].any()
            assert not torch.equal(last0["p.encoder"][g, :s], init[g, :s])


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_three_steps_match_separate_kernels(case):
    """``fused_tail=True`` under the default policy and every policy bit combination against
    ``fused_tail=False`` over three eager steps, ``torch.equal`` on masters, both moments, bf16 shadows,
    row norms, bias and its moments, ``out`` and the feature counts.

    (The separate ``bias_adam_kernel`` once rounded its moment updates as packed multiplies and adds where
    the tail used fused multiply-adds, and ``loss_reduce_kernel`` summed |b|^2 in another order than the
    tail's per-32-column partials: bias, its moments and |b| then differed in the last bits from the
    second step on, 7e-10 at most on the bias.  Both now share the written-out forms of csrc/adam.hip.)
    """
    from sparse_coding__amd.ops import adam as adam_ops

    models, sig, B, xs = _case(case)
    _, ref = _run(models, sig, B, xs, 0, fused_tail=False)
    bad = []
    for pol in (adam_ops.DEFAULT_POLICY,) + POLICIES:
        _, got = _run(models, sig, B, xs, pol, fused_tail=True)
        for k, want in ref.items():
            ne = got[k] != want
            if ne.any():
                diff = (got[k].float() - want.float()).abs().max().item()
                bad.append(f"policy {pol}: {k}: {int(ne.sum())} of {ne.numel()} differ, max |diff| {diff:.3g}")
    print("\n".join(bad[: len(ref)]))
    assert not bad, f"{len(bad)} tensors differ from the separate kernels; first: {bad[0]}"


def test_every_policy_row_shard_matches_adam_rows():
    """``update(sets=row_sets(lo, hi, grads), row0=lo)`` on a shard that starts inside model 0 and ends
    in a partial block, against ``adam_rows`` on the same shard: bitwise on the shard, nothing outside it
    written."""
    from sparse_coding__amd.engine.fused import FusedSAEEnsemble
    from sparse_coding__amd.models.signatures import FunctionalSAE
    from sparse_coding__amd.ops import adam as adam_ops

    torch.manual_seed(33)
    G, n, d, B = 3, 256, 256, 128
    lo, hi = 40, 40 + 4 * 57 + 2  # crosses into model 1; the last block holds two rows
    models = [FunctionalSAE.init(d, n, l1, device=DEV) for l1 in (1e-4, 1e-3, 1e-2)]
    adam_ops.set_policy(0)
    e = FusedSAEEnsemble(models, FunctionalSAE, lr=1e-3, batch_size=B, device=DEV).use_flat_grads()
    x = e.prepare(e._x_bf16(_batches(B, d, steps=1)[0]))
    e._tail_ready()
    e.forward(x)
    e.backward_weights(x)
    grads = [e.g_dec.view(-1, d)[lo:hi].clone(), e.g_enc.view(-1, d)[lo:hi].clone()]
    keys = ("encoder", "decoder")
    tensors = {f"{w}.{k}": t[k] for w, t in (("p", e.params), ("m", e.m), ("v", e.v)) for k in keys}
    tensors.update(enc_shadow=e.enc_shadow, dec_shadow=e.dec_shadow, norms=e.norms)
    before = {k: t.clone() for k, t in tensors.items()}

    def restore():
        for k, t in tensors.items():
            t.copy_(before[k])
        e.step_dev.zero_()

    adam_ops.adam_rows(e.row_sets(lo, hi, grads), e.lr, 1, *e.betas, e.eps, rows_per_model=n,
                       step_dev=e.step_dev, row0=lo)
    torch.cuda.synchronize()
    want = {k: t.clone() for k, t in tensors.items()}
    rows = lambda t: t.view(G * n, -1)  # noqa: E731
    for k in want:
        assert torch.equal(rows(want[k])[:lo], rows(before[k])[:lo]) and torch.equal(rows(want[k])[hi:],
                                                                                      rows(before[k])[hi:])
        assert not torch.equal(rows(want[k])[lo:hi], rows(before[k])[lo:hi])
    for pol in (adam_ops.DEFAULT_POLICY,) + POLICIES:
        restore()
        adam_ops.set_policy(pol)
        e.update(e.row_sets(lo, hi, grads), row0=lo)
        torch.cuda.synchronize()
        assert int(e.step_dev.item()) == 1
        for k, t in tensors.items():
            assert torch.equal(t, want[k]), f"policy {pol}: {k}"
        restore()
        adam_ops.adam_rows(e.row_sets(lo, hi, grads), e.lr, 1, *e.betas, e.eps, rows_per_model=n,
                           step_dev=e.step_dev, row0=lo)
        torch.cuda.synchronize()
        for k, t in tensors.items():
            assert torch.equal(t, want[k]), f"adam_rows, policy {pol}: {k}"


def test_every_policy_topk_tail_matches_separate_launches():
    """``sc_topk_tail`` (3 models, n = 1024, d = 768) under every policy against the separate Adam launch
    and torch reductions on the plain policy: masters, moments, shadow and row norms bitwise over three
    steps; the MSE (another reduction order in the separate path) to fp32 rounding there, and bitwise
    between the policies."""
    from sparse_coding__amd.engine.topk import FusedTopKEnsemble
    from sparse_coding__amd.models.topk import TopKEncoder
    from sparse_coding__amd.ops import adam as adam_ops

    torch.manual_seed(23)
    d, n, B = 768, 1024, 256
    models = [TopKEncoder.init(d, n, k, device=DEV) for k in (4, 16, 64)]
    xs = [torch.randn(B, d, device=DEV).to(torch.bfloat16) for _ in range(3)]

    def run(pol, fused_tail):
        adam_ops.set_policy(pol)
        e = FusedTopKEnsemble(models, batch_size=B, device=DEV, lr=1e-3, fused_tail=fused_tail)
        assert e._tail == fused_tail
        mse = torch.stack([e.step_batch(x).clone() for x in xs])
        torch.cuda.synchronize()
        assert int(e.step_dev.item()) == len(xs)
        return dict(p=e.params["dict"], m=e.m["dict"], v=e.v["dict"], shadow=e.shadow, norms=e.norms), mse

    ref, ref_mse = run(0, False)
    _, mse0 = run(0, True)
    torch.testing.assert_close(mse0, ref_mse, rtol=1e-5, atol=0)
    for pol in (adam_ops.DEFAULT_POLICY,) + POLICIES:
        got, mse = run(pol, True)
        for k, want in ref.items():
            assert torch.equal(got[k], want), f"policy {pol}: {k}"
        assert torch.equal(mse, mse0), f"policy {pol}: mse"
