"""The references, the comparator and the cases of the end-of-step update tests (``step_update_cases.py``),
checked without a GPU: the references against autograd, the exact tier's conditions, the plain evaluation
against the comparator, every planted error against the same comparator (a planted error no case can see is
a hole in the cases), and the host gates on the row width against the kernels' instantiated widths."""

import pytest
import torch

import step_update_cases as sc
from step_update_cases import F32, F64


def _id(c):
    return c.name


def _row_got(case, inp, dtype, mut=None):
    out = sc.row_eval(case, inp, dtype, mut)
    return {k: v for k, v in out.items() if not k.startswith(("dp", "floor"))}


# --------------------------------------------------------------------- references against autograd
@pytest.mark.parametrize("case", [c for c in sc.ROW_CASES if c.special and not c.gbf16][:3], ids=_id)
def test_row_reference_matches_autograd(case):
    inp = sc.row_inputs(case)
    ref = sc.row_eval(case, inp, F64)
    bc1, bc2 = 1 - case.b1 ** case.t, 1 - case.b2 ** case.t
    lr = inp["lr"].double()[sc.row_models(case)][:, None]
    for s, st in enumerate(inp["sets"]):
        p = st["p"].double().requires_grad_()
        g_hat = st["g"].double().sum(0)
        w = p / torch.clamp(p.norm(dim=-1, keepdim=True), min=1e-8) if st["norm"] else p
        (w * g_hat).sum().backward()
        g = p.grad
        m = case.b1 * st["m"].double() + (1 - case.b1) * g
        v = case.b2 * st["v"].double() + (1 - case.b2) * g * g
        p_new = p.detach() - lr * (m / bc1) / ((v / bc2).sqrt() + sc.EPS)
        for k, x in (("m", m), ("v", v), ("p", p_new)):
            torch.testing.assert_close(ref[f"{k}{s}"], x, rtol=1e-8, atol=1e-300)
        if st["norm"]:
            nrm = ref[f"p{s}"].norm(dim=-1)
            torch.testing.assert_close(ref[f"norms{s}"], nrm, rtol=1e-12, atol=0)
            torch.testing.assert_close(ref[f"sv{s}"], ref[f"p{s}"] / nrm[:, None], rtol=1e-12, atol=1e-300)
        else:
            assert torch.equal(ref[f"sv{s}"], ref[f"p{s}"])
        assert bool(ref[f"floor{s}"].any()) == bool(st["norm"])  # rows 1 and 3 sit on the floor


@pytest.mark.parametrize("case", sc.BIAS_CASES[:-1], ids=_id)
def test_bias_reference_matches_autograd(case):
    inp = sc.bias_inputs(case)
    ref = sc.bias_eval(case, inp, F64)
    b = inp["b"].double().requires_grad_()
    beta = inp["bias_decay"].double()
    ((beta * b.norm(dim=-1)).sum() + inp["gscale"] * (inp["colpart"].double().sum(1) * b).sum()).backward()
    g = b.grad
    assert bool(torch.isfinite(g).all())
    m = sc.B1 * inp["m"].double() + (1 - sc.B1) * g
    v = sc.B2 * inp["v"].double() + (1 - sc.B2) * g * g
    b_new = b.detach() - inp["lr"].double()[:, None] * (m / (1 - sc.B1 ** case.t)) / (
        (v / (1 - sc.B2 ** case.t)).sqrt() + sc.EPS)
    for k, x in (("m", m), ("v", v), ("b", b_new)):
        torch.testing.assert_close(ref[k], x, rtol=1e-10, atol=1e-300)
    l_rec = inp["dec_part"].double().sum(1) / (case.B * case.d)
    l_l1 = inp["l1"].double() * inp["enc_part"].double()[..., 0].sum(1) / case.B
    l_bd = beta * inp["b"].double().norm(dim=-1)
    for i, x in enumerate((l_rec + l_l1 + l_bd, l_rec, l_l1, l_bd, inp["enc_part"].double()[..., 1].sum(1) / case.B,
                           inp["b"].double().norm(dim=-1))):
        torch.testing.assert_close(ref[f"out{i}"], x, rtol=1e-12, atol=0)
    if case.counting:
        assert torch.equal(ref["count"], inp["feat_count"].double() + inp["cnt_part"].double().sum(1))


# --------------------------------------------------------------------- exact tier
@pytest.mark.parametrize("case", sc.EXACT_ROW_CASES, ids=_id)
def test_exact_conditions(case):
    inp = sc.row_inputs(case)
    sc.check_exact(case, inp)
    # exact in any order: the plain fp32 evaluation hits the reference's bits too
    plain, ref = sc.row_eval(case, inp, F32), sc.row_eval(case, inp, F64)
    for k in sc.row_exact_names(case):
        assert torch.equal(plain[k], ref[k].float()), k


def test_check_exact_refuses_inexact_inputs():
    case = sc.EXACT_ROW_CASES[0]
    inp = sc.row_inputs(case)
    inp["sets"][0]["g"][0, 0, 0] += 1.0  # odd
    with pytest.raises(AssertionError):
        sc.check_exact(case, inp)
    inp = sc.row_inputs(case)
    inp["sets"][0]["p"][0, 5] = 3.0  # not 2^k e_j
    with pytest.raises(AssertionError):
        sc.check_exact(case, inp)


# --------------------------------------------------------------------- comparator: passes and must be able to fail
@pytest.mark.parametrize("case", sc.ALL_ROW_CASES, ids=_id)
def test_row_plain_passes_and_mutations_fail(case):
    inp = sc.row_inputs(case)
    ref, e32, floor_rows, extra = sc.row_check_parts(case, inp)
    kw = dict(extra=extra, floor_rows=floor_rows, exact=sc.row_exact_names(case))
    fails, _ = sc.compare(_row_got(case, inp, F32), ref, e32, **kw)
    assert not fails, fails
    if not case.exact:
        for s in range(len(case.norm)):  # the recipe's scale: the update dominates ulp(p)
            assert 1e-7 < e32[f"p{s}"] < 2e-4, e32
    for mut in sc.ROW_MUTATIONS:
        if not sc.row_reachable(case, mut):
            continue
        fails, _ = sc.compare(_row_got(case, inp, F64, mut), ref, e32, **kw)
        assert fails, f"planted error {mut!r} is invisible in {case.name}"
        if mut == "shadow_of_old_p":  # only the shadows (and the row norms) can tell
            assert all(f.startswith(("sv", "norms")) for f in fails), fails


def test_row_mutations_all_reachable():
    for mut in sc.ROW_MUTATIONS:
        assert any(sc.row_reachable(c, mut) for c in sc.ROW_CASES), mut
    for t in sc.STEPS:
        for dev in (False, True):
            assert any(c.t == t and c.device_step == dev for c in sc.ROW_CASES)
    assert {c.d for c in sc.ROW_CASES} >= set(sc.parsed_widths()["SC_ADAM"])


@pytest.mark.parametrize("case", sc.BIAS_CASES, ids=_id)
def test_bias_plain_passes_and_mutations_fail(case):
    inp = sc.bias_inputs(case)
    ref, e32, extra = sc.bias_check_parts(case, inp)
    plain = sc.bias_eval(case, inp, F32)
    fails, _ = sc.compare(plain, ref, e32, extra=extra)
    assert not fails, fails
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    for mut in sc.BIAS_MUTATIONS:
        if not sc.bias_reachable(case, mut):
            continue
        fails, _ = sc.compare(sc.bias_eval(case, inp, F64, mut), ref, e32, extra=extra)
        assert fails, f"planted error {mut!r} is invisible in {case.name}"


def test_bias_mutations_all_reachable():
    for mut in sc.BIAS_MUTATIONS:
        assert any(sc.bias_reachable(c, mut) for c in sc.BIAS_CASES), mut


def test_compare_reports_nan_and_shadow_half_ulp():
    ref = {"sv0": torch.tensor([[1.0 + 2.0 ** -9, 0.3]], dtype=F64), "p0": torch.tensor([[1.0]], dtype=F64)}
    e32 = {"sv0": 0.0, "p0": 0.0}
    ok = {"sv0": torch.tensor([[1.0, 0.30078125]]).to(torch.bfloat16), "p0": torch.tensor([[1.0]])}
    assert not sc.compare(ok, ref, e32)[0]
    off = {"sv0": torch.tensor([[1.0078125, 0.30078125]]).to(torch.bfloat16), "p0": torch.tensor([[float("nan")]])}
    fails, _ = sc.compare(off, ref, e32)
    assert len(fails) == 2  # the second-nearest bf16, and the NaN


# --------------------------------------------------------------------- host gates against the instantiations
def test_row_width_gates_match_instantiations():
    from sparse_coding__amd.ops import adam as adam_ops

    w = sc.parsed_widths()
    assert w["SC_ADAM"] == (256, 512, 768, 1024, 1536, 2048, 4096) and w["SC_TAIL"] == (256, 512, 768, 1024)
    assert tuple(sorted(adam_ops.ROW_WIDTHS)) == w["SC_ADAM"] and tuple(sorted(adam_ops.TAIL_WIDTHS)) == w["SC_TAIL"]
    lr = torch.ones(1)
    for d in list(range(128, 8192 + 1, 128)) + [0, 4, 100, 260]:
        assert adam_ops.row_width_supported(d) == (d in w["SC_ADAM"])
        assert adam_ops.tail_width_supported(d) == (d in w["SC_TAIL"])
        if d and not adam_ops.row_width_supported(d):  # refused by name before any launch
            z = torch.zeros(1, 1, d)
            with pytest.raises(ValueError, match="row widths"):
                adam_ops.adam_rows([dict(p=z, g=z, m=z, v=z, shadow=None, norms=None, norm=False)], lr, 1)
        if d and not adam_ops.tail_width_supported(d):
            z = torch.zeros(1, 32, d)
            with pytest.raises(ValueError, match="row width"):
                adam_ops.topk_tail(z, z, z, z, z.to(torch.bfloat16), torch.zeros(1, 32), lr, 0.9, 0.999, 1e-8,
                                   torch.zeros(1, dtype=torch.int32), torch.zeros(1, 4), torch.zeros(1), 1.0,
                                   torch.zeros(adam_ops.TICKET_INTS, dtype=torch.int32))
            with pytest.raises(ValueError, match="row width"):
                adam_ops.step_tail([dict(p=z, g=z, m=z, v=z, shadow=None, norms=None, norm=False)], lr, 0.9, 0.999,
                                   1e-8, torch.zeros(1, dtype=torch.int32), *[torch.zeros(1, 32)] * 3,
                                   torch.zeros(1, 1, 32), torch.zeros(1, 1, 2), torch.zeros(1, 1), lr, lr,
                                   torch.zeros(1, 6), 128, 1.0, torch.zeros(2, 1, 1),
                                   torch.zeros(adam_ops.TICKET_INTS, dtype=torch.int32))


def test_engine_gates_ask_the_predicate():
    """No engine keeps a row-width gate of its own in front of a row-Adam launch."""
    import inspect

    from sparse_coding__amd.engine import fused, topk, unrolled

    for mod in (fused, topk, unrolled):
        src = inspect.getsource(mod)
        assert "row_width_supported" in src, mod.__name__
        assert "<= 4096" not in src.replace("n <= 4096", ""), mod.__name__
