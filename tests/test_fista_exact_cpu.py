"""The cases, references, dispatch mirror and planted errors of the FISTA solver tests (``fista_exact_cases.py``),
checked without a GPU: the mirror against the launch tables parsed from fista.hip and the wrapper's shape sets,
a case for every instantiated kernel, every case's proof of exactness, the references against the batched fp32
oracle where no rounding separates them, and every planted error against every case that can see it (a planted
error no case can see is a hole in the cases)."""

import pytest
import torch

import fista_exact_cases as fc
from fista_exact_cases import F32, F64


def _id(c):
    return c.name


_CACHE = {}


def _ref(case):
    """(inputs, reference, checker) of a case, computed once."""
    if case.name not in _CACHE:
        inp = fc.inputs(case)
        _CACHE[case.name] = (inp,) + fc.check_exact(case, inp)
    return _CACHE[case.name]


# --------------------------------------------------------------------- dispatch mirror
def test_mirror_matches_launch_tables():
    from sparse_coding__amd.ops import fista as F

    direct, gram = fc.parsed_tables()
    assert gram == fc.GRAM_TABLE
    assert {("direct",) + k for k in direct} == {k for k in fc.mirror_instantiations() if k[0] == "direct"}
    assert len(direct) == 48 and sum(k[0] == "gram" for k in fc.mirror_instantiations()) == 21
    assert set(fc.DIRECT_RT1) == F.DIRECT_TILES and set(fc.DIRECT_RT2) <= F.DIRECT_TILES
    assert tuple(128 * nw for nw in sorted(fc.GRAM_TABLE)) == tuple(F.GRAM_N)


def test_every_instantiation_has_a_case():
    """Fails when fista.hip gains an instantiation that no case launches."""
    direct, gram = fc.parsed_tables()
    want = {("direct",) + k for k in direct}
    for nw, by_mode in gram.items():
        for m, by_rt in by_mode.items():
            want |= {("gram", nw, rt) + hp + (m,) for rt, hp in by_rt.items() if hp is not None}
    # T >= 2 with mom[0] != 0 is the least that exercises an instantiation's momentum and slab slots
    have = {c.key for c in fc.CASES if c.T >= 2 and c.a0 and not c.wrapper}
    assert want - have == set(), f"instantiations without a case: {sorted(want - have)}"
    assert have - want == set()
    held = {c.name for c in fc.INST_CASES if c.T < 3}
    assert held == set(fc.HELD_AT_T2)
    assert all(c.inst != fc.REFUSED for c in fc.CASES)


def test_rows_argument_of_the_gram_launcher():
    """rows = 0 / 16 launch what they launched before rows = 32 was honoured; rows = 32 forces the 32-row kernel
    exactly where one is instantiated for (n, mode) and B % 32 == 0."""
    for nw, by_mode in fc.GRAM_TABLE.items():
        for mode, by_rt in by_mode.items():
            for G, B in ((3, 48), (3, 96), (2, 128), (4, 4096), (16, 1024), (15, 1024), (1, 16384), (1, 16368)):
                before = B % 32 == 0 and G * (B // 32) >= 512  # the heuristic alone (rows != 16)
                for rows in (0, 16, 32):
                    two = {0: before, 16: False, 32: B % 32 == 0}[rows]
                    rt = 2 if two and by_rt[2] is not None else 1
                    assert fc.dispatch("gram", 128 * nw, 128 * nw, mode, G, B, rows) == (nw, rt) + by_rt[rt] + (mode,)
    assert fc.dispatch("gram", 640, 640, 0, 3, 48, 0) == fc.REFUSED
    assert fc.dispatch("direct", 256, 384, 0, 3, 48, 0) == fc.REFUSED
    assert fc.dispatch("direct", 1024, 512, 0, 3, 96, 32)[2] == 2      # 2 x 80 KB of LDS: the limit itself
    assert fc.dispatch("direct", 1024, 1024, 0, 3, 96, 32)[2] == 1     # no 32-row kernel at (8, 8)
    assert fc.dispatch("direct", 256, 256, 1, 3, 96, 32)[2] == 1       # the coefficient search takes no rows
    assert [fc.dispatch("direct", 128 * dw, 2048, 0, 3, 48, 0)[4] for dw in (2, 4, 8)] == [2, 4, 4]


def test_cases_cover_the_edges():
    cs = fc.CASES
    assert {c.T for c in cs} == {0, 1, 2, 3}
    for form in ("direct", "gram"):
        mine = [c for c in cs if c.form == form]
        assert any(not c.a0 for c in mine)
        grids = {c.G * (c.B // (16 * c.RT)) for c in mine}
        assert any(g % 8 == 0 for g in grids) and any(g % 8 for g in grids)
        assert all(c.G >= 3 for c in fc.INST_CASES)
    assert sum(c.wrapper for c in cs) == 1
    m = fc.MOM
    assert m[0] != 0 and len(set(m)) == len(m)
    assert len(set(fc.ETA)) == 3 and len(set(fc.LAM)) == 3 and len({e * l for e, l in zip(fc.ETA, fc.LAM)}) == 3


# --------------------------------------------------------------------- exactness
@pytest.mark.parametrize("case", fc.CASES, ids=_id)
def test_case_is_exact(case):
    inp, ref, chk = _ref(case)
    assert chk.worst < 2.0 ** 24
    # exact in any order: the plain fp32 evaluation of the same recurrence hits the reference's bits
    plain = fc.evaluate(case, inp, F32)
    for k in fc.EXACT_OUTPUTS:
        if k in ref:
            assert torch.equal(plain[k].double(), ref[k]), k
    if case.T >= 1 and not case.wrapper:
        out = ref["cbar" if case.adjoint else "A"]
        frac = float((out != 0).double().mean())
        assert 0.05 < frac < 0.99, f"both branches of the relu / the support mask should be live ({frac:.2f} nonzero)"


def test_bf16_rounding_of_the_iterate_is_live():
    """Were bf16(Y_t) = Y_t, a kernel that forgot to round would pass: count the entries rounding changes."""
    case = next(c for c in fc.CASES if c.name == "gram_n256_r16_m1")
    inp, ref, _ = _ref(case)
    s = fc._Steps(None, F64)
    e, lam, thr, mom = fc._params(case, inp, F64, None, s)
    Y = A = inp["A0"].double()
    for t in range(2):
        Q = inp["C"].double() - torch.bmm(fc.bf(Y), inp["Gm"].double())
        A, Y = fc._fista_update(case, s, Y, Q, A, A, e, thr, mom[t], t, None, True)
    nz = Y != 0
    changed = float((fc.bf(Y) != Y)[nz].double().mean())
    assert 0.2 < changed < 0.9, changed
    assert torch.equal(fc.bf(Y), ref["Ysave"][:, 2])


def test_check_exact_refuses_inexact_inputs():
    case = next(c for c in fc.CASES if c.name == "direct_2x2_r16_m2")
    inp = fc.inputs(case)
    fc.check_exact(case, inp)
    bad = dict(inp, X=inp["X"].clone())
    bad["X"][0, 0, 0] = 1.0 / 3.0          # not a bf16 value
    with pytest.raises(AssertionError):
        fc.check_exact(case, bad)
    bad = dict(inp, eta=torch.tensor([0.25, 0.3, 0.5]))   # eta Z and eta lam round in fp32
    with pytest.raises(AssertionError):
        fc.check_exact(case, bad)
    bad = dict(inp, A0=inp["A0"] * (1 + 2.0 ** -7) * 2.0 ** 12)  # bf16-exact operands whose sums need > 24 bits
    with pytest.raises(AssertionError, match="2\\^24"):
        fc.check_exact(case, bad)
    gcase = next(c for c in fc.CASES if c.name == "gram_n256_r16_m2")
    ginp = fc.inputs(gcase)
    bad = dict(ginp, V0=ginp["V0"] * (1.0 + 2.0 ** -20))
    with pytest.raises(AssertionError):
        fc.check_exact(gcase, bad)


# --------------------------------------------------------------------- references against the oracle
@pytest.mark.parametrize("form", ["direct", "gram"])
def test_reference_matches_fp32_oracle_at_one_iteration(form):
    """At T = 1 the only operand is the integer warm start (its bf16 rounding is the identity), so A_1 of the
    references equals the batched fp32 oracle's wherever the residual was a bf16 value; the direct and the Gram
    reference agree with each other the same way."""
    from sparse_coding__amd.ops import fista as F

    case = next(c for c in fc.CASES if c.name == f"{form}_T1_m0")
    inp, ref, _ = _ref(case)
    A, _ = F.fista_torch(inp["X"].double(), inp["D"].double(), inp["lam"].double(), inp["A0"].double(), iters=1,
                         eta=inp["eta"].double())
    if form == "gram":
        assert torch.equal(A.double(), ref["A"])
    else:
        res0 = inp["X"].double() - torch.bmm(inp["A0"].double(), inp["D"].double())
        rows = (fc.bf(res0) == res0).all(-1)
        assert bool(rows.any()) and torch.equal(A.double()[rows], ref["A"][rows])


def test_adjoint_reference_matches_autograd():
    """The mode-2 recurrence is the adjoint of the Gram iteration: autograd through the unrolled fp64 loop (the
    forward's supports as fixed masks, no bf16 rounding) gives the reference's cbar in every row whose Vbar_0
    the bf16 rounding of the product operand left unchanged (a sparse seed keeps many such rows)."""
    case = next(c for c in fc.CASES if c.name == "gram_T2_m2")
    inp = fc.inputs(case)
    keep = torch.rand(inp["V0"].shape, generator=fc._gen("adjoint seed")) < 0.03
    inp = dict(inp, V0=inp["V0"] * keep)
    ref = fc.evaluate(case, inp, F64)
    e, mom = inp["eta"].double()[:, None, None], [float(m) for m in fc.MOM]
    Gm, C = inp["Gm"].double(), inp["C"].double()
    supp = inp["Asave"].double() != 0
    c = inp["A0"].double().requires_grad_()
    A_prev, Y = c, c
    for t in range(case.T):
        A = (Y + e * (C - torch.bmm(Y, Gm))) * supp[:, t]
        Y = A + (A - A_prev) * mom[t]
        A_prev = A
    (A * inp["V0"].double()).sum().backward()   # dL / dV_{T-1} = V0 (it lies on the support of A_T)
    V0 = inp["V0"].double()
    V1 = (1 + mom[0]) * (V0 - e * torch.bmm(V0, Gm)) * supp[:, 0]
    assert torch.equal(fc.bf(V1), ref["Vslab"][:, 0]) and torch.equal(ref["Vsum"], V0 + V1)
    rows = (fc.bf(V1) == V1).all(-1)
    assert float(rows.double().mean()) > 0.25 and bool((V1[rows] != 0).any())
    assert torch.equal(c.grad[rows], ref["cbar"][rows])


# --------------------------------------------------------------------- planted errors
def _differs(ref, got):
    return any(k in ref and not torch.equal(ref[k], got[k]) for k in fc.EXACT_OUTPUTS)


@pytest.mark.parametrize("case", fc.CASES, ids=_id)
def test_planted_errors_are_visible(case):
    inp, ref, _ = _ref(case)
    blind = [m for m in fc.MUTATIONS if fc.reachable(case, m) and not _differs(ref, fc.evaluate(case, inp, F64, mut=m))]
    assert not blind, f"{case.name}: planted errors that change no compared output: {blind}"


def test_planted_errors_all_reachable():
    for m in fc.MUTATIONS:
        assert any(fc.reachable(c, m) for c in fc.CASES), m
    # every instantiation sees the errors that concern its own geometry
    for c in fc.INST_CASES:
        assert fc.reachable(c, "tile_swap") and fc.reachable(c, "kstep_dropped") and fc.reachable(c, "mom_next")
        assert fc.reachable(c, "row_tile_alias") == (c.RT == 2)
        if c.T == 3:
            assert fc.reachable(c, "aprev_frozen_pass") == (c.passes > 1)


# --------------------------------------------------------------------- elementwise adjoint + dictionary update
def test_adjoint_kernel_reference_is_exact_and_sees_the_slot():
    inp = fc.adjoint_kernel_inputs()
    assert (fc.ADJ_G * fc.ADJ_B * fc.ADJ_N) % 256
    for t in (None, 0, 2, fc.ADJ_T - 1):
        ref = fc.adjoint_kernel_eval(inp, t)   # (asserts every step representable in fp32)
        assert all(torch.equal(v.float().double(), v) for v in ref.values())
    for t in (2, fc.ADJ_T - 1):  # the support of A_t comes from slot t - 1
        assert not torch.equal(fc.adjoint_kernel_eval(inp, t)["Vbar"], fc.adjoint_kernel_eval(inp, t, mut="slot")["Vbar"])
    v = fc.adjoint_kernel_eval(inp, 2)["Vbar"]
    assert 0.1 < float((v == 0).double().mean()) < 0.6


@pytest.mark.parametrize("case", fc.UPDATE_CASES, ids=_id)
def test_update_reference_matches_torch_path(case):
    """``update_eval`` against the torch branch of ``quadratic_basis_update`` (it works in fp32), fed a Res / A
    pair whose step Res^T A / B is the case's dBt; the two differ only where the torch branch has no floor (the
    zero column divides 0 by 0 there)."""
    from sparse_coding__amd.ops import fista as F

    inp = fc.update_inputs(case)
    ref = fc.update_eval(case, inp, F64)["D"]
    G, n, d = case.G, case.n, case.d
    A = torch.eye(n, dtype=F64).expand(G, n, n).contiguous()          # B = n rows: Res^T A / B = Res^T / n
    Res = inp["U"].double() * n
    got = F.quadratic_basis_update(inp["D"].double(), Res, A, inp["H"].double(), fc.LOWEST, 1.0, case.nonneg,
                                   "row" if case.row_mode else "column", backend="torch")
    live = torch.isfinite(got)
    assert float(live.double().mean()) > 0.9
    torch.testing.assert_close(got[live].double(), ref[live], rtol=2e-5, atol=1e-7)
    assert bool((ref[~live] == 0).all())
    assert bool((ref[:, 1] == 0).all()) and bool((ref[:, :, 5] == 0).all())
    assert bool((ref[:, 2] == 0).all()) == case.nonneg


@pytest.mark.parametrize("shape", fc.HESSIAN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_hessian_reference_matches_torch_path(shape):
    from sparse_coding__amd.ops import fista as F

    inp = fc.hessian_inputs(*shape)
    ref = fc.hessian_eval(inp, F64)["H"]
    got = F.hessian_ema(inp["H"].double(), inp["A"].double(), fc.HISTORY, backend="torch")
    torch.testing.assert_close(got, ref, rtol=1e-6, atol=0)   # (the launcher's factors are fp32 values)
    assert shape[1] % 4 and bool((inp["A"][:, :, 3] == 0).all())


# --------------------------------------------------------------------- realistic magnitudes, T = 1
def _real_got(case, out, names):
    return {k: (out[k] if not k.startswith("sv_") else out[k[3:]].to(torch.bfloat16)) for k in names}


@pytest.mark.parametrize("case", fc.REAL_CASES, ids=_id)
def test_real_tier_bound_admits_plain_and_refuses_planted_errors(case):
    from step_update_cases import MARGIN, compare

    assert case.T == 1 and case.inst != fc.REFUSED
    inp = fc.real_inputs(case)
    assert float(inp["mom"][0]) == 0.0   # the schedule's first entry: no momentum term at T = 1
    thr = inp["eta"].double() * inp["lam"].double()
    assert not torch.equal(thr.float().double(), thr)   # eta lam rounds in fp32
    ref, e32, extra, exact = fc.real_check_parts(case, inp, MARGIN)
    fails, _ = compare(_real_got(case, fc.evaluate(case, inp, F32), ref), ref, e32, extra=extra, exact=exact)
    assert not fails, fails
    for k, x in extra.items():   # the allowance for flipped bf16 roundings touches few entries
        assert float((x > 0).double().mean()) < 0.5 or k == "Res", k
    for mut in ("eta_neighbour", "lam_neighbour", "tile_swap", "kstep_dropped", "kstep_doubled"):
        if not fc.reachable(case, mut):
            continue
        bad = fc.evaluate(case, inp, F64, mut=mut)
        fails, _ = compare(_real_got(case, bad, ref), ref, e32, extra=extra, exact=exact)
        assert fails, f"{case.name}: the bound lets the planted error {mut} through"
