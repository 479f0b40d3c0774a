"""The persistent FISTA solvers (``ops/csrc/fista.hip``) and the dictionary-update kernels
(``ops/csrc/fista_update.hip``) against the fp64 references of ``fista_exact_cases.py``.

Exact tier: every instantiated ``fista_kernel`` / ``fista_gram_kernel`` (one test per instantiation, named after
it) and the edge cases, through ``sc_fista`` / ``sc_coef_search`` / ``sc_fista_gram`` with the operand packing of
``ops/fista.py``; every output -- A, Res, cbar, Vsum as fp32, the slabs as bf16 -- must be ``torch.equal`` to the
reference, which ``test_fista_exact_cpu.py`` proves exact for these inputs.  Only the adjoint's ``epart`` (a sum
of fp32 x bf16 products) carries a bound, derived from the accumulation length.

Realistic tier: one iteration per form and mode on unit-norm random atoms with the real momentum schedule, within
``MARGIN`` x the error of the plain fp32 evaluation of the same recurrence (``real_check_parts``).

Dictionary update: ``sc_hessian_ema`` / ``sc_basis_apply`` within ``MARGIN`` x the error of a plain fp32
evaluation (``step_update_cases.compare``), the bf16 shadow bit-equal to the rounded output."""

import pytest
import torch

import fista_exact_cases as fc
from fista_exact_cases import BF, F32, F64
from step_update_cases import MARGIN, compare, e32_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _id(c):
    return c.name


def _L():
    from sparse_coding__amd.ops import _lib

    return _lib, _lib.lib()


def _frag(M):
    """[G, R, K] bf16 -> MFMA-fragment order [G][R / 16][K / 32][4][16][8] (ops/fista.py)."""
    G, R, K = M.shape
    return M.contiguous().view(G, R // 16, 16, K // 32, 4, 8).permute(0, 1, 3, 4, 2, 5).contiguous()


def _dev(t, dtype=None):
    return None if t is None else t.to(DEV, dtype or t.dtype).contiguous()


def _nan(*shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _report(name, fails, seen, e32):
    for k, obs in seen.items():
        print(f"{name} {k}: E32 {e32[k]:.3e} observed {obs:.3e}")
    assert not fails, "\n".join([name] + fails)


# ===================================================================== launchers (one per entry point)
def run_direct(case, inp):
    """``sc_fista`` (modes 0 / 2) or ``sc_coef_search`` (mode 1) as ``ops.fista`` packs their operands."""
    _lib, L = _L()
    G, B, n, d, T = case.G, case.B, case.n, case.d, case.T
    Xb, Db = _dev(inp["X"], BF), _dev(inp["D"], BF)
    Dfb, Dtb = _frag(Db), _frag(Db.transpose(1, 2))
    a0, eta, lam, mom = _dev(inp["A0"]), _dev(inp["eta"]), _dev(inp["lam"]), _dev(inp["mom"])
    assert mom.numel() >= max(T, 1) and eta.numel() == G and lam.numel() == G
    A, Res = _nan(G, B, n), _nan(G, B, d)
    p, st = _lib.ptr, _lib.stream_handle()
    out = {"A": A, "Res": Res}
    if case.mode == 1:
        rc = L.sc_coef_search(p(Xb), p(Dfb), p(Dtb), p(a0), p(eta), p(lam), p(mom), p(A), p(Res), G, B, n, d, T,
                              inp.get("gscale", fc.GSCALE), inp.get("lscale", fc.LSCALE), st)
    elif case.mode == 2:
        assert T >= 1
        out.update(Ysave=_nan(G, T, B, n, dtype=BF), Rsave=_nan(G, T, B, d, dtype=BF), Asave=_nan(G, T, B, n, dtype=BF))
        rc = L.sc_fista(p(Xb), p(Dfb), p(Dtb), p(a0), p(eta), p(lam), p(mom), p(A), p(Res), G, B, n, d, T,
                        p(out["Ysave"]), p(out["Rsave"]), p(out["Asave"]), st, case.rows)
    else:
        rc = L.sc_fista(p(Xb), p(Dfb), p(Dtb), p(a0), p(eta), p(lam), p(mom), p(A), p(Res), G, B, n, d, T,
                        None, None, None, st, case.rows)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def run_gram(case, inp):
    """``sc_fista_gram`` in its three modes; the wrapper case goes through ``ops.fista.fista(form="gram")``."""
    _lib, L = _L()
    G, B, n, T = case.G, case.B, case.n, case.T
    if case.wrapper:
        from sparse_coding__amd.ops import fista as F

        A, _ = F.fista(_dev(inp["X"]), _dev(inp["D"]), _dev(inp["lam"]), _dev(inp["A0"]), iters=T, eta=_dev(inp["eta"]),
                       backend="hip", with_res=False, form="gram", rows=case.rows)
        torch.cuda.synchronize()
        return {"A": A}
    Gmf = _frag(_dev(inp["Gm"], BF))
    eta, lam, mom = _dev(inp["eta"]), _dev(inp["lam"]), _dev(inp["mom"])
    assert mom.numel() >= max(T, 1)
    p, st = _lib.ptr, _lib.stream_handle()
    if case.mode == 2:
        out = {"cbar": _nan(G, B, n), "Vsum": _nan(G, B, n), "Vslab": _nan(G, T, B, n, dtype=BF),
               "epart": torch.zeros(G, B // 16, device=DEV)}
        V0, As, Qs = _dev(inp["V0"]), _dev(inp["Asave"]), _dev(inp["Qslab"])
        assert As.shape == Qs.shape == (G, T, B, n) and As.dtype == BF and Qs.dtype == BF
        rc = L.sc_fista_gram(None, p(Gmf), p(V0), p(eta), p(lam), p(mom), p(out["cbar"]), G, B, n, T, st, case.rows, 2,
                             p(out["Vslab"]), p(As), p(out["Vsum"]), p(Qs), p(out["epart"]))
    else:
        C, a0 = _dev(inp["C"]), _dev(inp["A0"])
        out = {"A": _nan(G, B, n)}
        slabs = [None] * 3
        if case.mode == 1:
            out.update({k: _nan(G, T, B, n, dtype=BF) for k in ("Ysave", "Asave", "Qslab")})
            slabs = [out["Ysave"], out["Asave"], out["Qslab"]]
        rc = L.sc_fista_gram(p(C), p(Gmf), p(a0), p(eta), p(lam), p(mom), p(out["A"]), G, B, n, T, st, case.rows,
                             case.mode, p(slabs[0]), p(slabs[1]), None, p(slabs[2]), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def _where(case, k, bad):
    """Which models, workgroups, 16-column tiles and slab slots of output k differ (the planted-error table of
    the cases module is the lookup from here)."""
    idx = bad.nonzero()
    R = 16 * case.RT
    parts = [f"{int(bad.sum())} of {bad.numel()} elements", f"models {sorted(set(idx[:, 0].tolist()))}"]
    if bad.dim() == 4:
        parts.append(f"slots {sorted(set(idx[:, 1].tolist()))}")
    parts.append(f"row blocks {sorted(set((idx[:, -2] // R).tolist()))[:12]}")
    parts.append(f"rows in block {sorted(set((idx[:, -2] % R).tolist()))[:32]}")
    parts.append(f"column tiles {sorted(set((idx[:, -1] // 16).tolist()))[:24]}")
    return f"{k}: " + "; ".join(parts)


@pytest.mark.parametrize("case", fc.CASES, ids=_id)
def test_solver_is_bit_exact(case):
    inp = fc.inputs(case)
    ref = fc.evaluate(case, inp, F64, dev=DEV)
    got = (run_direct if case.form == "direct" else run_gram)(case, inp)
    fails = []
    for k in fc.EXACT_OUTPUTS:
        if k not in got:
            continue
        want = ref[k].to(got[k].dtype)          # fp32 as fp32, slabs as bf16 (the reference holds those values)
        assert torch.equal(want.double(), ref[k])
        if not torch.equal(got[k], want):
            fails.append(_where(case, k, ~(got[k] == want)))
    assert not fails, "\n".join([f"{case.name} {case.inst}:"] + fails)
    if case.adjoint:
        R = 16 * case.RT
        assert bool((got["epart"][:, case.B // R:] == 0).all()), "epart: a slot past B / R was written"
        err = (got["epart"].double().sum(1) - ref["epart"].sum(1)).abs()
        bound = fc.epart_bound(case, ref)
        print(f"{case.name} epart.sum(1): |got - ref| = {err.tolist()} bound {bound.tolist()} ref {ref['epart'].sum(1).tolist()}")
        assert bool((err <= bound).all()), (err.tolist(), bound.tolist())


@pytest.mark.parametrize("case", fc.REAL_CASES, ids=_id)
def test_solver_at_realistic_magnitudes(case):
    """One iteration on unit-norm random atoms with the real momentum schedule and eta lam: within MARGIN x the
    error of the plain fp32 evaluation (+ the derived allowance for bf16 roundings that sit on a tie)."""
    inp = fc.real_inputs(case)
    ref, e32, extra, exact = fc.real_check_parts(case, inp, MARGIN)
    out = (run_direct if case.form == "direct" else run_gram)(case, inp)
    got = {k: out[k[3:] if k.startswith("sv_") else k].cpu() for k in ref}
    fails, seen = compare(got, ref, e32, extra=extra, exact=exact)
    _report(f"real {case.name}", fails, seen, e32)
    if case.adjoint:
        full = fc.evaluate(case, inp, F64)
        err = (out["epart"].double().sum(1).cpu() - full["epart"].sum(1)).abs()
        print(f"{case.name} epart.sum(1): |got - ref| = {err.tolist()} bound {fc.epart_bound(case, full).tolist()}")
        assert bool((err <= fc.epart_bound(case, full)).all())


def test_gram_refuses_slabs_without_iterations():
    """Modes 1 and 2 index slab slot T - 1: T = 0 is refused (code 1), nothing is launched."""
    _lib, L = _L()
    x = torch.zeros(16 * 256, device=DEV)
    p = _lib.ptr
    for mode in (1, 2):
        assert L.sc_fista_gram(p(x), p(x), p(x), p(x), p(x), p(x), p(x), 1, 16, 256, 0, _lib.stream_handle(), 0, mode,
                               p(x), p(x), p(x), p(x), p(x)) == 1
    torch.cuda.synchronize()


# ===================================================================== elementwise adjoint kernels
@pytest.mark.parametrize("t", [None, 0, 2, fc.ADJ_T - 1], ids=lambda t: "init" if t is None else f"t{t}")
def test_adjoint_kernels_are_bit_exact(t):
    _lib, L = _L()
    G, B, n, T = fc.ADJ_G, fc.ADJ_B, fc.ADJ_N, fc.ADJ_T
    inp = fc.adjoint_kernel_inputs()
    ref = fc.adjoint_kernel_eval(inp, t)
    T2, Vbar, Yn, As, eta = (_dev(inp[k]) for k in ("T2", "Vbar", "Ynext", "Aslab", "eta"))
    Vs = torch.full((G, T, B, n), 7.0, dtype=BF, device=DEV)
    Ycur, cbar = _nan(G, B, n), _nan(G, B, n)
    p, st = _lib.ptr, _lib.stream_handle()
    if t is None:
        rc = L.sc_fista_adjoint_init(p(T2), p(Vbar), p(As), p(Vs), G, B, n, T, st)
        slot = T - 1
    else:
        rc = L.sc_fista_adjoint(p(T2), p(Vbar), p(Yn), p(Ycur), p(As), p(Vs), p(cbar), p(eta),
                                fc.MOM[t - 1] if t >= 1 else 0.0, fc.MOM[t], G, B, n, T, t, st)
        slot = t - 1
    assert rc == 0
    torch.cuda.synchronize()
    got = {"Vbar": Vbar, "Ycur": Ycur, "cbar": cbar}
    for k, r in ref.items():
        if k == "Vslot":
            assert torch.equal(Vs[:, slot], r.to(DEV, BF)), k
        else:
            assert torch.equal(got[k], r.to(DEV, F32)), k
    untouched = [s for s in range(T) if "Vslot" not in ref or s != slot]
    assert bool((Vs[:, untouched] == 7.0).all()), "a slab slot of another iteration was written"
    if t != 0:
        assert bool(torch.isnan(cbar).all())
    else:
        assert torch.equal(Vbar, _dev(inp["Vbar"]))


# ===================================================================== dictionary update
@pytest.mark.parametrize("shape", fc.HESSIAN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_hessian_ema_against_fp64(shape):
    _lib, L = _L()
    G, B, n = shape
    inp = fc.hessian_inputs(G, B, n)
    ref = fc.hessian_eval(inp, F64)
    e32 = e32_of(fc.hessian_eval(inp, F32), ref)
    A, H = _dev(inp["A"]), _dev(inp["H"]).clone()
    assert L.sc_hessian_ema(_lib.ptr(A), _lib.ptr(H), G, B, n, fc.HISTORY, _lib.stream_handle()) == 0
    torch.cuda.synchronize()
    fails, seen = compare({"H": H.cpu()}, ref, e32)
    _report(f"hessian_ema {shape}", fails, seen, e32)


@pytest.mark.parametrize("case", fc.UPDATE_CASES, ids=_id)
def test_basis_apply_against_fp64(case):
    _lib, L = _L()
    inp = fc.update_inputs(case)
    ref = fc.update_eval(case, inp, F64)
    e32 = e32_of(fc.update_eval(case, inp, F32), ref)
    D, U, H = _dev(inp["D"]).clone(), _dev(inp["U"]), _dev(inp["H"])   # (held: the launch reads them later)
    shadow = torch.full(D.shape, 7.0, dtype=BF, device=DEV) if case.shadow else None
    rc = L.sc_basis_apply(_lib.ptr(D), _lib.ptr(U), _lib.ptr(H), _lib.ptr(shadow), case.G, case.n, case.d, fc.LOWEST,
                          int(case.nonneg), int(case.row_mode), _lib.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(D).all())
    assert bool((D[:, 1] == 0).all()) and bool((D[:, :, 5] == 0).all())   # the norm floors: 0 / floor
    if case.nonneg:
        assert bool((D[:, 2] == 0).all()) and bool((D >= 0).all())
    if case.shadow:
        assert torch.equal(shadow, D.to(BF)), "the bf16 shadow is not the rounded output"
    fails, seen = compare({"D": D.cpu()}, ref, e32)
    _report(f"basis_apply {case.name}", fails, seen, e32)
