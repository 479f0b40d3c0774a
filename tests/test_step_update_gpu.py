"""The end-of-step update kernels (``ops/csrc/adam.hip``, ``row_adam.h``) against the fp64 references of
``step_update_cases.py``, through ``ops.adam`` on synthetic tensors: ``adam_rows``, ``shadow_rows``,
``bias_loss``, ``step_tail`` and ``topk_tail``; then the two engine gates on the row width.  The bound of
every comparison is computed from the inputs alone (``MARGIN * E32``, see the cases module).

``SC_STEP_UPDATE_REPORT=<file>`` writes every case's E32 and the kernel's observed error per tensor as a
markdown table (profiles/r20/step_update/README.md); no test reads it."""

import os
from dataclasses import dataclass
from typing import Optional, Tuple

import pytest
import torch

import step_update_cases as sc
from step_update_cases import BF, F32, F64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("SC_STEP_UPDATE_REPORT")
    if not path or not _REPORT:
        return
    lines = ["| kernel | case | tensor | E32 (CPU, from the inputs) | bound | observed max error (MI355X) | obs / E32 |",
             "|---|---|---|---|---|---|---|"]
    for kern, name, k, e, bound, obs in _REPORT:
        ratio = f"{obs / e:.2f}" if e > 0 else ("0" if obs == 0 else "inf")
        lines.append(f"| {kern} | {name} | {k} | {e:.3e} | {bound} | {obs:.3e} | {ratio} |")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def _check(kern, name, got, ref, e32, extra=None, floor_rows=None, exact=(), collect=None):
    """Compares, prints and records; fails at once, or (``collect``: a list) leaves the failures there for the
    end of a test of several steps."""
    fails, seen = sc.compare(got, ref, e32, extra=extra, floor_rows=floor_rows, exact=exact)
    for k, obs in seen.items():
        bound = "bit-equal" if k in exact else ("4 E32" + (" + bc" if extra and k in extra else "")
                                                + (" + bf16 half ulp" if k.startswith("sv") else ""))
        print(f"{kern} {name} {k}: E32 {e32.get(k, 0.0):.3e} observed {obs:.3e} ({bound})")
        _REPORT.append((kern, name, k, e32.get(k, 0.0), bound, obs))
    if collect is not None:
        collect.extend(f"{kern} {name}: {f}" for f in fails)
        return
    assert not fails, "\n".join([f"{kern} {name}:"] + fails)


def _id(c):
    return c.name


# ===================================================================== adam_rows
def _launch_rows(case, inp, launch):
    """Puts a row case on the device, runs ``launch(sets, lr, kw)`` and returns the kernel's tensors on the
    CPU as ``compare`` wants them, after the checks no tolerance applies to (rows the update must not touch)."""
    R, d, ns = case.R, case.d, case.nsplit
    shape = (R, d) if (case.rows is not None or case.n == 1) else (case.G, case.n, d)
    gstride = R * d + 192 if ns > 1 else 0  # slabs further apart than the tensor
    sets = []
    for st in inp["sets"]:
        gbuf = torch.full((max(ns * gstride, R * d),), float("nan"), dtype=st["g"].dtype, device=DEV)
        for i in range(ns):
            gbuf[i * gstride:i * gstride + R * d] = st["g"][i].reshape(-1).to(DEV)
        sets.append(dict(p=st["p"].to(DEV).view(shape).clone(), g=gbuf[:R * d].view(shape),
                         m=st["m"].to(DEV).view(shape).clone(), v=st["v"].to(DEV).view(shape).clone(),
                         shadow=torch.full(shape, 7.0, dtype=BF, device=DEV),
                         norms=torch.full(shape[:-1], -3.0, device=DEV) if st["norm"] else None, norm=st["norm"]))
    kw = dict(rows_per_model=case.n, nsplit=ns, gstride=gstride,
              live=torch.tensor(case.live, dtype=torch.int32, device=DEV) if case.live else None)
    launch(sets, inp["lr"].to(DEV), kw)
    torch.cuda.synchronize()
    act = sc.row_active(case)
    got = {}
    for s, (st, ds) in enumerate(zip(inp["sets"], sets)):
        for k in ("p", "m", "v"):
            x = ds[k].cpu().view(R, d)
            assert torch.equal(x[~act], st[k][~act]), f"{k}{s}: a row past the live count changed"
            assert bool(torch.isfinite(x).all()), f"{k}{s} not finite"
            got[f"{k}{s}"] = x
        sh = ds["shadow"].cpu().view(R, d)
        assert bool((sh[~act] == 7.0).all()), f"shadow{s}: a row past the live count was written"
        got[f"sv{s}"] = sh
        if st["norm"]:
            nr = ds["norms"].cpu().view(R)
            assert bool((nr[~act] == -3.0).all()), f"norms{s}: a row past the live count was written"
            got[f"norms{s}"] = nr
        if case.special and act[2]:  # zero g / m / v: exactly unchanged
            assert torch.equal(got[f"p{s}"][2], st["p"][2]) and not bool(got[f"m{s}"][2].any()) \
                and not bool(got[f"v{s}"][2].any())
    return got, act


def _check_rows(kern, case, inp, got, act, collect=None):
    ref, e32, floor_rows, extra = sc.row_check_parts(case, inp)
    for k in got:  # rows the update skips have no norm / shadow to compare
        if k.startswith(("sv", "norms")):
            got[k] = got[k].clone().double()
            got[k][~act] = ref[k][~act]
    if case.special:
        assert any(bool(m.any()) for m in floor_rows.values()), "no row on the norm floor"
    _check(kern, case.name, got, ref, e32, extra, floor_rows, sc.row_exact_names(case), collect)


@pytest.mark.parametrize("case", sc.ALL_ROW_CASES, ids=_id)
def test_adam_rows(case):
    from sparse_coding__amd.ops import adam as adam_ops

    inp = sc.row_inputs(case)
    if case.exact:
        sc.check_exact(case, inp)

    def launch(sets, lr, kw):
        if case.device_step:  # the host step is ignored beside a device counter
            kw["step_dev"] = torch.tensor([case.t - 1], dtype=torch.int32, device=DEV)
        adam_ops.adam_rows(sets, lr, case.t + (3 if case.device_step else 0), case.b1, case.b2, sc.EPS,
                           row0=case.row0, **kw)
        if case.device_step:
            assert int(kw["step_dev"]) == case.t - 1  # adam_rows reads the counter, bias_loss advances it

    old = adam_ops.policy()
    try:
        if case.policy is not None:
            adam_ops.set_policy(case.policy)
        got, act = _launch_rows(case, inp, launch)
    finally:
        adam_ops.set_policy(old)
    _check_rows("adam_rows", case, inp, got, act)


def test_adam_rows_refuses_unsupported_width():
    from sparse_coding__amd.ops import adam as adam_ops

    z = torch.zeros(2, 4, 1280, device=DEV)
    with pytest.raises(ValueError, match="row widths"):
        adam_ops.adam_rows([dict(p=z, g=z, m=z, v=z, shadow=None, norms=None, norm=False)],
                           torch.ones(2, device=DEV), 1)


# ===================================================================== shadow_rows
@pytest.mark.parametrize("d", sc.SHADOW_D)
@pytest.mark.parametrize("rows", sc.SHADOW_ROWS)
def test_shadow_rows(rows, d):
    from sparse_coding__amd.ops import adam as adam_ops

    # the un-normalised copy is a bf16 cast, round to nearest even, bit for bit
    p = sc.shadow_inputs(rows, d, special=True)
    for with_norms in (False, True):
        sh = torch.full((rows, d), 7.0, dtype=BF, device=DEV)
        norms = torch.full((rows,), -3.0, device=DEV) if with_norms else None
        adam_ops.shadow_rows(p.to(DEV), sh, norms, normalize=False)
        want = p.to(BF)
        assert torch.equal(sh.cpu().view(torch.int16), want.view(torch.int16)), (
            p.flatten()[(sh.cpu().view(torch.int16) != want.view(torch.int16)).flatten()][:8])
        assert norms is None or bool((norms == -3.0).all())  # only the normalised form has norms to write
    p = sc.shadow_inputs(rows, d, special=False)
    ref = sc.shadow_eval(p, F64)
    e32 = sc.e32_of(sc.shadow_eval(p, F32), ref)
    for with_norms in (False, True):
        sh = torch.full((rows, d), 7.0, dtype=BF, device=DEV)
        norms = torch.full((rows,), -3.0, device=DEV) if with_norms else None
        adam_ops.shadow_rows(p.to(DEV), sh, norms, normalize=True)
        got = {"sv": sh.cpu()}
        if with_norms:
            got["norms"] = norms.cpu()
        _check("shadow_rows", f"rows{rows}_d{d}{'_norms' if with_norms else ''}", got, ref, e32)


# ===================================================================== bias_loss
def _bias_dev(case, inp):
    dv = {k: (v.to(DEV).clone() if torch.is_tensor(v) else v) for k, v in inp.items()}
    dv["out"] = torch.full((case.G, 6), float("nan"), device=DEV)
    return dv


def _bias_got(case, dv):
    got = {"b": dv["b"].cpu(), "m": dv["m"].cpu(), "v": dv["v"].cpu()}
    if case.counting:
        got["count"] = dv["feat_count"].cpu()
    out = dv["out"].cpu()
    got.update({f"out{i}": out[:, i] for i in range(6)})
    assert all(bool(torch.isfinite(x).all()) for x in got.values()), "NaN / inf in the bias update or loss terms"
    return got


@pytest.mark.parametrize("case", sc.BIAS_CASES, ids=_id)
def test_bias_loss(case):
    from sparse_coding__amd.ops import adam as adam_ops

    inp = sc.bias_inputs(case)
    dv = _bias_dev(case, inp)
    step_dev = torch.tensor([case.t - 1], dtype=torch.int32, device=DEV) if case.device_step else None
    adam_ops.bias_loss(dv["b"], dv["m"], dv["v"], dv["colpart"], case.tm, dv["enc_part"], case.enc_tiles,
                       dv["dec_part"], case.dec_tiles, dv["l1"], dv["bias_decay"], dv["lr"], dv["out"], case.B,
                       case.d, case.t + (3 if case.device_step else 0), inp["gscale"],
                       cnt_part=dv["cnt_part"] if case.counting else None,
                       feat_count=dv["feat_count"] if case.counting else None, b1=sc.B1, b2=sc.B2, eps=sc.EPS,
                       step_dev=step_dev)
    torch.cuda.synchronize()
    if case.device_step:  # advanced by exactly one; the bias Adam used the advanced value (the reference's t)
        assert int(step_dev) == case.t
    if not case.counting:
        assert torch.equal(dv["feat_count"].cpu(), inp["feat_count"])
    ref, e32, extra = sc.bias_check_parts(case, inp)
    _check("bias_loss", case.name, _bias_got(case, dv), ref, e32, extra)


# ===================================================================== step_tail
@dataclass(frozen=True)
class TailCase:
    name: str
    G: int
    n: int
    d: int
    norm: Tuple[bool, ...]
    t0: int = 0                       # completed steps before the first tail
    grows: Optional[int] = None       # rows of the next-batch gather
    tm: int = 3
    cnt_tm: Optional[int] = None
    enc_tiles: int = 2
    dec_tiles: int = 3
    live: Optional[Tuple[int, ...]] = None
    row0: int = 0
    rows: Optional[int] = None
    gbf16: bool = False
    nsplit: int = 1
    blocks: Optional[int] = None      # the grid the case is there for


TAIL_CASES = [
    TailCase("g1_n32_d256_10blocks", 1, 32, 256, (True,), blocks=10, tm=1),
    TailCase("g2_63blocks", 2, 32, 512, (True, False), t0=0, grows=107, blocks=63, tm=8),
    TailCase("g2_64blocks", 2, 32, 512, (True, False), t0=9, grows=111, blocks=64, tm=13),
    TailCase("g2_65blocks", 2, 32, 256, (True, False), t0=999, grows=115, blocks=65, tm=1, cnt_tm=5),
    TailCase("g2_129blocks", 2, 32, 768, (True, False), t0=1, grows=371, blocks=129, enc_tiles=255, dec_tiles=256),
    TailCase("g3_n64_d768", 3, 64, 768, (True, False), t0=0, enc_tiles=600, dec_tiles=1),
    TailCase("g3_n64_d1024_one_set", 3, 64, 1024, (True,), t0=8, grows=5),
    TailCase("g1_n64_d1024_bf16_split3", 1, 64, 1024, (True, False), t0=1, gbf16=True, nsplit=3),
    TailCase("live_5_32_0", 3, 32, 512, (True, False), t0=1, live=(5, 32, 0), grows=9),
    TailCase("shard_row0_20", 3, 32, 256, (True, False), t0=998, row0=20, rows=50),
]


def _gather_setup(grows, t0, steps, salt):
    gen = sc._gen("gather", salt)
    buf = torch.randn(300, 64, generator=gen).to(BF)
    perm = torch.randint(0, 300, ((steps + 2) * grows,), generator=gen)
    ep0 = t0 - 1  # the first tail fetches batch 2 of the permutation
    return buf, perm, ep0


@pytest.mark.parametrize("tc", TAIL_CASES, ids=_id)
def test_step_tail(tc):
    from sparse_coding__amd.ops import adam as adam_ops

    G, n, d, steps = tc.G, tc.n, tc.d, 3
    beta = tuple(0.1 if g % 2 == 0 else 0.0 for g in range(G))
    state, bstate, problems = None, None, []
    step_dev = torch.tensor([tc.t0], dtype=torch.int32, device=DEV)
    ticket = torch.zeros(adam_ops.TICKET_INTS, dtype=torch.int32, device=DEV)
    bsq = torch.full((2, G, n // 32), float("nan"), device=DEV)
    if tc.grows:
        buf, perm, ep0 = _gather_setup(tc.grows, tc.t0, steps, tc.name)
        gout = torch.zeros(tc.grows, 64, dtype=BF, device=DEV)
        gather = (buf.to(DEV), perm.to(DEV), torch.tensor([ep0], dtype=torch.int32, device=DEV), gout)
    for k in range(steps):
        t = tc.t0 + k + 1
        case = sc.RowCase(f"{tc.name}_step{k}", d, G=G, n=n, norm=tc.norm, gbf16=tc.gbf16, nsplit=tc.nsplit, t=t,
                          device_step=True, row0=tc.row0, rows=tc.rows, live=tc.live, special=(k == steps - 1))
        inp = sc.row_inputs(case, state)
        bcase = sc.BiasCase(f"{tc.name}_step{k}", n, G=G, tm=tc.tm, cnt_tm=tc.cnt_tm, enc_tiles=tc.enc_tiles,
                            dec_tiles=tc.dec_tiles, beta=beta, zero_model={1: None, 2: 0, 3: 2}[G] if k == 0 else None, t=t,
                            device_step=True, B=256, d=d)
        binp = sc.bias_inputs(bcase)
        if bstate is not None:  # the kernel's own state of the step before, fresh gradients and partials
            binp.update(bstate)
        dv = _bias_dev(bcase, binp)
        if k == 0:
            adam_ops.bias_sq_parts(dv["b"], bsq, tc.t0 & 1)
        blocks = []

        def launch(sets, lr, kw):
            nrows = sets[0]["p"].numel() // d
            arows = len(sets) * (sum(min(n, x) for x in tc.live) if tc.live else nrows)
            blocks.append(G + G * (n // 32) + (arows + 3) // 4 + ((tc.grows + 3) // 4 if tc.grows else 0))
            kw.pop("rows_per_model")
            adam_ops.step_tail(sets, lr, sc.B1, sc.B2, sc.EPS, step_dev, dv["b"], dv["m"], dv["v"], dv["colpart"],
                               dv["enc_part"], dv["dec_part"], dv["l1"], dv["bias_decay"], dv["out"], bcase.B,
                               binp["gscale"], bsq, ticket, cnt_part=dv["cnt_part"], feat_count=dv["feat_count"],
                               gather=gather if tc.grows else None, row0=tc.row0 if tc.rows is not None else None,
                               live_host=list(tc.live) if tc.live else None, **kw)

        binp["lr"] = inp["lr"]  # (one lr vector serves the rows and the bias)
        got, act = _launch_rows(case, inp, launch)
        assert tc.blocks is None or blocks[0] == tc.blocks
        assert int(step_dev) == t and not bool(ticket.any()), "counter / ticket after the tail"
        _check_rows("step_tail", case, inp, got, act, problems)
        ref, e32, extra = sc.bias_check_parts(bcase, binp)
        bgot = _bias_got(bcase, dv)
        _check("step_tail", bcase.name, bgot, ref, e32, extra, collect=problems)
        # the b^2 partials of the new bias at the next step's parity (from the kernel's own new bias)
        # (a few values only, so the bound is the a-priori one of a sum of 32 squares in any order: 32 x 2^-24)
        sq = bgot["b"].double().square().view(G, n // 32, 32).sum(-1)
        assert bool(((bsq[t & 1].cpu().double() - sq).abs() <= 32 * 2.0 ** -24 * sq).all()), "b^2 partials"
        if tc.grows:
            assert torch.equal(gout.cpu(), sc.gather_reference(buf, perm, t - 1, ep0, tc.grows)), "gathered batch"
        state = [{k2: got[f"{k2}{s}"] for k2 in ("p", "m", "v")} for s in range(len(tc.norm))]
        bstate = {"b": bgot["b"], "m": bgot["m"], "v": bgot["v"], "feat_count": bgot["count"]}
    assert not problems, "\n".join(problems)


# ===================================================================== topk_tail
@pytest.mark.parametrize("d,se_rows,with_gather,t0", [(256, 1, False, 0), (768, 255, True, 9), (1024, 257, True, 998)])
def test_topk_tail(d, se_rows, with_gather, t0):
    from sparse_coding__amd.ops import adam as adam_ops

    G, n, steps, grows = 3, 12, 3, 7
    name = f"d{d}_se{se_rows}"
    step_dev = torch.tensor([t0], dtype=torch.int32, device=DEV)
    ticket = torch.zeros(adam_ops.TICKET_INTS, dtype=torch.int32, device=DEV)
    se_scale = sc.f32(1.0 / (se_rows * d))
    if with_gather:
        buf, perm, ep0 = _gather_setup(grows, t0, steps, name)
        gout = torch.zeros(grows, 64, dtype=BF, device=DEV)
        gather = (buf.to(DEV), perm.to(DEV), torch.tensor([ep0], dtype=torch.int32, device=DEV), gout)
    state, problems = None, []
    for k in range(steps):
        t = t0 + k + 1
        case = sc.RowCase(f"topk_{name}_step{k}", d, G=G, n=n, norm=(True,), gbf16=(d == 768),
                          t=t, device_step=True, special=(k == steps - 1))
        inp = sc.row_inputs(case, state)
        row_se = torch.rand(G, se_rows, generator=sc._gen("row_se", name, k)) * 4
        mse = torch.full((G,), float("nan"), device=DEV)

        def launch(sets, lr, kw):
            s = sets[0]
            adam_ops.topk_tail(s["p"], s["g"], s["m"], s["v"], s["shadow"], s["norms"], lr, sc.B1, sc.B2, sc.EPS,
                               step_dev, row_se.to(DEV), mse, se_scale, ticket, gather=gather if with_gather else None)

        got, act = _launch_rows(case, inp, launch)
        assert int(step_dev) == t and not bool(ticket.any()), "counter / ticket after the tail"
        _check_rows("topk_tail", case, inp, got, act, problems)
        ref, e32 = sc.mse_check_parts(row_se, se_scale)
        _check("topk_tail", case.name, {"mse": mse.cpu()}, ref, e32, collect=problems)
        if with_gather:
            assert torch.equal(gout.cpu(), sc.gather_reference(buf, perm, t - 1, ep0, grows)), "gathered batch"
        state = [{k2: got[f"{k2}0"] for k2 in ("p", "m", "v")}]
    assert not problems, "\n".join(problems)


# ===================================================================== engine gates on the row width
def test_threshold_engine_with_unsupported_vector_width_steps():
    """n = 1280 = 256 x 5 has no row-Adam kernel: the activation scale takes the torch form of the update."""
    from sparse_coding__amd.engine.fused import FusedSAEEnsemble
    from sparse_coding__amd.models.signatures import FunctionalThresholdingSAE as T

    torch.manual_seed(3)
    d, n, B = 256, 1280, 128
    models = [T.init(d, n, l1, device=DEV) for l1 in (1e-4, 1e-3)]
    for p, _ in models:
        p["activation_scale"].uniform_(0.7, 1.3)
        p["activation_gain"].uniform_(-0.2, 0.4)
    eng = FusedSAEEnsemble(models, T, lr=[1e-3, 2e-3], batch_size=B, device=DEV)
    s0 = eng.params["activation_scale"].clone()
    x = torch.randn(B, d, device=DEV).to(BF)
    out = eng.step_batch(x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    b1, b2 = eng.betas
    g = eng.dotpart.sum(dim=1) * s0 * (2.0 * eng._alpha)
    assert float(g.abs().max()) > 0
    m, v = (1 - b1) * g, (1 - b2) * g * g
    want = s0 - eng.lr[:, None] * (m / (1 - b1)) / ((v / (1 - b2)).sqrt() + eng.eps)
    torch.testing.assert_close(eng.params["activation_scale"], want, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(eng.m["activation_scale"], m, rtol=1e-5, atol=1e-12)


def test_fused_engines_refuse_unsupported_row_width():
    from sparse_coding__amd.engine.fused import FusedSAEEnsemble
    from sparse_coding__amd.engine.topk import FusedTopKEnsemble
    from sparse_coding__amd.models.signatures import FunctionalSAE
    from sparse_coding__amd.models.topk import TopKEncoder

    models = [FunctionalSAE.init(1280, 128, 1e-3, device=DEV)]
    with pytest.raises(ValueError, match=r"row widths \(256, 512, 768, 1024, 1536, 2048, 4096\)"):
        FusedSAEEnsemble(models, FunctionalSAE, lr=1e-3, batch_size=128, device=DEV)
    models = [TopKEncoder.init(1280, 128, 8, device=DEV)]
    with pytest.raises(ValueError, match=r"row widths \(256, 512, 768, 1024, 1536, 2048, 4096\)"):
        FusedTopKEnsemble(models, lr=1e-3, batch_size=128, device=DEV)
