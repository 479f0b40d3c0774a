"""The kernels of ``ops/csrc/elementwise.hip`` against the references of ``layer_pass_cases.py``: the LISTA
and residual layer passes through ``ops._lib`` exactly as ``engine/unrolled.py`` calls them (``_lib.ptr``,
``None`` for an absent pointer, ``_lib.stream_handle()``, ``_lib.check``), the centring as ``engine/fused.py``
does, the gathers through ``ops.rows``.  Every output buffer is filled with a sentinel first and has slack past
its end that must stay untouched; inputs must come back unchanged.  Every bound is computed from the inputs
alone (see the cases module).

``SC_LAYER_PASS_REPORT=<file>`` writes every case's checks as a markdown table
(profiles/r25/layer_pass/README.md); no test reads it."""

import os

import pytest
import torch

import layer_pass_cases as lp
from layer_pass_cases import BF, F32, SENTINEL, SENTINEL_BYTE, SLACK

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_REPORT = []

_README_HEAD = """# Reference tests of the layer-pass, centring and gather kernels (`ops/csrc/elementwise.hip`)

Written by `tests/test_layer_pass_gpu.py` with `SC_LAYER_PASS_REPORT` set, on an MI355X; no test reads it.
References, tiers, bounds and planted errors: `tests/layer_pass_cases.py`.

Kinds of check:

* **bit-equal to the fp64 reference** -- exact tier (inputs on a 0.25 grid: every product and sum is exact in
  fp32 in any order), reductions included;
* **bit-equal to the fp32 evaluation** -- rounding tier, outputs that are one fp32 operation after exact
  selections;
* **bit-equal to bf16(its fp32 source, as written)** -- a bf16 output against the fp32 output of the same
  launch, raw bits, no tolerance; where the mode omits the source the launch is repeated with it and the bf16
  bits must agree across the two launches;
* **derived bound** -- `abs(kernel - ref64) <= 4 x bound`, the bound from the formula alone; the column shows the
  largest observed error over the bound (1.0 would be the whole first-order bound, 4.0 the limit).

Bit-equality against a reference ignores the sign of a zero and treats all NaNs alike.  "left out" counts the
elements whose L1 sign is undetermined (|y'| at or below its own rounding bound); they are left out of the
dr / dxs comparison and allowed for in the partial sums' bounds.

Every output buffer was filled with a sentinel and had 64 elements of slack; the tests also require that no
sentinel is left inside an output, that the slack is untouched and that the inputs are unchanged.

Not run, checked by reading: tensors beyond 2^31 elements.  Every element offset in the kernels is formed in
`long` (`(long)blockIdx.x * 256`, `((long)g * B + r) * n + j`, `src * row_vec` with `long src`), the
theta / model index in `int` after a division by `B n` or a remainder by `n`, which fit.

Bugs found: none; no kernel was changed for these tests.

"""


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("SC_LAYER_PASS_REPORT")
    if not path or not _REPORT:
        return
    worst, left_out = {}, 0
    for kern, name, k, kind, ratio, left in _REPORT:
        left_out += left or 0
        if ratio is not None and ratio >= worst.get((kern, k), (-1.0, ""))[0]:
            worst[(kern, k)] = (ratio, name)
    lines = [_README_HEAD, f"{len(_REPORT)} checks; {left_out} elements left out in all.  Largest observed error over the "
             "derived bound, per entry point and tensor:\n", "| kernel | tensor | observed error / bound | case |", "|---|---|---|---|"]
    lines += [f"| {kern} | {k} | {r:.3f} | {name} |" for (kern, k), (r, name) in sorted(worst.items())]
    lines += ["", "Every check:", "", "| kernel | case | tensor | check | observed error / bound | left out |",
              "|---|---|---|---|---|---|"]
    for kern, name, k, kind, ratio, left in _REPORT:
        lines.append(f"| {kern} | {name} | {k} | {kind} | {'' if ratio is None else f'{ratio:.3f}'} | {left or ''} |")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


class _Out:
    """An output buffer: ``numel`` elements of sentinel plus slack."""

    def __init__(self, numel, dtype=F32):
        self.numel = numel
        self.flat = torch.full((numel + SLACK,), SENTINEL, dtype=dtype, device=DEV)

    @property
    def t(self):
        return self.flat[:self.numel]

    def cpu(self, shape, name):
        x = self.flat.cpu()
        assert bool((x[self.numel:] == SENTINEL).all()), f"{name}: written past its end"
        assert not bool((x[:self.numel] == SENTINEL).any()), f"{name}: elements left unwritten"
        return x[:self.numel].view(shape)


def _launch(case, inp):
    """Runs one case; the outputs on the CPU, after the checks no tolerance applies to."""
    from sparse_coding__amd.ops import _lib

    G, B, n, rb = case.G, case.B, case.n, case.rb
    p, lib, st = _lib.ptr, _lib.lib(), _lib.stream_handle()
    host = lp.present(case, inp)
    dv = {k: (None if v is None else v.to(DEV).contiguous()) for k, v in host.items()}
    N, s = case.numel, (G, B, n)
    on = case.on
    outs = {}

    def out(name, numel=N, dtype=F32, given=True):
        if not given:
            return None
        outs[name] = _Out(numel, dtype)
        return outs[name].t

    shapes = {}
    if case.kern == "lista_fwd":
        xo, yo = out("xo"), out("yo")
        if case.alias:  # r over a: a lives in a buffer with slack of its own
            abuf = _Out(N)
            abuf.t.copy_(dv["a"].view(-1))
            a, r_out = abuf.t, abuf.t
            outs["r"] = abuf
        else:
            a, r_out = dv["a"], out("r", given="r_out" in on)
        yob = out("yob", dtype=BF, given="yob" in on)
        absp = out("absp", N // lp.BLOCK, given="absp" in on)
        shapes = dict(xo=s, yo=s, r=s, yob=s, absp=(N // lp.BLOCK,))
        if case.entry == "sc_lista_fwd":
            rc = lib.sc_lista_fwd(p(dv["y"]), p(a), p(dv["xs"]), p(dv["theta"]), p(dv["m"]), p(xo), p(yo), G, B, n, st)
        else:
            rc = lib.sc_lista_fwd2(p(dv["y"]), p(a), p(dv["xs"]), p(dv["theta"]), p(dv["m"]), p(xo), p(yo), p(r_out),
                                   p(yob), p(absp), G, B, n, st)
    elif case.kern == "lista_bwd":
        gr, gxs = out("gr", given="gr" in on), out("gxs", given="gxs" in on)
        grb, ub = out("grb", dtype=BF, given="grb" in on), out("ub", dtype=BF, given="ub" in on)
        gth, gm = out("gth_part", G * (B // rb) * n), out("gm_part", G * (B // rb) * (n // 256))
        shapes = dict(gr=s, gxs=s, grb=s, ub=s, gth_part=(G, B // rb, n), gm_part=(G, B // rb, n // 256))
        if case.entry == "sc_lista_bwd":
            rc = lib.sc_lista_bwd(p(dv["gy"]), p(dv["gx"]), p(dv["y"]), p(dv["a"]), p(dv["xs"]), p(dv["theta"]),
                                  p(dv["m"]), p(gr), p(gxs), p(gth), p(gm), G, B, n, rb, st)
        else:
            rc = lib.sc_lista_bwd2(p(dv["gy"]), p(dv["gy2"]), p(dv["gx"]), p(dv["y"]), p(dv["a"]), p(dv["xs"]),
                                   p(dv["theta"]), p(dv["m"]), p(dv["l1c"]), p(gr), p(grb), case.gsign, p(gxs), p(ub),
                                   p(gth), p(gm), G, B, n, rb, st)
    elif case.kern == "res_fwd":
        cout = out("cout", given="cout" in on)
        hb = out("hb", dtype=BF)
        absp = out("absp", N // lp.BLOCK, given="absp" in on)
        shapes = dict(cout=s, hb=s, absp=(N // lp.BLOCK,))
        rc = lib.sc_res_fwd(p(dv["u"]), p(dv["c"]), p(dv["th"]), p(cout), p(hb), p(absp), int("fin" in on), G, B, n, st)
    else:
        o = out("out", given="out" in on)
        ob, cp = out("outb", dtype=BF), out("cpart", G * (B // rb) * n)
        shapes = dict(out=s, outb=s, cpart=(G, B // rb, n))
        rc = lib.sc_res_bwd(p(dv["gin"]), p(dv["gadd"]), p(dv["pre"]), p(dv["th"]), p(dv["l1c"]), p(o), p(ob), p(cp),
                            G, B, n, rb, st)
    _lib.check(rc, case.entry)
    torch.cuda.synchronize()
    for k, v in dv.items():  # inputs are inputs (a under an aliasing r_out was copied into its own buffer)
        assert v is None or torch.equal(v.cpu(), host[k]), f"input {k} changed"
    return {k: b.cpu(shapes[k], k) for k, b in outs.items()}


@pytest.mark.parametrize("case", lp.CASES, ids=lp._id)
def test_layer_pass(case):
    inp = lp.layer_inputs(case)
    if case.exact:
        lp.check_exact(case, inp)
    got = _launch(case, inp)
    assert set(got) == set(lp.select(case, lp.EVAL[case.kern](case, inp, F32)))
    twin = _launch(lp.twin_case(case), inp) if lp.needs_twin(case) else None
    fails, rows = lp.compare_with_twin(case, inp, got, twin)
    for k, kind, ratio, left in rows:
        print(f"{case.entry} {case.name} {k}: {kind}" + ("" if ratio is None else f", observed / bound {ratio:.3f}")
              + (f", {left} left out" if left else ""))
        _REPORT.append((case.entry, case.name, k, kind, ratio, left))
    assert not fails, "\n".join([f"{case.entry} {case.name}:"] + fails)


# ===================================================================== the autograd wrapper
@pytest.mark.parametrize("B", [12, 68])
def test_lista_step_rb4_branch_matches_autograd(B):
    """``_ListaStep`` with B % 64 != 0 (its backward's rb = 4 branch) on exact-tier inputs, r = 0 and
    |r| = theta included: the gradients of y, a, xs, theta and m equal torch autograd's on the CPU, bit for bit."""
    from sparse_coding__amd.engine.unrolled import _ListaStep, lista_step
    from sparse_coding__amd.models.lista import shrinkage

    case = lp.Case("lista_bwd", "sc_lista_bwd", "autograd", frozenset({"a", "gx", "gr", "gxs"}), 3, B, 256, 4, exact=True)
    inp = lp.layer_inputs(case)
    stats = lp.check_exact(case, inp)
    assert stats["r0"] > 0 and stats["edge"] > 0 and B % 64 != 0 and B % 4 == 0
    names = ("y", "a", "xs", "theta", "m")

    def grads(device, fn):
        leaf = [inp[k].clone().to(device).requires_grad_() for k in names]
        yo, xo = fn(*leaf)
        ((yo * inp["gy"].to(device)).sum() + (xo * inp["gx"].to(device)).sum()).backward()
        return [yo.detach().cpu(), xo.detach().cpu()] + [t.grad.cpu() for t in leaf]

    def plain(y, a, xs, theta, m):
        x_ = shrinkage(y + a, theta.unsqueeze(1))
        return x_ + m.view(-1, 1, 1) * (x_ - xs), x_

    want = grads("cpu", plain)
    got = grads(DEV, lista_step)
    assert lista_step(*[inp[k].clone().to(DEV).requires_grad_() for k in names])[0].grad_fn.name().startswith(_ListaStep.__name__)
    for k, g, w in zip(("yo", "xo") + names, got, want):
        bad = lp.canon(g) != lp.canon(w)
        assert not bool(bad.any()), f"{k}: {int(bad.sum())} of {bad.numel()} elements differ from autograd"
        _REPORT.append(("_ListaStep", f"B{B}_n256_rb4_exact", k if k in ("yo", "xo") else "d" + k,
                        "bit-equal to torch autograd (CPU)", None, 0))


# ===================================================================== centring
@pytest.mark.parametrize("shape", lp.CENTER_SHAPES, ids=str)
def test_center_rows(shape):
    from sparse_coding__amd.ops import _lib

    G, B, d = shape
    x, c = lp.center_inputs(G, B, d)
    want = lp.center_eval(x, c)
    xd, cd = x.to(DEV), c.to(DEV)
    o = _Out(G * B * d, BF)
    rc = _lib.lib().sc_center_rows(_lib.ptr(xd), _lib.ptr(cd.contiguous()), _lib.ptr(o.t), G, B, d, _lib.stream_handle())
    _lib.check(rc, "sc_center_rows")
    torch.cuda.synchronize()
    flat = o.flat.cpu()
    assert bool((flat[o.numel:] == SENTINEL).all()), "written past the end"
    got = flat[:o.numel].view(G, B, d)
    assert torch.equal(lp.bits(xd.cpu()), lp.bits(x)) and torch.equal(lp.bits(cd.cpu()), lp.bits(c))
    fails = lp.center_compare(got, want)
    _REPORT.append(("sc_center_rows", f"G{G}_B{B}_d{d}", "out", "bit-equal to the fp32 evaluation (NaN stays NaN)", None, 0))
    assert not fails, fails


# ===================================================================== gathers
def _gather_out(case):
    flat = torch.full((case.out_rows * case.row_bytes + SLACK,), SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
    dt = lp.GATHER_DTYPES[case.dtype]
    return flat, flat[:case.out_rows * case.row_bytes].view(dt).view(case.out_rows, -1)


def _gather_check(case, flat, ref, what):
    x = flat.cpu()
    nb = case.out_rows * case.row_bytes
    assert bool((x[nb:] == SENTINEL_BYTE).all()), f"{case.name} {what}: written past the end"
    got = x[:nb].view(case.out_rows, case.row_bytes)
    bad = (got != ref).any(-1)
    assert not bool(bad.any()), f"{case.name} {what}: rows {bad.nonzero().flatten().tolist()} differ"


@pytest.mark.parametrize("case", lp.GATHER_CASES, ids=lp._id)
def test_gathers(case):
    from sparse_coding__amd.ops import rows

    inp = lp.gather_inputs(case)
    dt = lp.GATHER_DTYPES[case.dtype]
    buf = inp["buf"].to(DEV).view(dt).view(case.nbuf, -1)
    flat, out = _gather_out(case)
    if case.kind == "rows":
        assert int(inp["idx"].min()) >= 0 and int(inp["idx"].max()) < case.nbuf  # (this kernel has no clamp)
        rows.gather_rows(buf, inp["idx"].to(DEV), out=out)
        torch.cuda.synchronize()
        _gather_check(case, flat, lp.gather_ref(case, inp), "gather_rows")
        fresh = rows.gather_rows(buf, inp["idx"].to(DEV))
        assert torch.equal(fresh.view(torch.uint8).cpu().view(case.rows, -1), lp.gather_ref(case, inp))
    elif case.kind == "perm":
        perm = inp["perm"].to(DEV)
        step = torch.tensor([case.step], dtype=torch.int32, device=DEV)
        ep0 = torch.tensor([case.ep0], dtype=torch.int32, device=DEV)
        for k in range(2):  # the cursor lives on the device: the second launch follows a device-side increment
            rows.gather_rows_perm(buf, perm, step, ep0, out, stride=case.stride, offset=case.offset, inner=case.inner,
                                  ostride=case.ostride)
            step.add_(1)
            flat_k = flat.clone()
            flat.fill_(SENTINEL_BYTE)
            _gather_check(case, flat_k, lp.gather_ref(case, inp, case.step + k), f"gather_rows_perm launch {k}")
        assert int(step) == case.step + 2 and int(ep0) == case.ep0
        assert torch.equal(perm.cpu(), inp["perm"])
    else:
        rows.gather_rows_blocks(buf, inp["perm"].to(DEV), case.offset, case.stride, case.inner, out)
        torch.cuda.synchronize()
        _gather_check(case, flat, lp.gather_ref(case, inp), "gather_rows_blocks")
    assert torch.equal(buf.view(torch.uint8).cpu().view(case.nbuf, -1), inp["buf"])
    n0 = lp.gather_clamped(case, inp)
    _REPORT.append((f"sc_gather_rows{'' if case.kind == 'rows' else '_' + case.kind}", case.name, "out",
                    "raw bytes equal to the index formula's" + (f" ({n0} rows clamped to row 0)" if n0 else ""), None, 0))


# ===================================================================== refusals
def _refusal(entry, what):
    """(call, outputs): a call of ``entry`` with the shape that is wrong in ``what`` and nothing else."""
    from sparse_coding__amd.ops import _lib

    p, lib, st = _lib.ptr, _lib.lib(), _lib.stream_handle()
    G, B, n, rb = 2, 8, 256, 4
    if entry in ("sc_lista_fwd", "sc_lista_fwd2", "sc_res_fwd"):
        B, n = (3, 6) if what == "n % 4" else (3, 260)
    elif entry == "sc_center_rows":
        n = 6
    else:
        n = 260 if what == "n % 256" else 256
        B, rb = {"rb < 4": (8, 2), "rb % 4": (12, 6), "B % rb": (12, 8)}.get(what, (B, rb))
    N = G * B * n
    z = lambda: torch.zeros(N + SLACK, device=DEV)  # noqa: E731
    outs = [_Out(N) for _ in range(4)] + [_Out(N, BF) for _ in range(2)]
    o = [b.t for b in outs]
    v = torch.zeros(G * n + SLACK, device=DEV)
    if entry == "sc_lista_fwd":
        return (lambda: lib.sc_lista_fwd(p(z()), p(z()), p(z()), p(v), p(v), p(o[0]), p(o[1]), G, B, n, st)), outs
    if entry == "sc_lista_fwd2":
        return (lambda: lib.sc_lista_fwd2(p(z()), p(z()), p(z()), p(v), p(v), p(o[0]), p(o[1]), p(o[2]), p(o[4]),
                                          p(o[3]) if "absp" in what else None, G, B, n, st)), outs
    if entry == "sc_res_fwd":
        fin = what == "fin without cout"
        return (lambda: lib.sc_res_fwd(p(z()), p(z()), p(v), None if fin else p(o[0]), p(o[4]),
                                       p(o[3]) if "absp" in what else None, int(fin), G, B, n, st)), outs
    if entry == "sc_lista_bwd":
        return (lambda: lib.sc_lista_bwd(p(z()), p(z()), p(z()), p(z()), p(z()), p(v), p(v), p(o[0]), p(o[1]), p(o[2]),
                                         p(o[3]), G, B, n, rb, st)), outs
    if entry == "sc_lista_bwd2":
        return (lambda: lib.sc_lista_bwd2(p(z()), p(z()), p(z()), p(z()), p(z()), p(z()), p(v), p(v), p(v), p(o[0]),
                                          p(o[4]), -1.0, p(o[1]), p(o[5]), p(o[2]), p(o[3]), G, B, n, rb, st)), outs
    if entry == "sc_res_bwd":
        return (lambda: lib.sc_res_bwd(p(z()), p(z()), p(z()), p(v), None, p(o[0]), p(o[4]), p(o[1]), G, B, n, rb, st)), outs
    if entry == "sc_center_rows":
        return (lambda: lib.sc_center_rows(p(z().to(BF)), p(v), p(o[4]), G, B, n, st)), outs
    buf = torch.zeros(16, 64, device=DEV)
    idx = torch.zeros(64, dtype=torch.int64, device=DEV)
    i32 = torch.zeros(1, dtype=torch.int32, device=DEV)
    rb_ = 24 if what == "row_bytes % 16" else 32
    if entry == "sc_gather_rows":
        return (lambda: lib.sc_gather_rows(p(buf), p(idx), p(o[0]), 8, rb_, st)), outs
    if entry == "sc_gather_rows_blocks":
        return (lambda: lib.sc_gather_rows_blocks(p(buf), 16, p(idx), 64, 0, 4, 4, 2, p(o[0]), rb_, st)), outs
    rows_, stride, offset, inner = {"stride < inner": (8, 2, 0, 4), "offset < 0": (8, 8, -1, 4),
                                    "rows % inner": (6, 8, 0, 4)}.get(what, (8, 8, 0, 4))
    return (lambda: lib.sc_gather_rows_perm(p(buf), 16, p(idx), 64, p(i32), p(i32), p(o[0]), rows_, rb_, stride, offset,
                                            inner, inner, st)), outs


@pytest.mark.parametrize("entry,what", lp.REFUSALS, ids=lambda x: x.replace(" ", "_"))
def test_rejected_shapes_raise_and_write_nothing(entry, what):
    from sparse_coding__amd.ops import _lib

    call, outs = _refusal(entry, what)
    with pytest.raises(_lib.KernelError, match=entry):
        _lib.check(call(), entry)
    torch.cuda.synchronize()
    for b in outs:
        assert bool((b.flat == SENTINEL).all()), f"{entry} ({what}) wrote an output"
    _REPORT.append((entry, what.replace("%", "mod").replace("<", "below"), "-", "KernelError, outputs keep the sentinel", None, 0))


def test_gather_wrappers_refuse_rows_that_are_no_16_byte_multiple():
    from sparse_coding__amd.ops import rows

    buf = torch.zeros(4, 6, device=DEV)  # 24-byte rows
    idx = torch.zeros(2, dtype=torch.int64, device=DEV)
    i32 = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.full((2, 6), SENTINEL, device=DEV)
    with pytest.raises(ValueError, match="16"):
        rows.gather_rows(buf, idx, out=out)
    with pytest.raises(ValueError, match="16"):
        rows.gather_rows_perm(buf, idx, i32, i32, out)
    with pytest.raises(ValueError):
        rows.gather_rows_blocks(buf, idx, 0, 2, 2, out)
    assert bool((out == SENTINEL).all())
