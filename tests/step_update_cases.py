"""Cases, input recipes, fp64 references, the fp32 "plain evaluation", the comparator and the planted errors
for the end-of-step update (``ops/csrc/adam.hip``, ``row_adam.h``): row Adam with the norm Jacobian, the bf16
shadow and row norms, bias Adam, the loss terms and the top-k tail's MSE.  ``test_step_update_cpu.py`` checks
all of this without a GPU, ``test_step_update_gpu.py`` compares the kernels with it.

Every formula is written once (``row_eval`` / ``bias_eval`` / ``mse_eval``) from the reference's definition,
not from the kernel, and evaluated in two number formats: fp64 is the reference, fp32 -- one torch operation
per step, every sum accumulated left to right -- the plain evaluation.  ``E32[tensor] = max |plain32 - ref64|``
is what fp32 costs an honest evaluation of the formula on these inputs; a kernel passes where
``|kernel - ref64| <= MARGIN * E32`` elementwise (its reduction tree and its written-out multiply-adds round
in another order, under the same first-order bound).  Nothing here is measured on a kernel.  On a tensor of
two or three values (a loss term per model, the top-k MSE) the plain evaluation can be right to a few
hundredths of an ulp by luck; the bound then admits only the fp32 value nearest the reference, which a kernel
that accumulates in fp64 and rounds once delivers (``loss_terms`` / ``tail_mse`` do; their fp32 forms were
1-2 ulp off and missed it in three cases).

Rows whose norm is at or below the 1e-8 floor take ``g * 1e8`` and get moments of 1e6 .. 1e13: they are
bounded relative to the reference value (``E32[name + "_rel"]``), derived the same way.

Device step counter: the kernel's ``__powf`` may miss ``1 - beta^t`` by ``DELTA_BC`` = 2^-21 absolute (one
ulp of a result near 1, plus the propagated error of the exponent: |x| 2^-x <= 0.54); propagated into the
update that is ``|dp_ref| (DELTA_BC / bc1 + DELTA_BC / (2 bc2))`` (``bc_allowance``), added to the bound.

Exact tier: ``b1 = b2 = 0.5``, even-integer g / m / v below 2^12, ``norm=False`` rows and ``norm=True`` rows
``2^k e_j`` -- norm, inverse, dot product and projection are exact powers of two there and the projected
gradient at j is exactly 0 -- so the new moments are exact in fp32 in any order (``check_exact``).
"""

from __future__ import annotations

import re
import zlib
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Tuple

import numpy as np
import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
HIP_SOURCE = Path(__file__).resolve().parent.parent / "sparse_coding__amd" / "ops" / "csrc" / "adam.hip"

MARGIN = 4.0
DELTA_BC = 2.0 ** -21
STEPS = (1, 2, 10, 1000)


def f32(x) -> float:
    """The fp32 value the kernel receives for the host double ``x``."""
    return float(np.float32(x))


B1, B2, EPS, FLOOR = f32(0.9), f32(0.999), f32(1e-8), f32(1e-8)
INV_FLOOR = 1e8  # exact in fp32


def parsed_widths():
    """The instantiated row widths of ``sc_adam_rows`` and of the step tails, from the SC_ADAM(..) /
    SC_TAIL(..) lists of adam.hip."""
    src = HIP_SOURCE.read_text()
    out = {}
    for name in ("SC_ADAM", "SC_TAIL"):
        body = src.split(f"#define {name}(NVV)")[1].split(f"#undef {name}")[0]
        sw = body[body.index("switch"):]
        out[name] = tuple(sorted(256 * int(v) for v in re.findall(rf"{name}\((\d+)\)", sw)))
    return out


def _gen(*seed):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(seed).encode()))
    return g


def seqsum(x, dim):
    """Left-to-right sum in x's own format (the plain evaluation's reduction; any order in fp64)."""
    return torch.cumsum(x, dim=dim).select(dim, -1)


def _s(x, dtype):
    return torch.tensor(x, dtype=dtype)


def bias_corr(b1, b2, t, dtype):
    return 1 - _s(b1, dtype) ** t, 1 - _s(b2, dtype) ** t


# ===================================================================== row Adam
@dataclass(frozen=True)
class RowCase:
    name: str
    d: int
    G: int = 3
    n: int = 10                       # rows per model
    norm: Tuple[bool, ...] = (True,)  # one flag per parameter set
    gbf16: bool = False
    nsplit: int = 1
    t: int = 5
    device_step: bool = False
    row0: int = 0
    rows: Optional[int] = None        # a [rows, d] shard (default: the whole [G, n, d] stack)
    live: Optional[Tuple[int, ...]] = None
    special: bool = False             # row 1 zero, row 2 with zero g / m / v, row 3 of norm ~1e-9
    exact: bool = False
    b1: float = B1
    b2: float = B2
    policy: Optional[int] = None

    @property
    def R(self):
        return self.rows if self.rows is not None else self.G * self.n


WIDTHS = (256, 512, 768, 1024, 1536, 2048, 4096)

ROW_CASES = (
    [RowCase(f"d{d}", d, norm=(True, False), special=True, t=STEPS[i % 4], device_step=bool(i % 2))
     for i, d in enumerate(WIDTHS)]
    + [RowCase(f"d{d}_bf16_split3", d, gbf16=True, nsplit=3, norm=(False, True), t=STEPS[(i + 1) % 4],
               device_step=not i % 2) for i, d in enumerate(WIDTHS)]
    + [RowCase(f"t{t}_{'dev' if dev else 'host'}", 512, t=t, device_step=dev, special=True)
       for t in STEPS for dev in (False, True)]
    + [RowCase("nonorm_split3", 256, norm=(False,), nsplit=3, t=2),
       RowCase("bf16_one_set", 768, gbf16=True, norm=(True,), special=True, t=10),
       RowCase("shard_row0_7", 512, row0=7, rows=19, norm=(True, False), t=2),
       RowCase("shard_row0_7_dev", 256, row0=7, rows=19, nsplit=3, device_step=True, t=10),
       RowCase("live_10_3_0", 512, live=(10, 3, 0), norm=(True, False), t=2, device_step=True),
       RowCase("vector_rpm1", 256, G=5, n=1, norm=(False,), device_step=True, t=1),
       RowCase("vector_rpm1_1536", 1536, G=3, n=1, norm=(False,), t=1000)]
    + [RowCase(f"policy{p}", 1024, norm=(True, False), special=True, t=2, policy=p) for p in range(4)]
)
EXACT_ROW_CASES = [RowCase(f"exact_d{d}", d, norm=(True, False), nsplit=1 + 2 * (i % 2), exact=True, b1=0.5,
                           b2=0.5, t=1 + i, device_step=False) for i, d in enumerate(WIDTHS)]
ALL_ROW_CASES = ROW_CASES + EXACT_ROW_CASES


def row_inputs(case: RowCase, state=None):
    """The fp32 (bf16 gradient: bf16) tensors the kernel receives.  Per set: p, m, v [R, d], g
    [nsplit, R, d] (slabs); lr [G].  ``state``: per set {p, m, v} to take instead of the recipe's (the step
    before of a multi-step test); the gradient is then drawn around that p."""
    R, d, ns = case.R, case.d, case.nsplit
    gen = _gen("row", case.name)
    lr = torch.tensor([0.1 + 0.4 * ((3 * i + 1) % 7) / 7 for i in range(case.G)], dtype=F32)
    sets = []
    for s, norm in enumerate(case.norm):
        if case.exact:
            ev = lambda lo, hi, *shape: 2.0 * torch.randint(lo, hi, shape, generator=gen).float()  # noqa: E731
            g = ev(-340, 341, ns, R, d)  # |sum of 3 slabs| <= 2040 < 2^12
            m, v = ev(-2047, 2048, R, d), ev(0, 2048, R, d)
            if norm:
                p = torch.zeros(R, d)
                j = torch.randint(0, d, (R,), generator=gen)
                j[0], j[1] = 0, d - 1
                p[torch.arange(R), j] = 2.0 ** (torch.arange(R) % 4).float() * (1 - 2 * (torch.arange(R) % 2)).float()
            else:
                p = torch.randn(R, d, generator=gen)
            sets.append(dict(p=p, g=g, m=m, v=v, norm=norm))
            continue
        p = torch.randn(R, d, generator=gen) / d ** 0.5 * (0.5 + 1.5 * torch.rand(R, 1, generator=gen))
        if state is not None:
            p = state[s]["p"].clone()
        if case.special:
            p[1] = 0.0
            p[3] *= 1e-9 / max(1.0, float(p[3].norm()))
        w_hat = p / p.norm(dim=-1, keepdim=True).clamp_min(1e-8)
        # g = 0.03 w_hat + 0.1 noise with every 7th column scaled by 1e-8 (columns where eps matters), the
        # noise made orthogonal to w_hat: <w_hat, g> is then 0.03 x 6/7 in every row.  Left to chance it is
        # near 0 in some row, and there the projected gradient of the 7th columns -- w_hat_j <w_hat, g> / |w|,
        # divided by eps in the update -- is rounding noise of the dot product's summation order alone.
        seventh = torch.zeros(d, dtype=torch.bool)
        seventh[::7] = True
        noise = 0.1 * torch.randn(R, d, generator=gen)
        noise[:, seventh] *= 1e-8
        w_rest = w_hat * ~seventh
        noise -= w_rest * ((w_hat * noise).sum(-1, keepdim=True) / (w_hat * w_rest).sum(-1, keepdim=True).clamp_min(1e-30))
        g = noise + 0.03 * w_rest
        m = 0.1 * torch.randn(R, d, generator=gen)
        v = 1e-2 * torch.rand(R, d, generator=gen)
        m[:, seventh] *= 1e-8
        v[:, seventh] = 1e-17
        if state is not None:
            m, v = state[s]["m"].clone(), state[s]["v"].clone()
        if case.special:
            g[2], m[2], v[2] = 0.0, 0.0, 0.0
        slabs = [0.05 * torch.randn(R, d, generator=gen) for _ in range(ns - 1)]
        for sl in slabs:
            sl[:, seventh] *= 1e-8  # (a sum that cancels to 1e-9 from 0.05 would be rounding noise too)
            sl -= w_rest * ((w_hat * sl).sum(-1, keepdim=True) / (w_hat * w_rest).sum(-1, keepdim=True).clamp_min(1e-30))
            if case.special:
                sl[2] = 0.0
        g = torch.stack([g - sum(slabs)] + slabs) if slabs else g[None]
        if case.gbf16:
            g = g.to(BF)
        sets.append(dict(p=p, g=g.contiguous(), m=m, v=v, norm=norm))
    return dict(sets=sets, lr=lr)


def row_models(case: RowCase, mut=None):
    """Model index of every row (the lr index)."""
    r = torch.arange(case.R)
    idx = (r if mut == "row0_ignored" else r + case.row0) // case.n
    if mut == "lr_neighbour":
        idx = (idx + 1) % case.G
    return idx.clamp(max=case.G - 1) if mut == "row0_ignored" else idx


def row_active(case: RowCase):
    """Rows the update touches (all, or those below their model's live count)."""
    r = torch.arange(case.R) + case.row0
    if case.live is None:
        return torch.ones(case.R, dtype=torch.bool)
    return (r % case.n) < torch.tensor(case.live)[r // case.n]


ROW_MUTATIONS = ("no_projection", "eps_in_sqrt", "bc_swapped", "t_off_by_one", "lr_neighbour", "row0_ignored",
                 "slab2_dropped", "floor_rows_zero_grad", "shadow_of_old_p")


def row_reachable(case: RowCase, mut):
    # (eps only matters beside v ~ eps^2: the exact tier's integer moments are far from it)
    return {"no_projection": any(case.norm), "eps_in_sqrt": not case.exact, "bc_swapped": case.b1 != case.b2, "lr_neighbour": case.G > 1,
            "row0_ignored": case.row0 % case.n != 0 or case.row0 >= case.n, "slab2_dropped": case.nsplit > 1,
            "floor_rows_zero_grad": case.special and any(case.norm)}.get(mut, True)


def row_eval(case: RowCase, inp, dtype, mut=None):
    """The row update of every set in ``dtype``: {p, m, v, norms, sv (the shadow's value before its bf16
    rounding), dp (the update), floor (rows at or below the norm floor)} + the set index.  Rows that are not
    live keep p / m / v; their norms / sv entries are meaningless."""
    t = case.t + (mut == "t_off_by_one")
    bc1, bc2 = bias_corr(case.b1, case.b2, t, dtype)
    if mut == "bc_swapped":
        bc1, bc2 = bc2, bc1
    b1, b2, eps = _s(case.b1, dtype), _s(case.b2, dtype), _s(EPS, dtype)
    floor = _s(FLOOR, dtype)
    lr = inp["lr"].to(dtype)[row_models(case, mut)][:, None]
    act = row_active(case)[:, None]
    out = {}
    for s, st in enumerate(inp["sets"]):
        p, m, v = (st[k].to(dtype) for k in ("p", "m", "v"))
        slabs = st["g"].to(dtype)
        if mut == "slab2_dropped":
            slabs = torch.cat([slabs[:1], slabs[2:]])
        g = seqsum(slabs, 0)
        small = torch.zeros(case.R, dtype=torch.bool)
        if st["norm"]:
            nrm = seqsum(p * p, -1).sqrt()[:, None]
            small = (nrm <= floor)[:, 0]
            w_hat = p / torch.maximum(nrm, floor)
            proj = 0 if mut == "no_projection" else w_hat * seqsum(w_hat * g, -1)[:, None]
            g_floor = torch.zeros_like(g) if mut == "floor_rows_zero_grad" else g * INV_FLOOR
            g = torch.where(small[:, None], g_floor, (g - proj) / torch.where(small[:, None], torch.ones_like(nrm), nrm))
        m_new = b1 * m + (1 - b1) * g
        v_new = b2 * v + (1 - b2) * g * g
        den = (v_new / bc2 + eps).sqrt() if mut == "eps_in_sqrt" else (v_new / bc2).sqrt() + eps
        dp = lr * (m_new / bc1) / den
        p_new = p - dp
        src = p if mut == "shadow_of_old_p" else p_new
        if st["norm"]:
            nn = torch.maximum(seqsum(src * src, -1).sqrt(), floor)
            sv = src / nn[:, None]
        else:
            nn, sv = torch.zeros(case.R, dtype=dtype), src
        out.update({f"p{s}": torch.where(act, p_new, p), f"m{s}": torch.where(act, m_new, m),
                    f"v{s}": torch.where(act, v_new, v), f"norms{s}": nn, f"sv{s}": sv,
                    f"dp{s}": torch.where(act, dp, torch.zeros_like(dp)), f"floor{s}": small & act[:, 0]})
    return out


def check_exact(case: RowCase, inp):
    """The conditions under which m_new / v_new are exact in fp32 whatever the order of operations."""
    assert case.exact and case.b1 == 0.5 and case.b2 == 0.5 and not case.gbf16 and case.live is None
    for st in inp["sets"]:
        for k in ("g", "m", "v"):
            x = st[k].double()
            assert bool((x == 2 * (x / 2).round()).all()) and float(x.abs().max()) < 4096, k
        assert float(st["g"].double().sum(0).abs().max()) < 4096 and float(st["v"].min()) >= 0
        if st["norm"]:
            p = st["p"].double()
            assert bool(((p != 0).sum(-1) == 1).all())
            k = torch.log2(p.abs().max(-1).values)
            assert bool((k == k.round()).all()) and float(k.min()) >= 0 and float(k.max()) <= 3
    ref = row_eval(case, inp, F64)
    for s, st in enumerate(inp["sets"]):
        for k in ("m", "v"):
            x = ref[f"{k}{s}"]
            assert torch.equal(x.float().double(), x), f"{k}{s} is not representable in fp32"
        if st["norm"]:  # the projected gradient at the row's own column is exactly 0: m_new = m / 2 there
            j = st["p"].abs().argmax(-1)
            r = torch.arange(case.R)
            assert torch.equal(ref[f"m{s}"][r, j], st["m"].double()[r, j] / 2)


# ===================================================================== comparator
def bf16_half_ulp(x):
    """Half a bf16 ulp at the fp64 values x (bf16: 8 significant bits, fp32's exponent range)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 8)


def e32_of(plain, ref, floor_rows=None):
    """E32 per tensor from the plain evaluation and the reference.  ``floor_rows``: {tensor name: bool row
    mask} of rows bounded relatively (``name_rel``) instead."""
    out = {}
    for k, r in ref.items():
        if not r.dtype.is_floating_point:
            continue
        err = (plain[k].double() - r).abs()
        mask = (floor_rows or {}).get(k)
        if mask is not None and bool(mask.any()):
            out[k + "_rel"] = float((err[mask] / r[mask].abs().clamp_min(1e-300)).max())
            err = err[~mask]
        out[k] = float(err.max()) if err.numel() else 0.0
    return out


def compare(got, ref, e32, extra=None, floor_rows=None, exact=(), margin=MARGIN):
    """Failures (strings) of ``got`` against the fp64 ``ref``: elementwise |got - ref| <= margin E32[k]
    (+ ``extra[k]``, a derived elementwise allowance); ``sv*`` tensors as bf16 shadows (half a bf16 ulp of the
    reference value more); names in ``exact``: bitwise equal to the reference cast to fp32.  Also returns the
    observed error per tensor (``sv*``: the largest |got - ref| / bound)."""
    fails, seen = [], {}
    for k, r in ref.items():
        if k not in got or not r.dtype.is_floating_point:
            continue
        x = got[k].double()
        if k in exact:
            seen[k] = float((x - r).abs().max())
            if not torch.equal(got[k].float(), r.float()):
                fails.append(f"{k}: not bit-equal to the reference ({int((got[k].float() != r.float()).sum())} elements)")
            continue
        err = (x - r).abs()
        bound = torch.full_like(r, margin * e32[k])
        mask = (floor_rows or {}).get(k)
        if mask is not None and bool(mask.any()):
            bound[mask] = margin * e32[k + "_rel"] * r[mask].abs()
        if extra and k in extra:
            bound = bound + extra[k]
        if k.startswith("sv"):
            bound = bound + bf16_half_ulp(r)
        bad = ~(err <= bound)  # (NaN fails)
        seen[k] = float(err[~mask].max()) if mask is not None and bool((~mask).any()) else float(err.max())
        if k.startswith("sv"):  # (the error of a bf16 value says little: the largest share of its bound)
            seen[k] = float((err / bound).max())
        if bool(bad.any()):
            i = int((err - bound).masked_fill(~bad, -1).argmax()) if not bool(torch.isnan(err).any()) else int(bad.flatten().nonzero()[0])
            fails.append(f"{k}: {int(bad.sum())} of {bad.numel()} elements beyond the bound; worst at flat index {i}: "
                         f"|got - ref| = {float(err.flatten()[i]):.3e} > {float(bound.flatten()[i]):.3e} "
                         f"(E32 = {e32[k]:.3e}, ref = {float(r.flatten()[i]):.6e})")
    return fails, seen


def bc_allowance(dp, b1, b2, t):
    """What a bias correction off by DELTA_BC may move the update ``dp`` by (device step counter)."""
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    return dp.abs() * (DELTA_BC / bc1 + DELTA_BC / (2 * bc2))


def row_check_parts(case: RowCase, inp):
    """(ref64, E32, floor_rows, extra) of a row case: what ``compare`` needs besides the kernel's output."""
    ref, plain = row_eval(case, inp, F64), row_eval(case, inp, F32)
    floor_rows, extra = {}, {}
    for s in range(len(case.norm)):
        for k in ("p", "m", "v"):
            floor_rows[f"{k}{s}"] = ref[f"floor{s}"]
        if case.device_step:
            extra[f"p{s}"] = bc_allowance(ref[f"dp{s}"], case.b1, case.b2, case.t)
            if case.norm[s]:
                # d(w / |w|) = (dw - w_hat <w_hat, dw>) / |w|: per element at most (|dw|_inf + |dw|_2) / |w|,
                # and the norm itself moves by at most |dw|_2
                l2 = extra[f"p{s}"].square().sum(-1).sqrt()
                extra[f"sv{s}"] = ((extra[f"p{s}"].amax(-1) + l2) / ref[f"norms{s}"])[:, None] \
                    * torch.ones_like(ref[f"sv{s}"])
                extra[f"norms{s}"] = l2
            else:
                extra[f"sv{s}"] = extra[f"p{s}"]
    ref = {k: v for k, v in ref.items() if not k.startswith(("dp", "floor"))}
    return ref, e32_of(plain, ref, floor_rows), floor_rows, extra


def row_exact_names(case: RowCase):
    return tuple(f"{k}{s}" for s in range(len(case.norm)) for k in ("m", "v")) if case.exact else ()


# ===================================================================== bias Adam + loss terms
@dataclass(frozen=True)
class BiasCase:
    name: str
    n: int
    G: int = 3
    tm: int = 3
    cnt_tm: Optional[int] = None      # slots of cnt_part (default tm)
    enc_tiles: int = 1
    dec_tiles: int = 1
    beta: Tuple[float, ...] = (0.1, 0.0, 0.1)
    zero_model: Optional[int] = 2     # b == 0 there (with beta > 0: no NaN)
    t: int = 5
    device_step: bool = False
    B: int = 384
    d: int = 256
    counting: bool = True

    @property
    def ctm(self):
        return self.cnt_tm or self.tm


BIAS_CASES = [
    BiasCase("n32", 32, tm=1, enc_tiles=1, dec_tiles=255, t=1),
    BiasCase("n96_dev", 96, tm=8, enc_tiles=255, dec_tiles=256, t=2, device_step=True),
    BiasCase("n36", 36, tm=13, enc_tiles=256, dec_tiles=600, t=10),
    BiasCase("n33_dev", 33, tm=3, enc_tiles=600, dec_tiles=1, t=1000, device_step=True),
    BiasCase("n33_tm13_dev", 33, tm=13, enc_tiles=3, dec_tiles=5, t=1, device_step=True),
    BiasCase("reduced_grad_cnt5", 96, tm=1, cnt_tm=5, enc_tiles=5, dec_tiles=5, t=10, device_step=True),
    BiasCase("cnt13_tm9", 64, tm=9, cnt_tm=13, enc_tiles=2, dec_tiles=2, t=1000),
    BiasCase("no_counts", 36, tm=8, counting=False, t=2, beta=(0.0, 0.1, 0.1), zero_model=0),
    BiasCase("n65568", 65568, G=2, tm=5, beta=(0.1, 0.0), zero_model=None, t=2, device_step=True),
]
BIAS_MUTATIONS = ("bnorm_post_update", "gscale_on_decay", "tiles_ge8_dropped", "cnt_tm_as_tm", "l1_over_Bd",
                  "bc_swapped", "t_off_by_one")


def bias_reachable(case: BiasCase, mut):
    decays = any(b > 0 and g != case.zero_model for g, b in enumerate(case.beta))
    return {"bnorm_post_update": decays, "gscale_on_decay": decays, "tiles_ge8_dropped": case.tm > 8,
            "cnt_tm_as_tm": case.counting and case.ctm > case.tm}.get(mut, True)


def bias_inputs(case: BiasCase, salt=0):
    G, n = case.G, case.n
    gen = _gen("bias", case.name, salt)
    b = 0.1 * torch.randn(G, n, generator=gen)
    if case.zero_model is not None:
        b[case.zero_model] = 0.0
    m = 0.1 * torch.randn(G, n, generator=gen)
    v = 1e-2 * torch.rand(G, n, generator=gen)
    colpart = torch.randn(G, case.tm, n, generator=gen)
    colpart[:, :, ::7] *= 1e-8
    m[:, ::7] *= 1e-8
    v[:, ::7] = 1e-17
    b[:, ::7] *= 1e-8
    return dict(
        b=b, m=m, v=v, colpart=colpart, gscale=f32(0.05),
        cnt_part=torch.randint(0, 129, (G, case.ctm, n), generator=gen).float(),
        feat_count=torch.randint(0, 1000, (G, n), generator=gen).float(),
        enc_part=torch.stack([torch.rand(G, case.enc_tiles, generator=gen) * 50,
                              torch.randint(0, 4000, (G, case.enc_tiles), generator=gen).float()], -1).contiguous(),
        dec_part=torch.rand(G, case.dec_tiles, generator=gen) * 1e3,
        l1=torch.tensor([1e-3 * (g + 1) for g in range(G)], dtype=F32),
        bias_decay=torch.tensor(case.beta, dtype=F32),
        lr=torch.tensor([0.1 + 0.4 * ((3 * i + 2) % 7) / 7 for i in range(G)], dtype=F32))


def bias_eval(case: BiasCase, inp, dtype, mut=None, t=None):
    """{b, m, v, count, out0..out5, dp} in ``dtype``; ``t``: the 1-based Adam step (default the case's)."""
    t = (case.t if t is None else t) + (mut == "t_off_by_one")
    bc1, bc2 = bias_corr(B1, B2, t, dtype)
    if mut == "bc_swapped":
        bc1, bc2 = bc2, bc1
    b1, b2, eps = _s(B1, dtype), _s(B2, dtype), _s(EPS, dtype)
    b, m, v = (inp[k].to(dtype) for k in ("b", "m", "v"))
    beta, lr = inp["bias_decay"].to(dtype)[:, None], inp["lr"].to(dtype)[:, None]
    gscale = _s(inp["gscale"], dtype)
    colsum = seqsum(inp["colpart"].to(dtype)[:, :8] if mut == "tiles_ge8_dropped" else inp["colpart"].to(dtype), 1)

    def update(bnorm):
        bd = torch.where((beta != 0) & (bnorm > 0), beta / torch.where(bnorm > 0, bnorm, torch.ones_like(bnorm)),
                         torch.zeros_like(bnorm))
        g = gscale * (colsum + bd * b) if mut == "gscale_on_decay" else gscale * colsum + bd * b
        m_new = b1 * m + (1 - b1) * g
        v_new = b2 * v + (1 - b2) * g * g
        dp = lr * (m_new / bc1) / ((v_new / bc2).sqrt() + eps)
        return m_new, v_new, dp

    bnorm = seqsum(b * b, -1).sqrt()[:, None]
    m_new, v_new, dp = update(bnorm)
    if mut == "bnorm_post_update":
        b_post = b - dp
        m_new, v_new, dp = update(seqsum(b_post * b_post, -1).sqrt()[:, None])
    out = dict(b=b - dp, m=m_new, v=v_new, dp=dp)
    if case.counting:
        cnt = inp["cnt_part"].to(dtype)
        out["count"] = inp["feat_count"].to(dtype) + seqsum(cnt[:, :case.tm] if mut == "cnt_tm_as_tm" else cnt, 1)
    enc, dec = inp["enc_part"].to(dtype), inp["dec_part"].to(dtype)
    Bf, Bd = _s(float(case.B), dtype), _s(float(case.B), dtype) * _s(float(case.d), dtype)
    l_rec = seqsum(dec, 1) / Bd
    l_l1 = inp["l1"].to(dtype) * seqsum(enc[..., 0], 1) / (Bd if mut == "l1_over_Bd" else Bf)
    l_bd = beta[:, 0] * bnorm[:, 0]
    for i, x in enumerate((l_rec + l_l1 + l_bd, l_rec, l_l1, l_bd, seqsum(enc[..., 1], 1) / Bf, bnorm[:, 0])):
        out[f"out{i}"] = x
    return out


def bias_check_parts(case: BiasCase, inp, t=None, device_step=None):
    ref, plain = bias_eval(case, inp, F64, t=t), bias_eval(case, inp, F32, t=t)
    extra = {}
    if case.device_step if device_step is None else device_step:
        extra["b"] = bc_allowance(ref["dp"], B1, B2, case.t if t is None else t)
    ref.pop("dp")
    return ref, e32_of(plain, ref), extra


# ===================================================================== top-k tail MSE
def mse_eval(row_se, se_scale, dtype):
    return {"mse": seqsum(row_se.to(dtype), 1) * _s(se_scale, dtype)}


def mse_check_parts(row_se, se_scale):
    ref = mse_eval(row_se, se_scale, F64)
    return ref, e32_of(mse_eval(row_se, se_scale, F32), ref)


def gather_reference(buf, perm, t, ep0, rows):
    """out[r] = buf[perm[(t + 1 - ep0) * rows + r]] (t: completed steps before this tail)."""
    return buf[perm[(t + 1 - ep0) * rows + torch.arange(rows)]]


# ===================================================================== shadow_rows inputs
SHADOW_ROWS, SHADOW_D = (1, 5), (4, 100, 256, 260, 768)


def shadow_inputs(rows, d, special: bool):
    """fp32 rows; ``special`` (the un-normalised copy): exact round-to-even ties, negative zero, fp32
    denormals and the bf16 overflow edge in the first columns."""
    p = torch.randn(rows, d, generator=_gen("shadow", rows, d))
    if special:
        edge = torch.tensor([0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000 - (1 << 32)],
                            dtype=torch.int32).view(F32)  # bf16 max, just below / at / above its rounding edge
        vals = torch.cat([torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -0.0, 0.0, 1e-40, -1e-45,
                                        2.0 ** -126, 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -24]), edge])
        flat = p.view(-1)
        k = min(vals.numel(), flat.numel())
        flat[:k] = vals[:k]
        if flat.numel() >= 2 * vals.numel():
            flat[-vals.numel():] = vals
    elif rows > 1:
        p[1] = 0.0  # a zero row: the floor of the norm
    return p


def shadow_eval(p, dtype):
    x = p.to(dtype)
    nrm = torch.maximum(seqsum(x * x, -1).sqrt(), _s(FLOOR, dtype))
    return {"norms": nrm, "sv": x / nrm[:, None]}
