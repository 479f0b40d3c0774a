"""Cases, input recipes, fp64 references, the dispatch mirror and the planted errors for the persistent FISTA
solvers (``ops/csrc/fista.hip``: ``fista_kernel`` / ``fista_gram_kernel`` behind ``sc_fista``, ``sc_coef_search``
and ``sc_fista_gram``).  ``test_fista_exact_cpu.py`` checks all of this without a GPU, ``test_fista_exact_gpu.py``
compares the kernels with it by ``torch.equal``.

Exact tier.  Dictionaries with four entries from {+-1, +-1/2} per atom, integer X in [-6, 6], a 5 %-dense
integer warm start, power-of-two ``eta`` and ``eta lam`` per model and a dyadic momentum table: for T <= 3 every
value the kernels form -- the product sums whatever their order or FMA contraction, and every fp32 elementwise
step -- is exactly representable, while the bf16 rounding of the iterate and of the residual stays non-trivial
(it is applied here exactly where the kernels apply it, round to nearest even).  ``check_exact`` proves that
per case from the inputs alone: for every product-sum the sum of the absolute values of its terms over the
smallest unit among the operands of its row stays below 2^24 (so every partial sum in any order is an fp32
value), and every elementwise intermediate equals its own fp32 rounding.

The recurrences are written from the solver's definition (reference ``autoencoders/fista.py:99-128``, the
coefficient search ``direct_coef_search.py:52-56`` and the adjoint of the unrolled loop), with the tile
geometry (column passes, row tiles, 16-column tiles, k-steps of 32) entering only through the planted errors."""

from __future__ import annotations

import re
import zlib
from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
HIP_SOURCE = Path(__file__).resolve().parent.parent / "sparse_coding__amd" / "ops" / "csrc" / "fista.hip"

# ===================================================================== dispatch mirror
# (d / 128, n / 128) of the direct solver: 16-row workgroups, and those that also have 32-row workgroups;
# every tile in modes 0 (solve), 1 (coefficient search), 2 (slab-saving)
DIRECT_RT1 = ((2, 2), (2, 4), (2, 8), (2, 16), (4, 4), (4, 8), (4, 16), (6, 6), (6, 12), (8, 4), (8, 8), (8, 16))
DIRECT_RT2 = ((2, 2), (2, 4), (4, 4), (8, 4))
DIRECT_MODES = (0, 1, 2)
# Gram solver: NW = n / 128 -> mode -> rows per workgroup / 16 -> (HALVES, PF), None where not instantiated
GRAM_TABLE = {
    2: {0: {2: (1, 4), 1: (1, 4)}, 1: {2: (1, 4), 1: (1, 4)}, 2: {2: (1, 4), 1: (1, 4)}},
    4: {0: {2: (1, 4), 1: (1, 8)}, 1: {2: (1, 4), 1: (1, 4)}, 2: {2: (4, 1), 1: (1, 2)}},
    6: {0: {2: (2, 2), 1: (2, 4)}, 1: {2: (2, 2), 1: (2, 4)}, 2: {2: None, 1: (3, 1)}},
    8: {0: {2: (4, 2), 1: (2, 4)}, 1: {2: None, 1: (2, 4)}, 2: {2: None, 1: (8, 1)}},
}
LDS_LIMIT = 160 * 1024
REFUSED = 2


def dispatch(form, d, n, mode, G, B, rows):
    """The instantiation a call launches: direct ``(DW, NW, RT, MODE, PH)``, Gram ``(NW, RT, HALVES, PF,
    MODE)``; ``REFUSED`` where the launcher returns 2 (shape not instantiated).  ``rows``: 0, 16 or 32."""
    if form == "direct":
        DW, NW = d // 128, n // 128
        rows = 0 if mode == 1 else rows  # sc_coef_search has no rows argument: the heuristic alone
        lds1 = 16 * (2 * n + 4 * d)
        rt2 = (rows != 16 and B % 32 == 0 and 2 * lds1 <= LDS_LIMIT and (rows == 32 or G * (B // 32) >= 256))
        ph = (4 if DW >= 4 else 2) if NW >= 16 else 1
        if d % 128 or n % 128 or lds1 > LDS_LIMIT:
            return REFUSED
        if rt2 and (DW, NW) in DIRECT_RT2:
            return (DW, NW, 2, mode, ph)
        return (DW, NW, 1, mode, ph) if (DW, NW) in DIRECT_RT1 else REFUSED
    NW = n // 128
    if n % 128 or NW not in GRAM_TABLE:
        return REFUSED
    two = B % 32 == 0 and rows != 16 and (rows == 32 or G * (B // 32) >= 512)
    by_rt = GRAM_TABLE[NW][mode]
    rt = 2 if (two and by_rt[2] is not None) else 1
    return (NW, rt) + by_rt[rt] + (mode,)


def parsed_tables():
    """The launch tables of fista.hip: ({(DW, NW, RT, MODE)} of the direct solver, the Gram table in the
    layout of ``GRAM_TABLE``)."""
    src = HIP_SOURCE.read_text()
    direct = set()
    for macro in ("SC_F2", "SC_F"):
        body = src.split(f"#define {macro}(DWV, NWV)")[1].split("#define" if macro == "SC_F" else "\n  SC_F2(")[0]
        kinds = [(int(rt), int(m)) for rt, m in re.findall(r"SC_FK\(DWV, NWV, (\d), (\d), lds\d\)", body)]
        for dw, nw in re.findall(rf"\b{macro}\((\d+), (\d+)\)", src):
            direct |= {(int(dw), int(nw), rt, m) for rt, m in kinds}
    gram = {}
    arg = r"(SC_GM|SC_G1)\(([\d, ]+)\)"
    for nw, h2, pf2, h1, pf1, k1, a1, k2, a2 in re.findall(
            rf"\n  SC_G\((\d+), (\d+), (\d+), (\d+), (\d+), {arg}, {arg}\)", src):
        row = {0: {2: (int(h2), int(pf2)), 1: (int(h1), int(pf1))}}
        for kind, args in ((k1, a1), (k2, a2)):
            v = [int(x) for x in args.split(",")]
            assert v[0] == int(nw)
            row[v[-1]] = ({2: (v[1], v[2]), 1: (v[3], v[4])} if kind == "SC_GM" else {2: None, 1: (v[1], v[2])})
        gram[int(nw)] = row
    return direct, gram


def mirror_instantiations():
    """Every instantiated kernel the mirror knows: ("direct", DW, NW, RT, MODE) / ("gram", NW, RT, H, PF, MODE)."""
    out = {("direct", dw, nw, 1, m) for dw, nw in DIRECT_RT1 for m in DIRECT_MODES}
    out |= {("direct", dw, nw, 2, m) for dw, nw in DIRECT_RT2 for m in DIRECT_MODES}
    for nw, by_mode in GRAM_TABLE.items():
        for m, by_rt in by_mode.items():
            out |= {("gram", nw, rt) + hp + (m,) for rt, hp in by_rt.items() if hp is not None}
    return out


# ===================================================================== cases
MOM = (0.5, 0.25, 0.75, 0.125)     # dyadic, all different, mom[0] != 0; the kernel gets the first max(T, 1)
ETA = (0.25, 0.125, 0.5)           # per model; eta lam = 1/2, 1, 1/4
LAM = (2.0, 8.0, 0.5)
GSCALE, LSCALE = 0.25, 0.25        # coefficient search: dyadic stand-ins for 2 / (B d) and 1 / B


@dataclass(frozen=True)
class Case:
    name: str
    form: str                      # "direct" | "gram"
    d: int
    n: int
    mode: int
    rows: int = 0                  # what the launcher is given
    G: int = 3
    B: int = 48
    T: int = 3
    a0: bool = True
    wrapper: bool = False          # through ops.fista.fista(form="gram"): its GEMMs, permutation and schedule
    real: bool = False             # realistic magnitudes (``real_inputs``): bounded, not exact

    @property
    def inst(self):
        return dispatch(self.form, self.d, self.n, self.mode, self.G, self.B, self.rows)

    @property
    def key(self):
        i = self.inst
        return (self.form,) + (i[:4] if self.form == "direct" else i)

    @property
    def RT(self):
        return self.inst[2] if self.form == "direct" else self.inst[1]

    @property
    def passes(self):
        """Column passes per wave: PH (direct) / HALVES (Gram)."""
        return self.inst[4] if self.form == "direct" else self.inst[2]

    @property
    def NW(self):
        return self.n // 128

    @property
    def adjoint(self):
        return self.form == "gram" and self.mode == 2


# Held at T = 2: at T = 3 the final product A_3 D of this case (n = 2048 terms per sum) has a row whose sum of
# |terms| over its smallest unit is 2^24.6, so an fp32 partial sum may round.  Its column passes (PH = 2) are
# still run at T = 3 by modes 1 and 2 of the same tile.  The 32-row coefficient search at (8, 4) has to run 8192
# rows a model to be reached at all; at T = 3 some element of its final Res = X - c_3 D needs 25 bits.
HELD_AT_T2 = ("direct_2x16_r16_m0", "direct_8x4_r32_m1")


def _inst_cases():
    out = []
    for dw, nw in DIRECT_RT1:
        for m in DIRECT_MODES:
            name = f"direct_{dw}x{nw}_r16_m{m}"
            out.append(Case(name, "direct", 128 * dw, 128 * nw, m, T=2 if name in HELD_AT_T2 else 3))
    for dw, nw in DIRECT_RT2:
        for m in DIRECT_MODES:
            # the coefficient search reaches 32-row workgroups through the heuristic only: 256 of them
            kw = dict(G=4, B=2048) if m == 1 else dict(rows=32, B=96)
            name = f"direct_{dw}x{nw}_r32_m{m}"
            out.append(Case(name, "direct", 128 * dw, 128 * nw, m, T=2 if name in HELD_AT_T2 else 3, **kw))
    for nw, by_mode in GRAM_TABLE.items():
        for m, by_rt in by_mode.items():
            out.append(Case(f"gram_n{128 * nw}_r16_m{m}", "gram", 128 * nw, 128 * nw, m))
            if by_rt[2] is not None:
                out.append(Case(f"gram_n{128 * nw}_r32_m{m}", "gram", 128 * nw, 128 * nw, m, rows=32, B=96))
    return out


INST_CASES = _inst_cases()
EDGE_CASES = (
    [Case(f"direct_T{T}_m{m}", "direct", 256, 256, m, T=T) for T in (0, 1, 2) for m in DIRECT_MODES if (T, m) != (0, 2)]
    + [Case(f"gram_T{T}_m{m}", "gram", 256, 256, m, T=T) for T in (0, 1, 2) for m in (0, 1, 2) if T or not m]
    + [Case(f"direct_noA0_m{m}", "direct", 256, 512, m, a0=False) for m in DIRECT_MODES]
    + [Case(f"gram_noA0_m{m}", "gram", 512, 512, m, a0=False) for m in (0, 1)]
    + [Case("direct_r32_T1", "direct", 256, 256, 2, rows=32, B=96, T=1),
       Case("gram_r32_T1_m2", "gram", 256, 256, 2, rows=32, B=96, T=1),
       Case("direct_grid8", "direct", 256, 256, 2, G=2, B=64),
       Case("direct_grid8_r32", "direct", 256, 256, 0, rows=32, G=2, B=128),
       Case("gram_grid8_m1", "gram", 256, 256, 1, G=2, B=64),
       Case("gram_grid8_m2", "gram", 256, 256, 2, G=2, B=64),
       # rows = 32 asked where no 32-row kernel exists, and with B % 32 != 0: the 16-row kernel
       Case("gram_n1024_rows32_m1", "gram", 1024, 1024, 1, rows=32, B=96, T=2),
       Case("gram_n256_rows32_B48", "gram", 256, 256, 0, rows=32, B=48, T=2),
       Case("gram_wrapper", "gram", 512, 512, 0, G=2, B=128, T=2, wrapper=True)]
)
CASES = INST_CASES + EDGE_CASES


def _gen(*seed):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(seed).encode()))
    return g


def momentum_schedule(T):
    """mom[t] = (t_k - 1) / t_{k+1}, t_1 = 1 (what ``ops.fista.fista`` hands the kernel), as fp32 values."""
    out, tk = [], 1.0
    for _ in range(T):
        tn = (1.0 + (1.0 + 4.0 * tk * tk) ** 0.5) / 2.0
        out.append(float(torch.tensor((tk - 1.0) / tn, dtype=F32)))
        tk = tn
    return tuple(out)


def case_mom(case):
    """The momentum table of a case, one entry more than the kernel reads (mom[t + 1] of the planted error)."""
    return momentum_schedule(case.T + 1) if (case.wrapper or case.real) else MOM


def inputs(case: Case):
    """fp32 tensors with exactly representable values: D [G, n, d], X [G, B, d], A0 [G, B, n] or None, eta /
    lam [G], mom [max(T, 1)]; Gram: also C = X D^T and Gm = D D^T (fp64 here, asserted fp32- / bf16-exact)."""
    G, B, n, d = case.G, case.B, case.n, case.d
    gen = _gen("fista", case.name)
    D = torch.zeros(G, n, d)
    cols = torch.randint(0, d, (G, n, 4), generator=gen)
    vals = torch.tensor([1.0, -1.0, 0.5, -0.5])[torch.randint(0, 4, (G, n, 4), generator=gen)]
    D.scatter_(2, cols, vals)
    X = torch.randint(-6, 7, (G, B, d), generator=gen).float()
    A0 = (torch.randint(1, 4, (G, B, n), generator=gen) * (torch.rand(G, B, n, generator=gen) < 0.05)).float()
    inp = dict(D=D, X=X, A0=A0 if case.a0 else None,
               eta=torch.tensor([ETA[g % 3] for g in range(G)]), lam=torch.tensor([LAM[g % 3] for g in range(G)]),
               mom=torch.tensor(case_mom(case)[:max(case.T, 1)]))
    if case.form == "gram":
        C, Gm = torch.bmm(X.double(), D.double().transpose(1, 2)), torch.bmm(D.double(), D.double().transpose(1, 2))
        assert torch.equal(Gm.float().to(BF).double(), Gm), "Gm is not exact in bf16"
        assert torch.equal(C.float().double(), C), "C is not exact in fp32"
        inp.update(C=C.float(), Gm=Gm.float())
    if case.adjoint:
        fwd = gram_eval(case, inp, F64, forward_slabs=True)
        V0 = torch.randint(-3, 4, (G, B, n), generator=gen).float() * (fwd["Asave"][:, case.T - 1] != 0)
        inp.update(V0=V0, Asave=fwd["Asave"].to(BF), Qslab=fwd["Qslab"].to(BF))
    return inp


# ===================================================================== exactness bookkeeping
def lsb_unit(x):
    """The value of the lowest set mantissa bit of every element of the fp64 tensor x (inf at zeros)."""
    m, e = torch.frexp(x.abs())
    v = (m * 2.0 ** 53).to(torch.int64)
    low = (v & -v).double() * torch.exp2((e - 53).double())
    return torch.where(x == 0, torch.full_like(x, float("inf")), low)


class Exactness:
    """Collects (and asserts) the two conditions of the exact tier while a reference is evaluated."""

    def __init__(self):
        self.worst = 0.0   # the largest abs-sum / unit of any product-sum

    def rep(self, x, name):
        assert torch.equal(x.float().double(), x), f"{name} is not representable in fp32"
        return x

    def product(self, a, b, name):
        """a [G, M, K] x b [G, K, N]: per output row, sum_k |a| |b| over (smallest unit in the row of a) x
        (smallest unit in b of that model) -- a lower bound of the smallest unit among the terms."""
        ua = lsb_unit(a).amin(-1)
        ub = lsb_unit(b).amin((-1, -2))[:, None]
        live = torch.isfinite(ua) & torch.isfinite(ub)
        ratio = torch.bmm(a.abs(), b.abs()).amax(-1) / torch.where(live, ua * ub, torch.ones_like(ua))
        self.worst = max(self.worst, float(ratio[live].max()) if bool(live.any()) else 0.0)
        assert self.worst < 2.0 ** 24, f"{name}: sum of |terms| / unit = {self.worst:.3e} >= 2^24"


def bf(x):
    """Round to nearest even to bf16, kept in x's format (x holds fp32 values)."""
    return x.float().to(BF).to(x.dtype)


# ===================================================================== planted errors
MUTATIONS = ("mom_prev", "mom_next", "aprev_frozen", "aprev_frozen_pass", "eta_neighbour", "lam_neighbour",
             "thr_before_step", "last_operand_Y", "slab_shift_Y", "slab_shift_R", "slab_shift_A", "slab_shift_Q",
             "slab_shift_V", "tile_swap", "kstep_dropped", "kstep_doubled", "row_tile_alias", "res_unrounded",
             "adj_support_slot", "vsum_no_init", "coef_buf_A0")


def reachable(case: Case, mut):
    """Whether the planted error can change an output the GPU test compares in this case."""
    T, mode, direct, adj = case.T, case.mode, case.form == "direct", case.adjoint
    fista_fwd = not adj and not (direct and mode == 1)          # the FISTA recurrence itself
    saves = (direct and mode == 2) or (not direct and mode == 1)
    # the first product has a non-zero operand: the iterate at t = 0 is A0 (direct: also the final product)
    first_live = case.a0 and (T >= 1 or direct)
    if mut in ("mom_prev", "mom_next"):
        # FISTA: Y_{t+1} is seen from T >= 2 (A0 given) -- without A0, A_1 - A_0 = A_1 still carries mom[0];
        # coefficient search: the buffer starts at 0, mom[0] multiplies it: seen from mom[1] on; adjoint: mom[T-1]
        # multiplies the zero Yb_prev, so T >= 2 as well
        return T >= 2
    if mut in ("aprev_frozen", "aprev_frozen_pass"):
        if mut == "aprev_frozen_pass" and case.passes == 1:
            return False
        return T >= 3 if fista_fwd else T >= 2   # A_1 in Y_2, which iteration 2 multiplies; buffer / Yb_prev at step 1
    if mut == "eta_neighbour":
        return T >= 1
    if mut == "lam_neighbour":
        return T >= 1 and not adj
    if mut == "thr_before_step":
        return T >= 1 and fista_fwd
    if mut == "last_operand_Y":
        return direct and mode != 1 and T >= 1
    if mut.startswith("slab_shift_"):
        which = mut[-1]
        has = {"Y": saves, "R": direct and mode == 2, "A": saves, "Q": not direct and mode == 1, "V": adj}[which]
        return has and T >= 2
    if mut == "tile_swap":
        return T >= 1
    if mut in ("kstep_dropped", "kstep_doubled"):
        return (T >= 1 and adj) or (not adj and (first_live or T >= 2))
    if mut == "row_tile_alias":
        return case.RT == 2 and ((T >= 1 and adj) or (not adj and (first_live or T >= 2)))
    if mut == "res_unrounded":
        return direct and T >= 2   # Res_0 = X - A0 D is made of small multiples of 1/2: bf16 values already
    if mut == "adj_support_slot":
        return adj and T >= 2
    if mut == "vsum_no_init":
        return adj
    if mut == "coef_buf_A0":
        return direct and mode == 1 and case.a0 and T >= 1
    raise KeyError(mut)


def _last_pass_columns(case: Case):
    """Columns a wave produces in the last of its column passes (PH / HALVES)."""
    tile = (torch.arange(case.n) % (case.NW * 16)) // 16
    return tile // (case.NW // case.passes) == case.passes - 1


def _first_product(case, a, b, mut, chk, name):
    """a [G, B, K] (the bf16 iterate) x b [G, K, N]: k-steps of 32 along K, RT row tiles of 16 per workgroup."""
    if mut == "row_tile_alias" and case.RT == 2:
        a = a.view(case.G, case.B // 32, 2, 16, -1)[:, :, [0, 0]].reshape(a.shape)
    out = torch.bmm(a, b)
    if chk is not None:
        chk.product(a, b, name)
    if mut in ("kstep_dropped", "kstep_doubled"):
        step = torch.bmm(a[:, :, 32:64], b[:, 32:64])
        out = out - step if mut == "kstep_dropped" else out + step
    return out


def _swap_tiles(z, mut):
    if mut == "tile_swap":
        z = z.clone()
        z[..., :32] = torch.cat([z[..., 16:32], z[..., :16]], -1)
    return z


def _mom_at(case, mom, t, mut):
    return mom[(t + {"mom_prev": -1, "mom_next": 1}.get(mut, 0)) % len(mom)]


def _shift(slab, on):
    return slab.roll(1, 1) if on else slab


class _Steps:
    """The fp32 elementwise steps of a recurrence, each checked for exactness where a checker is given."""

    def __init__(self, chk, dtype):
        self.chk, self.dtype = chk, dtype

    def __call__(self, x, name):
        if self.dtype == F32 or self.chk is None:
            return x
        return self.chk.rep(x, name)


def _params(case, inp, dtype, mut, s):
    eta, lam = inp["eta"].to(dtype), inp["lam"].to(dtype)
    if mut == "eta_neighbour":
        eta = eta.roll(1)
    if mut == "lam_neighbour":
        lam = lam.roll(-1)
    mom = [float(m) for m in case_mom(case)]
    return eta[:, None, None], lam[:, None, None], s(eta * lam, "eta lam")[:, None, None], mom


def _fista_update(case, s, Y, Z, A, A0, e, thr, mo, t, mut, need_next):
    """y = Y + eta Z; A' = relu(y - eta lam); Y' = A' + (A' - A) mom -- every step an fp32 operation."""
    if mut == "thr_before_step":
        An = torch.relu(torch.relu(Y - thr) + e * Z)
    else:
        y = s(Y + s(e * Z, "eta Z"), "y")
        An = torch.relu(s(y - thr, "y - thr"))
    Ap = A0 if mut == "aprev_frozen" else A
    if mut == "aprev_frozen_pass":
        Ap = torch.where(_last_pass_columns(case).to(A.device), A0, A)
    Yn = s(An + s(s(An - Ap, "A - A_prev") * mo, "(A - A_prev) mom"), "Y") if need_next else None
    return An, Yn


# ===================================================================== direct form
def direct_eval(case: Case, inp, dtype=F64, mut=None, chk: Optional[Exactness] = None, dev="cpu"):
    """Modes 0 / 2: {A, Res} (+ the slabs Ysave, Rsave, Asave [G, T, B, *], bf16 values); mode 1 (coefficient
    search): {A, Res}.  ``dtype`` F64: the reference; F32: the plain evaluation with the same rounding points."""
    G, B, n, d, T, mode = case.G, case.B, case.n, case.d, case.T, case.mode
    s = _Steps(chk, dtype)
    D, X = inp["D"].to(dev, dtype), inp["X"].to(dev, dtype)
    Dt = D.transpose(1, 2).contiguous()
    e, lam, thr, mom = _params(case, {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}, dtype, mut, s)
    A0 = torch.zeros(G, B, n, dtype=dtype, device=dev) if inp["A0"] is None else inp["A0"].to(dev, dtype)
    Y, A = A0, A0
    buf = A0 if mut == "coef_buf_A0" else torch.zeros_like(A0)
    buf0 = buf
    gscale, lscale = inp.get("gscale", GSCALE), inp.get("lscale", LSCALE)
    lsc = s(lam * lscale, "lam lscale")
    Ys, Rs, As, raw = [], [], [], {"Res": [], "A": []}
    for t in range(T):
        Yb = bf(Y)
        Res = s(X - _first_product(case, Yb, D, mut, chk, f"Y_{t} D"), f"Res_{t}")
        Rb = Res if mut == "res_unrounded" else bf(Res)
        if chk is not None:
            chk.product(Rb, Dt, f"Res_{t} D^T")
        Z = _swap_tiles(torch.bmm(Rb, Dt), mut)
        mo = _mom_at(case, mom, t, mut)
        Ys.append(Yb)
        Rs.append(bf(Res))
        raw["Res"].append(Res)
        if mode != 1:
            need = t + 1 < T or mut == "last_operand_Y"
            A, Yn = _fista_update(case, s, Y, Z, A, A0, e, thr, mo, t, mut, need)
            Y = Yn if need else A
        else:
            g = s(torch.where(Y > 0, lsc.expand_as(Y), torch.zeros_like(Y)) - s(Z * gscale, "gscale Z"), "g")
            prev = buf0 if mut == "aprev_frozen" else buf
            if mut == "aprev_frozen_pass":
                prev = torch.where(_last_pass_columns(case).to(dev), buf0, buf)
            buf = s(s(prev * mo, "mom buf") + g, "buf")
            A = torch.relu(s(Y - s(e * buf, "lr buf"), "c - lr buf"))
            Y = A
        As.append(bf(A))
        raw["A"].append(A)
    last = bf(Y if mut == "last_operand_Y" else A)
    out = {"A": A, "Res": s(X - _first_product(case, last, D, mut, chk, "A_T D"), "Res")}
    out.update({f"_{k}": torch.stack(v, 1) for k, v in raw.items() if v})  # unrounded, for the bounded tier
    if mode == 2:
        out["Ysave"] = _shift(torch.stack(Ys, 1), mut == "slab_shift_Y")
        out["Rsave"] = _shift(torch.stack(Rs, 1), mut == "slab_shift_R")
        out["Asave"] = _shift(torch.stack(As, 1), mut == "slab_shift_A")
    return out


# ===================================================================== Gram form
def gram_eval(case: Case, inp, dtype=F64, mut=None, chk: Optional[Exactness] = None, dev="cpu", forward_slabs=False):
    """Modes 0 / 1: {A} (+ Ysave, Asave, Qslab); mode 2 (the adjoint sweep): {cbar, Vsum, Vslab, epart
    [G, B / 16] (fp64 sums of the workgroups, zero past B / R), eabs (sum |v q| per workgroup, for the bound)}.
    ``forward_slabs``: the forward's slabs whatever the mode (the adjoint's inputs)."""
    G, B, n, T = case.G, case.B, case.n, case.T
    s = _Steps(chk, dtype)
    inp = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}
    Gm = inp["Gm"].to(dtype)
    e, lam, thr, mom = _params(case, inp, dtype, mut, s)
    if case.adjoint and not forward_slabs:
        return _adjoint_eval(case, inp, dtype, mut, chk, s, Gm, e, mom)
    C = inp["C"].to(dtype)
    A0 = torch.zeros(G, B, n, dtype=dtype, device=dev) if inp["A0"] is None else inp["A0"].to(dtype)
    Y, A = A0, A0
    Ys, As, Qs, raw = [], [], [], {"Q": [], "A": []}
    for t in range(T):
        Yb = bf(Y)
        Q = s(C - _swap_tiles(_first_product(case, Yb, Gm, mut, chk, f"Y_{t} Gm"), mut), f"Q_{t}")
        need = t + 1 < T
        A, Yn = _fista_update(case, s, Y, Q, A, A0, e, thr, _mom_at(case, mom, t, mut), t, mut, need)
        Y = Yn if need else A
        Ys.append(Yb)
        As.append(bf(A))
        Qs.append(bf(Q))
        raw["Q"].append(Q)
        raw["A"].append(A)
    out = {"A": A}
    out.update({f"_{k}": torch.stack(v, 1) for k, v in raw.items() if v})
    if case.mode == 1 or forward_slabs:
        out["Ysave"] = _shift(torch.stack(Ys, 1), mut == "slab_shift_Y")
        out["Asave"] = _shift(torch.stack(As, 1), mut == "slab_shift_A")
        out["Qslab"] = _shift(torch.stack(Qs, 1), mut == "slab_shift_Q")
    return out


def _adjoint_eval(case, inp, dtype, mut, chk, s, Gm, e, mom):
    """Reverse time t = T-1 .. 0 with Vbar_{T-1} = V0:  Yb = Vbar - eta Vbar Gm;  t >= 1: Vbar_{t-1} =
    ((1 + mom[t-1]) Yb - mom[t] Yb_prev) 1[A_t > 0] (A_t in slot t - 1 of Asave);  t == 0: cbar = Yb - mom[0]
    Yb_prev.  Vsum = sum_t Vbar_t; the slab holds bf16(Vbar_t) in slot t; epart = sum_t <Vbar_t, Q_t> per
    workgroup (fp32 Vbar, the forward's bf16 Q)."""
    G, B, n, T = case.G, case.B, case.n, case.T
    R = 16 * case.RT
    V = inp["V0"].to(dtype)
    Asave, Qslab = inp["Asave"].to(dtype), inp["Qslab"].to(dtype)
    Yprev0 = torch.zeros_like(V)
    Yprev = Yprev0
    Vsum = torch.zeros_like(V) if mut == "vsum_no_init" else V
    slots = [None] * T
    slots[T - 1] = bf(V)
    edot = torch.zeros(G, B // R, dtype=F64, device=V.device)
    eabs = torch.zeros_like(edot)
    cbar = None
    for it in range(T):
        ts = T - 1 - it
        mo = _mom_at(case, mom, ts, mut)
        Z = _swap_tiles(_first_product(case, bf(V), Gm, mut, chk, f"Vbar_{ts} Gm"), mut)
        vq = (V.double() * Qslab[:, ts].double()).view(G, B // R, R * n)
        edot, eabs = edot + vq.sum(-1), eabs + vq.abs().sum(-1)
        yb = s(V - s(e * Z, "eta Z"), "Yb")
        prev = Yprev0 if mut == "aprev_frozen" else Yprev
        if mut == "aprev_frozen_pass":
            prev = torch.where(_last_pass_columns(case).to(V.device), Yprev0, Yprev)
        if ts == 0:
            cbar = s(yb - s(prev * mo, "mom Yb_prev"), "cbar")
        else:
            m1 = float(torch.tensor(1.0, dtype=F32) + torch.tensor(mom[ts - 1], dtype=F32))  # formed in fp32
            supp = Asave[:, ts if mut == "adj_support_slot" else ts - 1] != 0
            ab = s(s(yb * m1, "(1 + mom) Yb") - s(prev * mo, "mom Yb_prev"), "Abar")
            V = torch.where(supp, ab, torch.zeros_like(ab))
            Vsum = s(Vsum + V, "Vsum")
            slots[ts - 1] = bf(V)
        Yprev = yb
    epart = torch.zeros(G, B // 16, dtype=F64, device=V.device)
    epart[:, :B // R] = edot
    return {"cbar": cbar, "Vsum": Vsum, "Vslab": _shift(torch.stack(slots, 1), mut == "slab_shift_V"),
            "epart": epart, "eabs": eabs}


def evaluate(case: Case, inp, dtype=F64, mut=None, chk=None, dev="cpu"):
    return (direct_eval if case.form == "direct" else gram_eval)(case, inp, dtype, mut, chk, dev)


EXACT_OUTPUTS = ("A", "Res", "Ysave", "Rsave", "Asave", "Qslab", "cbar", "Vsum", "Vslab")


def check_exact(case: Case, inp):
    """Proves the case exact from its inputs (asserts), returns the reference and the checker."""
    for k in ("D", "X"):
        assert torch.equal(inp[k].to(BF).float(), inp[k]), f"{k} is not exact in bf16"
    chk = Exactness()
    ref = evaluate(case, inp, F64, chk=chk)
    for k in EXACT_OUTPUTS:
        if k in ref:
            chk.rep(ref[k], k)
    return ref, chk


def epart_bound(case: Case, ref):
    """What fp32 accumulation may cost ``epart.sum(1)``: gamma_k sum |v q| with k the number of roundings on the
    way of one term -- its product, the T R n - 1 additions of its workgroup (any order: at most that many) and
    the B / 16 - 1 of the final sum over workgroups."""
    k = case.T * 16 * case.RT * case.n + case.B // 16
    u = k * 2.0 ** -24
    return u / (1 - u) * ref["eabs"].sum(1)


# ===================================================================== elementwise adjoint kernels
ADJ_G, ADJ_B, ADJ_N, ADJ_T = 3, 5, 77, 4   # G B n = 1155 elements: not a multiple of the 256-thread block


def adjoint_kernel_inputs():
    """Dyadic inputs of ``sc_fista_adjoint_init`` / ``sc_fista_adjoint`` (fista_update.hip): every step exact."""
    gen = _gen("adjoint kernels")
    shape = (ADJ_G, ADJ_B, ADJ_N)
    ints = lambda lo, hi, *sh: torch.randint(lo, hi, sh, generator=gen).float()  # noqa: E731
    aslab = (ints(0, 3, ADJ_G, ADJ_T, ADJ_B, ADJ_N) * 0.5).to(BF)   # about a third of the support empty
    return dict(T2=ints(-9, 10, *shape) * 0.25, Vbar=ints(-9, 10, *shape) * 0.5, Ynext=ints(-9, 10, *shape) * 0.125,
                Aslab=aslab, eta=torch.tensor(ETA))


def adjoint_kernel_eval(inp, t, mut=None):
    """fp64 {Ycur, Vbar, cbar | Vslot} of step t (``init``: t = None -> {Vbar, Vslot}); asserts exactness."""
    rep = Exactness().rep
    T2, V, Yn = (inp[k].double() for k in ("T2", "Vbar", "Ynext"))
    A = inp["Aslab"].double()
    if t is None:
        v = torch.where(A[:, ADJ_T - 1] > 0, -T2, torch.zeros_like(T2))
        return {"Vbar": v, "Vslot": bf(v)}
    m_prev, m_t = (MOM[t - 1] if t >= 1 else 0.0), MOM[t]
    yb = rep(V + rep(inp["eta"].double()[:, None, None] * T2, "eta T2"), "Yb")
    if t == 0:
        return {"Ycur": yb, "cbar": rep(yb - rep(Yn * m_t, "m Ynext"), "cbar")}
    m1 = float(torch.tensor(1.0) + torch.tensor(m_prev))
    ab = rep(rep(yb * m1, "(1 + m) Yb") - rep(Yn * m_t, "m Ynext"), "Abar")
    v = torch.where(A[:, t if mut == "slot" else t - 1] > 0, ab, torch.zeros_like(ab))
    return {"Ycur": yb, "Vbar": v, "Vslot": bf(v)}


# ===================================================================== dictionary update (fista_update.hip)
@dataclass(frozen=True)
class UpdateCase:
    name: str
    G: int
    n: int
    d: int
    row_mode: bool
    nonneg: bool
    shadow: bool


UPDATE_CASES = [UpdateCase(f"{'row' if r else 'col'}_n{n}_d{d}{'_nonneg' if nn else ''}{'_shadow' if sh else ''}",
                           3, n, d, r, nn, sh)
                for r, n in ((True, 7), (False, 6)) for d in (128, 384) for nn in (False, True) for sh in (False, True)]
LOWEST = float(torch.tensor(1e-3, dtype=F32))
HESSIAN_SHAPES = ((3, 13, 128), (2, 6, 64))   # (G, B, n): B no multiple of the 4 row groups
HISTORY = 300.0


def update_inputs(case: UpdateCase):
    """D, dBt [G, n, d], H [G, n]: atom 1 of every model all zero (the norm floor of row mode), column 5 all zero
    (the floor of column mode), atom 2 negative after the update (``nonneg`` clamps the whole row)."""
    gen = _gen("update", case.name)
    G, n, d = case.G, case.n, case.d
    D = torch.randn(G, n, d, generator=gen) / d ** 0.5
    U = 0.05 * torch.randn(G, n, d, generator=gen)
    H = 0.1 * torch.rand(G, n, generator=gen)
    D[:, 2] = -D[:, 2].abs() - 0.01
    U[:, 2] = -U[:, 2].abs()
    D[:, 1], U[:, 1] = 0.0, 0.0
    D[:, :, 5], U[:, :, 5] = 0.0, 0.0
    return dict(D=D, U=U, H=H)


def update_eval(case: UpdateCase, inp, dtype):
    """D' = D + dBt / (H + lowest) per atom, clamp, renormalise rows (floor 1e-8) or columns (floor 1e-30)."""
    from step_update_cases import seqsum

    D, U, H = (inp[k].to(dtype) for k in ("D", "U", "H"))
    v = D + U / (H + torch.tensor(LOWEST, dtype=dtype))[..., None]
    if case.nonneg:
        v = v.clamp(min=0)
    if case.row_mode:
        nrm = torch.maximum(seqsum(v * v, -1).sqrt(), torch.tensor(1e-8, dtype=F32).to(dtype))[..., None]
    else:
        nrm = torch.maximum(seqsum(v * v, 1).sqrt(), torch.tensor(1e-30, dtype=F32).to(dtype))[:, None]
    return {"D": v / nrm}


def hessian_inputs(G, B, n):
    gen = _gen("hessian", G, B, n)
    A = torch.relu(torch.randn(G, B, n, generator=gen) - 0.5)
    A[:, :, 3] = 0.0
    return dict(A=A, H=0.1 * torch.rand(G, n, generator=gen))


def hessian_eval(inp, dtype):
    """H' = H (history - 1) / history + mean_b(A^2) / history, the two factors formed as the launcher forms them."""
    from step_update_cases import seqsum

    A, H = inp["A"].to(dtype), inp["H"].to(dtype)
    h = torch.tensor(HISTORY, dtype=F32)
    keep, scale = ((h - 1) / h).to(dtype), (1 / (h * A.shape[1])).to(dtype)
    return {"H": keep * H + scale * seqsum(A * A, 1)}


# ===================================================================== realistic magnitudes, T = 1
REAL_CASES = ([Case(f"real_direct_m{m}", "direct", 256, 512, m, T=1, real=True) for m in DIRECT_MODES]
              + [Case(f"real_gram_m{m}", "gram", 256, 256, m, T=1, real=True) for m in (0, 1, 2)])


def real_inputs(case: Case):
    """Unit-norm random atoms and 0.3 N(0, 1) data as the bf16 values the kernels multiply, a rectified warm
    start, eta = 1 / lambda_max(D D^T), lam of 1e-3 .. 2e-2 (eta lam is no fp32-friendly number), the momentum
    schedule of ``ops.fista``; the coefficient search with its own 2 / (B d) and 1 / B."""
    G, B, n, d = case.G, case.B, case.n, case.d
    gen = _gen("real", case.name)
    D = torch.nn.functional.normalize(torch.randn(G, n, d, generator=gen), dim=-1).to(BF).float()
    X = (0.3 * torch.randn(G, B, d, generator=gen)).to(BF).float()
    A0 = 0.05 * torch.relu(torch.randn(G, B, n, generator=gen))
    gm = torch.bmm(D.double(), D.double().transpose(1, 2))
    inp = dict(D=D, X=X, A0=A0, eta=(1.0 / torch.linalg.eigvalsh(gm).amax(-1)).float(),
               lam=torch.tensor([1e-3, 5e-3, 2e-2]), mom=torch.tensor(case_mom(case)[:1]),
               gscale=float(torch.tensor(2.0 / (B * d), dtype=F32)), lscale=float(torch.tensor(1.0 / B, dtype=F32)))
    if case.form == "gram":
        inp.update(C=torch.bmm(X.double(), D.double().transpose(1, 2)).float(), Gm=gm.float().to(BF).float())
    if case.adjoint:
        fwd = gram_eval(case, inp, F64, forward_slabs=True)
        V0 = torch.randn(G, B, n, generator=gen) * (fwd["Asave"][:, 0] != 0)
        inp.update(V0=V0, Asave=fwd["Asave"].to(BF), Qslab=fwd["Qslab"].to(BF))
    return inp


def bf16_ulp(x):
    """The spacing of bf16 values at |x| (fp64 tensor)."""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


def tie_distance(x):
    """Distance of x to the nearest point where its bf16 rounding switches (the midpoints of its binade)."""
    u = bf16_ulp(x)
    return ((x.abs() / u) % 1.0 - 0.5).abs() * u


def real_check_parts(case: Case, inp, margin):
    """(ref, E32, extra, exact) for ``step_update_cases.compare``: the fp64 reference against the plain fp32
    evaluation of the same recurrence with the same rounding points.  Slabs enter as ``sv_*``: the unrounded
    value, which ``compare`` allows half a bf16 ulp more.

    The direct form rounds Res_0 to bf16 before the second product, and A_1 before the final one.  A value the
    kernel forms within ``margin x E32`` of the reference may round to the other neighbour where the reference
    lies that close to a tie; that moves the operand by one bf16 ulp.  ``extra`` is that effect carried through
    the product, elementwise: for A, eta (gscale) sum_k ulp(Res_0[b, k]) |D[j, k]| over the ambiguous k; for the
    final Res, sum_j delta[b, j] |D[j, k]| with delta one ulp at the entries of A_1 that are ambiguous under
    their own bound (or whose pre-activation is within it of the relu's kink)."""
    from step_update_cases import e32_of

    ref, plain = evaluate(case, inp, F64), evaluate(case, inp, F32)
    slabs = {"Rsave": "_Res", "Asave": "_A", "Qslab": "_Q"}

    def view(out):
        o = {k: v for k, v in out.items() if k in ("A", "Res", "cbar", "Vsum", "Ysave", "Vslab")}
        for k, raw in slabs.items():
            if k in out:
                o["sv_" + k] = out[raw]
        return o

    r, p = view(ref), view(plain)
    e32 = e32_of(p, r)
    exact = tuple(k for k in ("Ysave", "Vslab", "Vsum") if k in r)   # roundings / copies of the inputs
    extra = {}
    if case.form == "direct":
        absD = inp["D"].double().abs()
        R0 = ref["_Res"][:, 0]
        eR = margin * float((plain["_Res"][:, 0].double() - R0).abs().max())
        w = torch.where(tie_distance(R0) <= eR, bf16_ulp(R0), torch.zeros_like(R0))
        scale = inp["eta"].double()[:, None, None] * (inp["gscale"] if case.mode == 1 else 1.0)
        extra["A"] = scale * torch.bmm(w, absD.transpose(1, 2))
        bound = margin * e32["A"] + extra["A"]
        A = ref["A"]
        amb = (tie_distance(A) <= bound) | (A <= bound)
        delta = torch.where(amb, bf16_ulp(A.abs() + bound), torch.zeros_like(A))
        extra["Res"] = torch.bmm(delta, absD)
        if "sv_Asave" in r:
            extra["sv_Asave"] = extra["A"][:, None]
    return r, e32, extra, exact
