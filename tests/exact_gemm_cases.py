"""Cases for the bit-exact tests of the grouped MFMA GEMM (not collected: no ``test_`` prefix).

Every input is a bf16 tensor of small integers and every scalar is dyadic, so each product and each
partial sum the kernel can form is an integer (or a dyadic multiple) below 2^24: every fp32
accumulation order gives the same bits and the fp64 result of plain torch ops is the only right
answer.  This module holds the table of K-loop instantiations, the input recipes, the fp64
references, the assertions on the inputs and the coverage accounting; ``test_gemm_exact_cpu.py``
runs all of it without a GPU, ``test_gemm_exact_gpu.py`` compares the kernels against it with
``torch.equal``.
"""

from __future__ import annotations

import functools

import torch

BF = torch.bfloat16
F64 = torch.float64
EXACT = float(1 << 24)  # integers below this magnitude are exact in fp32

# cfg -> (BM, BN, BK, NST, K-loop body, FULL): csrc/sae_gemm.hip, sae_gemm_big.hip, sae_gemm_256x128.hip.
# Loop bodies (csrc/sae_gemm_kernel.h, gemm_block): "bk64pipe" the software-pipelined BK64 loop
# (steady / drain / peeled last tile), "p32" the pipelined BK32 loop unrolled by two, "plain".
# FULL instantiates every (layout, epilogue) pair; the others the step epilogues, fp32 layout 0 and
# bf16 layouts 0 and 3.
CFG_TABLE = {
    1: (128, 128, 64, 2, "bk64pipe", True),
    5: (128, 128, 64, 3, "bk64pipe", False),
    9: (128, 128, 32, 2, "plain", False),
    13: (128, 128, 32, 3, "plain", False),
    25: (128, 128, 32, 2, "p32", False),
    29: (128, 128, 32, 3, "p32", False),
    2: (256, 128, 64, 2, "bk64pipe", True),
    14: (256, 128, 32, 3, "plain", False),
    3: (256, 256, 64, 2, "plain", True),
    7: (256, 256, 32, 4, "plain", False),
    11: (256, 256, 32, 2, "plain", False),
    15: (256, 256, 32, 3, "plain", False),
}
ALL_CFGS = list(CFG_TABLE)
FULL_CFGS = [c for c, v in CFG_TABLE.items() if v[5]]
REFUSED_CFGS = [6, 10]  # 256x128 blocks exist on the BK64 x 2 and the eight-wave BK32 x 3 rings only

EPI_F32, EPI_BF16, EPI_ENC_ACT, EPI_DC_ACT, EPI_ROWMAX = 3, 4, 8, 9, 10


def block(cfg):
    return CFG_TABLE[cfg][:2]


def ring(cfg):
    return CFG_TABLE[cfg][2:4]


def max_l(cfg):
    """The K-tile counts 1 .. 2 NST + 3 reach every phase of every loop body (fewer tiles than
    stages, the steady loop once and twice, the drain, both tail parities)."""
    return 2 * CFG_TABLE[cfg][3] + 3


def plain_combos(cfg):
    """(output dtype, operand layout) pairs of the plain epilogues this cfg instantiates
    (layout bit 0: A is K-major, bit 1: B is K-major)."""
    if CFG_TABLE[cfg][5]:
        return [(dt, lay) for dt in (torch.float32, BF) for lay in (0, 1, 2, 3)]
    return [(torch.float32, 0), (BF, 0), (BF, 3)]


def refused_launches():
    """(cfg, epilogue, layout) the launcher must refuse (no such instantiation)."""
    out = [(cfg, EPI_F32, 0) for cfg in REFUSED_CFGS]
    for cfg in ALL_CFGS:
        if CFG_TABLE[cfg][5]:
            continue
        out += [(cfg, epi, 3) for epi in (EPI_ENC_ACT, EPI_DC_ACT, EPI_ROWMAX)]
        out += [(cfg, EPI_F32, lay) for lay in (1, 2, 3)]
        out += [(cfg, EPI_BF16, lay) for lay in (1, 2)]
    return out


# ------------------------------------------------------------------ K values and coverage
def whole_k_values(cfg):
    """Whole-K launches: every tile count 1 .. 2 NST + 3 on a BK64 ring; K % 64 == 0 leaves only the
    even counts on a BK32 ring."""
    bk = CFG_TABLE[cfg][2]
    return [t * bk for t in range(1, max_l(cfg) + 1) if (t * bk) % 64 == 0]


# (K, ksplit): uneven floor(ksi * nk / ksplit) ranges.  The launcher refuses ksplit > K / 64, so a
# split range on a BK32 ring holds at least two tiles; one tile is reached through NACT_K below.
SPLITS = [(192, 3), (320, 3), (448, 3), (576, 2), (640, 3), (704, 2)]
# a plain launch with per-model live K ranges (G = 3): K-tile counts ceil(live / BK)
NACT_K = (320, (32, 96, 224))
# two K segments of different lengths: (K1, K2)
SEGMENTS = [(64, 128), (128, 64), (64, 64), (192, 64)]


def split_ranges(k_total, bk, ksplit):
    nk = k_total // bk
    return [(ksi * nk // ksplit, (ksi + 1) * nk // ksplit) for ksi in range(ksplit)]


def straddling_split(k1, k2, bk):
    """The smallest ksplit >= 2 with a K-tile range that holds tiles of both segments (None when
    the ranges of every allowed ksplit end on the segment boundary)."""
    for ks in range(2, (k1 + k2) // 64 + 1):
        if any(a < k1 // bk < b for a, b in split_ranges(k1 + k2, bk, ks)):
            return ks
    return None


def plain_k_ranges(cfg):
    """Every (kbeg, nk) K-tile range a block of the plain-epilogue tests of this cfg runs."""
    bk = CFG_TABLE[cfg][2]
    out = [(0, k // bk) for k in whole_k_values(cfg)]
    for k, ks in SPLITS:
        out += split_ranges(k, bk, ks)
    out += [(0, -(-live // bk)) for live in NACT_K[1]]
    for k1, k2 in SEGMENTS:
        out.append((0, (k1 + k2) // bk))
        ks = straddling_split(k1, k2, bk) or 2
        out += split_ranges(k1 + k2, bk, ks)
    return out


def covered_l(cfg):
    return {nk - kbeg for kbeg, nk in plain_k_ranges(cfg)}


def fused_k_values(cfg):
    """K of the fused-epilogue cases: one and two BK64 tiles, one more than the ring is deep, 640."""
    return sorted({64, 128, 64 * (CFG_TABLE[cfg][3] + 1), 640})


# masked ensembles: live sizes that are not tile-aligned, odd K-tile counts on BK32 (96 -> 3, 32 -> 1)
MASK_N = 256
MASK_SIZES = [MASK_N, 100, 96, 32]
MASK_SIZES_ZERO = [MASK_N, 100, 0, 32]


def coverage_table():
    """Rows (cfg, block, ring, loop, plain (dtype/layout) pairs, covered L, fused K values)."""
    rows = []
    for cfg, (bm, bn, bk, nst, loop, _) in CFG_TABLE.items():
        combos = " ".join(("f32" if dt == torch.float32 else "bf16") + f"/{lay}" for dt, lay in plain_combos(cfg))
        ls = sorted(covered_l(cfg))
        dec_l = sorted({-(-s // bk) for s in MASK_SIZES})
        rows.append(f"cfg {cfg:2d}  {bm}x{bn}  BK{bk}x{nst}  {loop:8s}  plain [{combos}]  L={ls}  "
                    f"fused K={fused_k_values(cfg)}  masked-decoder L={dec_l}")
    return rows


# ------------------------------------------------------------------ integer inputs
def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def ternary(shape, density, g):
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    keep = torch.rand(shape, generator=g) < density
    return (sign * keep).to(torch.float32)


def ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float32)


POOL_G, POOL_M, POOL_N, POOL_K = 3, 512, 768, 704  # nothing larger is ever launched


@functools.lru_cache(maxsize=None)
def plain_pool(kind, seed=0):
    """Logical operands A [G, M, K], B [G, N, K] (fp32 holding integers) the plain-epilogue cases
    slice: "int" in [-3, 3] for fp32 outputs, "ter" ternary at density 1/2 for bf16 outputs."""
    g = _gen(100 + seed + (0 if kind == "int" else 50))
    if kind == "int":
        return ints((POOL_G, POOL_M, POOL_K), -3, 3, g), ints((POOL_G, POOL_N, POOL_K), -3, 3, g)
    return ternary((POOL_G, POOL_M, POOL_K), 0.5, g), ternary((POOL_G, POOL_N, POOL_K), 0.5, g)


def pool_kind(dtype):
    return "int" if dtype == torch.float32 else "ter"


@functools.lru_cache(maxsize=None)
def encoder_inputs(G, B, n, d, bias_lo=-6, bias_hi=0, seed=0):
    g = _gen(200 + seed)
    return dict(x=ternary((G, B, d), 0.5, g), w=ternary((G, n, d), 0.5, g), bias=ints((G, n), bias_lo, bias_hi, g))


@functools.lru_cache(maxsize=None)
def decoder_inputs(G, B, n, d, seed=0):
    g = _gen(300 + seed)
    c = ints((G, B, n), 1, 3, g) * (torch.rand((G, B, n), generator=g) < 0.125)
    return dict(c=c, wd=ternary((G, n, d), 0.25, g), x=ternary((G, B, d), 0.5, g))


@functools.lru_cache(maxsize=None)
def codegrad_inputs(G, B, n, d, seed=0):
    g = _gen(400 + seed)
    l1 = torch.tensor([2.0 ** -5 * (i + 1) for i in range(G)])
    return dict(r=ints((G, B, d), -3, 3, g), w=ternary((G, n, d), 0.5, g), l1=l1, tied_bias=ints((G, n), -6, 0, g))


@functools.lru_cache(maxsize=None)
def wgrad_masked_inputs(G, Bk, n, d, sizes, seed=0):
    """Weight-gradient operands of a masked ensemble: A (codes / code gradients, [G, Bk, n]) is zero
    past each model's live size, as the encoder and the code gradient leave it."""
    g = _gen(500 + seed)
    a = ints((G, Bk, n), -3, 3, g)
    for i, s in enumerate(sizes):
        a[i, :, s:] = 0
    return dict(a=a, b=ternary((G, Bk, d), 0.5, g))


# ------------------------------------------------------------------ fp64 references
def ref_plain(a, b, alpha=1.0):
    """alpha * A B^T of logical operands A [G or 1, M, K], B [G or 1, N, K]."""
    return alpha * (a.to(F64) @ b.to(F64).transpose(-1, -2))


def _slot_sums(t, slot=128):
    G, B, n = t.shape
    return t.reshape(G, B // slot, slot, n).sum(2)


def ref_encode(x, w, bias, live=None, reverse=False):
    """Codes, L1 / L0 totals per model and per-128-row-slot fire counts of the encoder epilogues."""
    acc = ref_plain(x if x.dim() == 3 else x[None], w)
    pre = acc + bias.to(F64)[:, None, :]
    on = pre > 0
    if live is not None:
        cols = torch.arange(w.shape[1], device=w.device)
        on = on & (cols[None, None, :] < torch.as_tensor(live, device=w.device)[:, None, None])
    c = torch.where(on, acc if reverse else pre, torch.zeros_like(pre))
    return dict(c=c, on=on, l1=c.abs().sum((1, 2)), l0=on.to(F64).sum((1, 2)), cnt=_slot_sums(on.to(F64)), pre=pre)


def ref_decode(c, wd, x):
    r = c.to(F64) @ wd.to(F64) - (x if x.dim() == 3 else x[None]).to(F64)
    return dict(r=r, sq=(r * r).sum((1, 2)), rcol=_slot_sums(r))


def ref_code_grad(r, w, c, on, l1, tied_bias=None, reverse=False):
    """dpre, its per-slot column sums and the norm-Jacobian row dots of the code-gradient epilogues."""
    d = r.shape[-1]
    acc = ref_plain(r, w)
    add = (l1.to(F64) * (d / 2.0))[:, None, None]
    cf = c.to(F64)
    if reverse:
        dpre = torch.where(on, acc + add * torch.sign(cf), torch.zeros_like(acc))
        return dict(dpre=dpre, colpart=torch.zeros_like(_slot_sums(dpre)), acc=acc)
    dpre = torch.where(on, acc + add, torch.zeros_like(acc))
    out = dict(dpre=dpre, colpart=_slot_sums(dpre), dot=_slot_sums(cf * acc), acc=acc)
    if tied_bias is not None:
        out["dot_tied"] = _slot_sums(cf * acc + dpre * (cf - tied_bias.to(F64)[:, None, :]))
    return out


# ------------------------------------------------------------------ the input conditions
def assert_exact(t, what, unit=1.0):
    """Every value is a multiple of ``unit`` (a power of two) of magnitude below 2^24 units."""
    q = t.to(F64) / unit
    assert torch.equal(q, q.round()), f"{what}: not a multiple of {unit}"
    assert q.abs().max().item() < EXACT, f"{what}: magnitude {q.abs().max().item()} >= 2^24"


def assert_bf16_out(t, what):
    assert torch.equal(t, t.round()) and t.abs().max().item() <= 256, f"{what}: bf16 output not an integer <= 256"
    assert torch.equal(t.float().to(BF).to(F64), t), what


def assert_accumulators(a, b, what, unit=1.0):
    """sum_k |a| |b| bounds every partial sum of every accumulation order of A B^T."""
    bound = (a.to(F64).abs() @ b.to(F64).abs().transpose(-1, -2)).max().item() / unit
    assert bound < EXACT, f"{what}: accumulator bound {bound}"


def assert_sum_exact(t, what, unit=1.0, slots=False):
    """Any partial sum of the values one output sums is exact (their magnitudes sum below 2^24):
    all of a model's values for a scalar partial, one column of a 128-row slot with ``slots``."""
    assert_exact(t, what, unit)
    mag = t.to(F64).abs() / unit
    tot = (_slot_sums(mag) if slots else mag.reshape(t.shape[0], -1).sum(1)).max().item()
    assert tot < EXACT, f"{what}: sum of magnitudes {tot} >= 2^24"


def assert_active(on, what):
    frac = on.to(F64).mean().item()
    assert 0.10 <= frac <= 0.90, f"{what}: {frac:.3f} of the codes active"


def assert_k_tiles_contribute(a, b, what, k_lo=0, k_hi=None, tile=32):
    """Every K-tile (of the finest ring, 32 deep) adds something non-zero to every model's product."""
    a, b = (a if a.dim() == 3 else a[None]).to(F64), (b if b.dim() == 3 else b[None]).to(F64)
    k_hi = a.shape[-1] if k_hi is None else k_hi
    flags = []
    for k in range(k_lo, k_hi, tile):
        part = a[..., k:k + tile] @ b[..., k:k + tile].transpose(-1, -2)
        flags.append(part.reshape(part.shape[0], -1).ne(0).any(1).all())
    assert bool(torch.stack(flags).all()), f"{what}: a K-tile contributes nothing ({[bool(f) for f in flags]})"


def check_plain(a, b, alpha, dtype, what):
    ref = ref_plain(a, b, alpha)
    assert_accumulators(a, b, what)
    assert_exact(ref, what, unit=0.5)
    if dtype == BF:
        assert_bf16_out(ref, what)
    assert_k_tiles_contribute(a, b, what)
    return ref


def check_encode(x, w, bias, live=None, reverse=False, what="encoder"):
    ref = ref_encode(x, w, bias, live, reverse)
    assert_accumulators(x if x.dim() == 3 else x[None], w, what)
    assert_exact(ref["pre"], what)
    assert_bf16_out(ref["c"], what + " codes")
    assert_sum_exact(ref["c"], what + " L1")
    if live is None:
        assert_active(ref["on"], what)
    else:  # judged on the live columns
        for g, s in enumerate(live):
            if s:
                assert_active(ref["on"][g, :, :s], f"{what} model {g}")
    assert_k_tiles_contribute(x, w, what)
    return ref


def check_decode(c, wd, x, what="decoder", live=None):
    ref = ref_decode(c, wd, x)
    assert_accumulators(c, wd.transpose(-1, -2), what)
    assert_bf16_out(ref["r"], what + " r")
    assert_sum_exact(ref["r"] * ref["r"], what + " sum r^2")
    assert_sum_exact(ref["r"], what + " rcol", slots=True)
    for g in range(c.shape[0]):
        hi = c.shape[-1] if live is None else live[g]
        if hi:
            assert_k_tiles_contribute(c[g:g + 1], wd[g:g + 1].transpose(-1, -2), f"{what} model {g}", 0, hi)
    return ref


def check_code_grad(r, w, c, on, l1, tied_bias=None, reverse=False, what="code gradient", live=None):
    ref = ref_code_grad(r, w, c, on, l1, tied_bias, reverse)
    assert_accumulators(r, w, what)
    add = l1.to(F64) * (r.shape[-1] / 2.0)
    assert torch.equal(add, add.round()), f"{what}: l1 d / 2 is not an integer"
    assert_bf16_out(ref["dpre"], what + " dpre")
    for g in range(on.shape[0]):  # (masked ensembles: judged on the live columns)
        hi = on.shape[-1] if live is None else live[g]
        if hi:
            assert_active(on[g, :, :hi], f"{what} model {g}")
    assert_sum_exact(ref["dpre"], what + " column sums", slots=True)
    if not reverse:
        cf = c.to(F64)
        assert_sum_exact(cf * ref["acc"], what + " dotpart", slots=True)
        if tied_bias is not None:
            assert_sum_exact(ref["dpre"] * (cf - tied_bias.to(F64)[:, None, :]), what + " tied dotpart", slots=True)
    assert_k_tiles_contribute(r, w, what)
    return ref
