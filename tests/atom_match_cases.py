"""Cases for the nearest-atom matching tests (not collected: no ``test_`` prefix).

The exact recipe: small-integer bf16 operands (``exact_gemm_cases.plain_pool("int")``), so every fp32
accumulation order gives the fp64 product and ``torch.equal`` against an fp64 reference is the only right
answer -- for the values AND for the columns, once the tie rule (lowest column among equal values) is part
of the reference.  Natural ties at a row's maximum are rare in these operands, so ties are planted: column
pairs at distances 1, 4, 16, 64 and 128 (inside a lane's registers, across the 16-lane groups of a row,
across wave tiles, across blocks) and at the last live column, each with a row of ``a`` that peaks at
exactly that pair; and a row that peaks at column 0, which the padded copies of ``b``'s first row tie with.
``test_atom_match_cpu.py`` asserts these properties without a GPU; ``test_atom_match_gpu.py`` compares the
kernels against the references below.
"""

from __future__ import annotations

import functools

import torch

import exact_gemm_cases as X

BF = torch.bfloat16
F64 = torch.float64

G, M, N, K = 2, 130, 257, 65
ALPHA = 0.5
# (j1, j2): b[:, j2] = b[:, j1]; distances 1, 4, 16, 64, 128 and the last live column
PLANTS = ((3, 4), (10, 14), (20, 36), (40, 104), (50, 178), (7, 256))
PLANT_ROWS = tuple(5 + 9 * r for r in range(len(PLANTS)))  # a[:, 5 + 9 r] = b[:, j1]
ZERO_ROW = 5 + 9 * len(PLANTS)                             # a[:, 59] = b[:, 0]: peaks at column 0


@functools.lru_cache(maxsize=None)
def exact_inputs():
    """(a [G, M, K], b [G, N, K]) bf16 on the CPU, with the planted ties."""
    a, b = (t.to(BF) for t in X.plain_pool("int"))
    a, b = a[:G, :M, :K].clone(), b[:G, :N, :K].clone()
    for r, (j1, j2) in zip(PLANT_ROWS, PLANTS):
        b[:, j2] = b[:, j1]
        a[:, r] = b[:, j1]
    a[:, ZERO_ROW] = b[:, 0]
    return a, b


def ref_sim(a, b, alpha=1.0):
    """alpha * A B^T in fp64; ``b`` [N, K] is shared by every model."""
    return X.ref_plain(a, b if b.dim() == 3 else b[None], alpha)


def ref_topm(sim, m, valid=None):
    """(values fp64, columns int32) [..., M, m]: value descending, then column ascending; (0.0, -1) where
    fewer than m valid columns exist."""
    from sparse_coding__amd.engine.atom_match import topm_reference

    return topm_reference(sim, m, valid)


def valid_mask(shape, live_cols=None, live_rows=None, exclude=None, exclude_self=False):
    """bool [G, M, N]: the (row, column) pairs that take part."""
    Gs, Ms, Ns = shape
    ok = torch.ones(Gs, Ms, Ns, dtype=torch.bool)
    cols, rows = torch.arange(Ns), torch.arange(Ms)
    if live_cols is not None:
        ok &= cols[None, None, :] < torch.as_tensor(live_cols)[:, None, None]
    if live_rows is not None:
        ok &= rows[None, :, None] < torch.as_tensor(live_rows)[:, None, None]
    if exclude_self:
        ok &= rows[:, None] != cols[None, :]
    if exclude is not None:
        for e in range(exclude.shape[-1]):
            col = exclude[..., e].long()
            hit = torch.zeros_like(ok).scatter_(2, col.clamp(min=0).unsqueeze(-1), (col >= 0).unsqueeze(-1))
            ok &= ~hit
    return ok


def tie_in_top(sim, k=4):
    """bool [..., M]: two of the row's k largest values are equal."""
    top = torch.sort(sim, dim=-1, descending=True).values[..., :k]
    return (top[..., 1:] == top[..., :-1]).any(-1)


# ------------------------------------------------------------------ unit-norm operands
UNIT_SHAPE = (3, 300, 517, 200)  # G, M, N, K


@functools.lru_cache(maxsize=None)
def unit_inputs(seed=7):
    Gu, Mu, Nu, Ku = UNIT_SHAPE
    gen = torch.Generator().manual_seed(seed)
    a = torch.nn.functional.normalize(torch.randn(Gu, Mu, Ku, generator=gen), dim=-1).to(BF)
    b = torch.nn.functional.normalize(torch.randn(Gu, Nu, Ku, generator=gen), dim=-1).to(BF)
    return a, b


def delta(a, b, k_padded):
    """The fp32 accumulation bound of <a_i, b_j> for bf16 operands: products of bf16 numbers are exact in
    fp32, a sum of K terms in any order errs by at most about K 2^-24 sum |a b| <= K 2^-24 |a_i| |b_j|; the
    factor 2 covers the MFMA's internal grouping and the multiplication by alpha.  [G, M, N] fp64."""
    na, nb = a.to(F64).norm(dim=-1), b.to(F64).norm(dim=-1)
    return k_padded * 2.0 ** -23 * na[..., :, None] * nb[..., None, :]


# ------------------------------------------------------------------ engines
ENG_G, ENG_B, ENG_N, ENG_D = 3, 128, 256, 256
ENG_SIZES = (128, 256, 256)
ENG_KS = (4, 16, 64)
ENG_SEED = 21


def separated_rows(dicts, dict_size, m=2):
    """bool [G, G, n]: rows whose reference top-(m + 1) values (fp64 products of ``dicts`` as given, the
    diagonal left out for g == h) are pairwise further apart than 2 delta -- there the kernel's fp32
    accumulation cannot reorder the first m matches."""
    from sparse_coding__amd.engine.atom_match import atom_matches_reference

    ref = atom_matches_reference(dicts, dict_size, m + 1, True)
    Gs, n, d = dicts.shape
    norms = dicts.to(F64).norm(dim=-1)
    dl = d * 2.0 ** -23 * norms[:, None, :, None] * norms.amax(-1)[None, :, None, None]  # [G, G, n, 1]
    v = ref.cos.to(F64)
    gaps = v[..., :-1] - v[..., 1:]
    full = (ref.idx >= 0).all(-1)
    return full & (gaps > 2 * dl).all(-1), ref
