"""Inputs shared by the CPU and GPU suites of the attribution kernels (``engine/attribution.py``,
``csrc/attribution.hip``).  Everything is built on the CPU from fixed seeds, and every oracle result is computed
once per case.

- ``planted(d, n)``: rows on which every fp32 operation of the kernels is exact -- integer ``x`` in [-4, 4], atoms
  with four non-zeros in {+-1/2, +-1}, codes in {1/2, 1, 2}.  Every intermediate is a multiple of 2^-4 far below
  2^20, so ``proj``, ``sse_row`` and all raw sums are the same in any order and compare with ``torch.equal``.
  Rows of 0, 1, 2, 63, 64, 65, 129, 257 and n entries (those that fit the model); with n = 96 model 0 is masked to
  70 live features.
- ``random_rows()``: G = 2, B = 128, n = 256, d = 512, about 16 entries per row, bf16 data: for the error bound.
- ``lists()``: codes, a hand-made ``proj`` and ``q`` for the list walk alone: lists of 0 / 1 / 63 / 64 / 65 / 129
  entries, one on every row, and three features whose ``c p`` terms are 2^53, 1, 1 at chosen list positions.
"""

import functools

import torch

from sparse_coding__amd.engine import attribution as at
from sparse_coding__amd.engine.feature_codes import feature_codes_reference
from sparse_coding__amd.engine.sparse_codes import SparseCodes, sparse_codes_reference

G = 2
PLANTED = [(64, 320), (512, 96), (768, 320), (1024, 96), (512, 320)]     # (d, n)
PLANTED_IDS = ["d%d-n%d" % c for c in PLANTED]
ROW_LENS = (0, 1, 2, 63, 64, 65, 129, 257)
N_PLANTED = 16
ROW0 = 5      # the row window of the window tests starts here


def live_of(n):
    return [70, n] if n == 96 else [n, n]


@functools.lru_cache(maxsize=None)
def planted(d, n):
    """dict(sc, D bf16 [G, n, d], x bf16 [G, N, d] (``x[0]`` doubles as the shared rows), live, lens)."""
    gen = torch.Generator().manual_seed(1000 + d + n)
    live = live_of(n)
    D = torch.zeros(G, n, d)
    where = torch.randint(0, d, (G, n, 4), generator=gen)
    what = torch.tensor([-1.0, -0.5, 0.5, 1.0])[torch.randint(0, 4, (G, n, 4), generator=gen)]
    D.scatter_(2, where, what)
    lens = [L for L in ROW_LENS if L <= n] + [n]
    lens = lens + torch.randint(3, 20, (N_PLANTED - len(lens),), generator=gen).tolist()
    dense = torch.zeros(G, N_PLANTED, n)
    for g in range(G):
        for r, L in enumerate(lens):
            cols = torch.randperm(live[g], generator=gen)[:min(L, live[g])]
            dense[g, r, cols] = 2.0 ** torch.randint(-1, 2, (cols.numel(),), generator=gen).float()
    x = torch.randint(-4, 5, (G, N_PLANTED, d), generator=gen).float()
    return dict(sc=sparse_codes_reference([dense]), D=D.to(torch.bfloat16), x=x.to(torch.bfloat16), live=live,
                lens=lens, dense=dense)


@functools.lru_cache(maxsize=None)
def planted_reference(d, n, shared=False):
    """The oracle's ``Attribution`` (with ``proj``) and ``ResidualProj`` of a planted case."""
    k = planted(d, n)
    x = k["x"][0] if shared else k["x"]
    ref = at.attribution_reference(k["sc"], k["D"], x, k["live"], return_proj=True)
    return ref, at.residual_proj_reference(k["sc"], k["D"], x, k["live"])


RAW = ("cnt", "A", "P1", "C2", "n_harm", "min_delta", "max_delta")


def same(got, want, fields=RAW + ("q", "skipped", "missing")):
    """Every raw field of two ``Attribution`` bit for bit."""
    assert got.n_rows == want.n_rows
    for f in fields:
        a, b = getattr(got, f).cpu(), getattr(want, f).cpu()
        assert a.dtype == b.dtype and torch.equal(a, b), f


# ---------------------------------------------------------------------------- random rows
RANDOM = dict(G=2, B=128, n=256, d=512, L0=16)


@functools.lru_cache(maxsize=None)
def random_rows():
    s = RANDOM
    gen = torch.Generator().manual_seed(77)
    D = torch.nn.functional.normalize(torch.randn(s["G"], s["n"], s["d"], generator=gen), dim=-1).to(torch.bfloat16)
    mask = torch.rand(s["G"], s["B"], s["n"], generator=gen) < s["L0"] / s["n"]
    codes = torch.where(mask, (0.25 + torch.rand(mask.shape, generator=gen)).to(torch.bfloat16).float(),
                        torch.zeros(()))
    x = torch.einsum("gbn,gnd->gbd", codes, D.float()) + 0.3 * torch.randn(s["G"], s["B"], s["d"], generator=gen)
    sc = sparse_codes_reference([codes])
    x = x.to(torch.bfloat16)
    return dict(sc=sc, D=D, x=x, ref=at.residual_proj_reference(sc, D, x))


# ---------------------------------------------------------------------------- the list walk alone
LIST_N, LIST_ROWS = 40, 160
(F_EMPTY, F_ONE, F_63, F_64, F_65, F_129, F_EVERY, F_ORDER_LANE0, F_ORDER_012, F_ORDER_MIX) = range(10)
BIG = 2.0 ** 53
# c p terms of 2^53, 1, 1.  At list positions 0, 64, 128 they all meet in lane 0: (2^53 + 1) + 1 = 2^53 (2^53 + 1
# rounds back to even, twice).  At positions 0, 1, 2 they sit in lanes 0, 1, 2 and lane 3 holds 0: the xor-1 step
# gives 2^53 + 1 = 2^53 and 1 + 0 = 1, the xor-2 step 2^53 + 1 = 2^53.  Both equal the sequential sum.  At
# positions 0, 1, 65 lane 1 adds 1 + 1 = 2 before the butterfly: 2^53 + 2, which a sequential sum never reaches.
ORDER_LANE0 = 9007199254740992.0
ORDER_012 = 9007199254740992.0
ORDER_MIX = 9007199254740994.0
SEQUENTIAL = (BIG + 1.0) + 1.0
assert SEQUENTIAL == ORDER_LANE0 == ORDER_012 and BIG + (1.0 + 1.0) == ORDER_MIX != SEQUENTIAL
ORDER_TERMS = {F_ORDER_LANE0: (0, 64, 128), F_ORDER_012: (0, 1, 2), F_ORDER_MIX: (0, 1, 65)}


def entry_values(sc: SparseCodes, dense_values: torch.Tensor) -> torch.Tensor:
    """fp32 [G, cap]: ``dense_values[g, row, col]`` at the position of every stored entry."""
    out = torch.zeros(sc.n_models, sc.cap)
    for g in range(sc.n_models):
        k = int(sc.row_ptr[g, -1])
        out[g, :k] = dense_values[g, sc.entry_rows(g), sc.col[g, :k].long()]
    return out


@functools.lru_cache(maxsize=None)
def lists():
    """dict(sc, fc, proj fp32 [G, cap], q fp32 [G, n], want): the list walk's inputs and the oracle's outputs."""
    gen = torch.Generator().manual_seed(31)
    N, n = LIST_ROWS, LIST_N
    mask = torch.rand(G, N, n, generator=gen) < 0.1
    mask[:, :, :10] = False
    mask[:, N // 3, F_ONE] = True
    for f, k in ((F_63, 63), (F_64, 64), (F_65, 65), (F_129, 129)):
        for g in range(G):
            mask[g, torch.randperm(N, generator=gen)[:k], f] = True
    mask[:, :, F_EVERY] = True
    for f in ORDER_TERMS:
        mask[:, :129, f] = True       # rows 0 .. 128: list position i is row i
    codes = torch.where(mask, (0.25 + torch.rand(mask.shape, generator=gen)).to(torch.bfloat16).float(),
                        torch.zeros(()))
    pd = torch.randn(G, N, n, generator=gen)
    for f, at_pos in ORDER_TERMS.items():
        codes[:, :129, f] = 1.0
        pd[:, :, f] = 0.0
        for p, v in zip(at_pos, (BIG, 1.0, 1.0)):
            pd[:, p, f] = v
    sc = sparse_codes_reference([codes])
    fc = feature_codes_reference(sc)
    proj = entry_values(sc, pd)
    q = (0.5 + torch.rand(G, n, generator=gen)).float()
    return dict(sc=sc, fc=fc, proj=proj, q=q, want=at.attr_list_sums_reference(fc, sc, proj, q))
