"""Inputs shared by the sparse reconstruction tests (``test_sparse_recon_cpu.py`` checks the oracle and the
fixtures' own properties, ``test_sparse_recon_gpu.py`` runs the kernels on them).  Everything is built on the
CPU from fixed seeds.

**Planted.**  ``x`` holds integers in [-3, 3], every atom has two non-zero coordinates from {+-1/2, +-1} and
every code is 1/2, 1, 2 or 4, so every residual element is a multiple of 1/4 and every partial sum of squares
a multiple of 1/16.  With ``m_k = |x_k| + sum_e c_e |D[col_e, k]|``, ``16 sum_k m_k^2 < 2^24`` for every row
(``planted_is_exact`` checks it on the oracle's own ``sum m^2``): every intermediate of the kernels' fp32
arithmetic is then an exactly representable number whatever the order, so their outputs equal the fp64
oracle's bit for bit.  Rows have L in {0, 1, 2, 7, 8, 9, 63, 64, 65, 257, n} entries (J - 1, J, J + 1 for
J = 1, 8, 64; one, four and five chunks of 64 entries; the whole dictionary).  Only four code values exist, so
equal codes are everywhere; on top, every row with at least nine entries carries the row's largest code, 4,
on the columns ``TIES`` = (5, 6, 68, 69, 261, n - 1): column distances 1, 63, 64 and 256 and the last live
column, which rank order must take in ascending column order before anything else.

**Random.**  Unit-norm atoms rounded to bf16, L about Poisson(24) plus a few rows of 100 - 300 entries,
bf16-valued codes and shared rows ``x = bf16(model 0's sum c D + noise)``, so that model 0's residual shrinks
along the curve while the other models' grows.
"""

import torch

PLANTED_G, PLANTED_N, PLANTED_ROWS = 2, 320, 64
PLANTED_L = (0, 1, 2, 7, 8, 9, 63, 64, 65, 257, PLANTED_N)
PLANTED_J = (0, 1, 8, 64)
DS = (64, 512, 768, 1024)
TIES = (5, 6, 68, 69, 261, PLANTED_N - 1)

RANDOM_G, RANDOM_N, RANDOM_ROWS = 3, 512, 256
U = 2.0 ** -24


def planted(d, seed=0):
    """(D bf16 [G, n, d], dense codes fp32 [G, N, n], x bf16 [G, N, d], keep bool [G, n])."""
    G, n, N = PLANTED_G, PLANTED_N, PLANTED_ROWS
    gen = torch.Generator().manual_seed(100 * seed + d)
    D = torch.zeros(G, n, d)
    vals = torch.tensor([-1.0, -0.5, 0.5, 1.0])
    for g in range(G):
        for f in range(n):
            at = torch.randperm(d, generator=gen)[:2]
            D[g, f, at] = vals[torch.randint(0, 4, (2,), generator=gen)]
    codes = torch.zeros(G, N, n)
    for g in range(G):
        for r in range(N):
            L = PLANTED_L[(r + g) % len(PLANTED_L)]
            cols = torch.randperm(n, generator=gen)[:L]
            codes[g, r, cols] = 2.0 ** torch.randint(-1, 2, (L,), generator=gen).float()
            if L >= 9:  # the planted ties (on top of, or instead of, some of the random columns)
                have = int((codes[g, r] > 0).sum())
                codes[g, r, list(TIES)] = 4.0
                extra = int((codes[g, r] > 0).sum()) - have
                if extra:  # keep the row's length: drop as many of its other columns
                    other = [c for c in torch.nonzero(codes[g, r]).flatten().tolist() if c not in TIES]
                    codes[g, r, other[:extra]] = 0.0
            assert int((codes[g, r] > 0).sum()) == L
    x = torch.randint(-3, 4, (G, N, d), generator=gen).to(torch.bfloat16)
    keep = torch.rand(G, n, generator=gen) < 0.5
    keep[:, TIES[0]], keep[:, TIES[1]], keep[:, n - 1] = True, False, True
    return D.to(torch.bfloat16), codes, x, keep


def planted_is_exact(ref):
    """The sufficient condition of the module docstring, on the oracle's own sums (``SparseRecon``)."""
    return float(max(ref.curve_mm.max(), ref.split_mm.max())) * 16 < 2 ** 24


def random_case(d, seed=0):
    """(D bf16 [G, n, d], dense codes fp32 [G, N, n], x bf16 [N, d], keep bool [G, n])."""
    G, n, N = RANDOM_G, RANDOM_N, RANDOM_ROWS
    gen = torch.Generator().manual_seed(300 * seed + d)
    D = torch.nn.functional.normalize(torch.randn(G, n, d, generator=gen), dim=-1).to(torch.bfloat16)
    lens = torch.poisson(torch.full((G, N), 24.0), generator=gen).long().clamp(0, n)
    lens[:, 3], lens[:, 77], lens[:, 200], lens[:, 255] = 100, 300, 191, 257
    lens[:, 0] = 0
    codes = torch.zeros(G, N, n)
    for g in range(G):
        for r in range(N):
            L = int(lens[g, r])
            cols = torch.randperm(n, generator=gen)[:L]
            codes[g, r, cols] = (torch.rand(L, generator=gen) * 4 + 0.01).to(torch.bfloat16).float()
    x = (torch.einsum("gbn,gnd->gbd", codes, D.float())[0] + 0.3 * torch.randn(N, d, generator=gen))
    keep = torch.rand(G, n, generator=gen) < 0.3
    return D, codes, x.to(torch.bfloat16), keep


def value_bound(value, rm, mm, cnt, d):
    """Bound on |kernel - oracle| of one squared norm, in fp64 from the oracle's quantities: ``2 u j sum_k |r_k|
    m_k + u^2 j^2 sum_k m_k^2 + (d / 64 + 8) u S`` with u = 2^-24, j the atoms subtracted (every fma leaves an
    element within ``u m_k`` of exact, so after j of them ``|dr_k| <= j u m_k`` and ``|d(r_k^2)| <= 2 |r_k| j u
    m_k + (j u m_k)^2``) and S the value (d / 64 per-lane adds, six butterfly adds and the roundings of the
    products)."""
    j = cnt.double()
    return 2 * U * j * rm + U * U * j * j * mm + (d / 64 + 8) * U * value


def brute_force(codes, D, x, J, keep=None):
    """Dense route: (curve [G, N, J + 1], split [G, N, 3]) in fp64 from dense codes [G, N, n] -- ``torch.topk``
    on a key that makes the tie rule explicit (code descending, then column ascending), masks and matmul."""
    G, N, n = codes.shape
    c, Dd = codes.double(), D.double()
    xd = x.double() if x.dim() == 3 else x.double().expand(G, *x.shape)
    # codes are bf16-valued: c 2^20 keeps them apart by far more than the column term, which breaks ties
    key = torch.where(c > 0, c * 2.0 ** 20 - torch.arange(n).double() / (2 * n), torch.full_like(c, -1.0))
    curve = torch.zeros(G, N, J + 1, dtype=torch.float64)
    for j in range(J + 1):
        sel = torch.zeros_like(c, dtype=torch.bool)
        if j:
            top = torch.topk(key, min(j, n), dim=-1)
            sel.scatter_(-1, top.indices, top.values > 0)
        curve[:, :, j] = (xd - (c * sel) @ Dd).pow(2).sum(-1)
    split = torch.zeros(G, N, 3, dtype=torch.float64)
    split[:, :, 0] = (xd - c @ Dd).pow(2).sum(-1)
    if keep is not None:
        k = keep.unsqueeze(1)
        split[:, :, 1] = (xd - (c * k) @ Dd).pow(2).sum(-1)
        split[:, :, 2] = (xd - (c * ~k) @ Dd).pow(2).sum(-1)
    return curve, split
