"""Case builders shared by ``test_value_order_cpu.py`` and ``test_value_order_gpu.py``: the smallest feature-major
lists at which a segmented sort and a tie-aware rank walk can still go wrong, and the comparators.

``lists(N, n, kind)`` builds the lists of G = 2 models directly (``col_ptr`` int64 [G, n + 1], ``row`` int32 /
``val`` fp32 [G, cap], rows ascending and distinct in a list, a zero tail behind them):

- model 0 holds lists of 0, 1, 2, 63, 64, 65, 127, 128, 129 and 1000 entries (as many as fit N) in that order,
  then short ones; model 1 is filled differently: random lengths up to 200, a list of exactly 200 entries and,
  at ``F_ALL``, a list of all N rows;
- the values of ``kind``: "bf16" (the two low digits of the key constant), "fp32" (random mantissas: four
  passes), "equal" (no pass: rows must stay ascending), "three" (3 distinct values: tie runs cross the 64-entry
  chunks), "lowbit" (neighbours in the lowest bit), "denormal", and for the sort alone "signed" (negative values,
  -0.0, +0.0 and positive ones).
"""

import torch

from sparse_coding__amd.engine.feature_codes import FeatureCodes

G = 2
LENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000)
F_ALL, F_200 = 3, 5                       # model 1: the list of all N rows, the list of exactly 200 entries
POSITIVE = ("bf16", "fp32", "equal", "three", "lowbit", "denormal")
KINDS = POSITIVE + ("signed",)
TAIL = 37                                 # unused positions behind the fuller model's lists
SHAPES = ((1024, 70), (512, 70), (256, 1))


def lengths(N, n):
    """Entries per list, two Python lists of n."""
    gen = torch.Generator().manual_seed(1000 * N + n)
    a = [min(x, N) for x in LENS][:n]
    a += torch.randint(0, 6, (n - len(a),), generator=gen).tolist()
    b = torch.randint(0, min(N, 200) + 1, (n,), generator=gen).tolist()
    if n > F_200:
        b[F_ALL], b[F_200] = N, min(N, 200)
    else:
        b[0] = N
    return a, b


def values(kind, count, gen):
    if kind == "bf16":
        return (torch.rand(count, generator=gen) * 4 + 0.01).to(torch.bfloat16).float()
    if kind == "fp32":
        return torch.rand(count, generator=gen) * 300 + 1e-3
    if kind == "equal":
        return torch.full((count,), 1.5)
    if kind == "three":
        return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (count,), generator=gen)]
    if kind == "lowbit":
        return (0x3F800000 + torch.randint(0, 4, (count,), generator=gen)).to(torch.int32).view(torch.float32)
    if kind == "denormal":
        bits = torch.randint(1, 2 ** 23, (count,), generator=gen)
        bits[::5] += 2 ** 23                                      # a few of the smallest normal numbers among them
        return bits.to(torch.int32).view(torch.float32)
    if kind == "signed":
        v = torch.randn(count, generator=gen)
        v[::4] = 0.0
        v[1::8] = -0.0
        v[2::16] = v[2::16].to(torch.bfloat16).float()
        return v
    raise ValueError(kind)


_CACHE = {}


def lists(N=1024, n=70, kind="bf16") -> FeatureCodes:
    """The crafted lists as a ``FeatureCodes`` over N rows (cached: treat as read-only)."""
    if (N, n, kind) in _CACHE:
        return _CACHE[(N, n, kind)]
    lens = lengths(N, n)
    cap = max(sum(ln) for ln in lens) + TAIL
    gen = torch.Generator().manual_seed(7 + KINDS.index(kind))
    col_ptr = torch.zeros(G, n + 1, dtype=torch.int64)
    row = torch.zeros(G, cap, dtype=torch.int32)
    val = torch.zeros(G, cap, dtype=torch.float32)
    for g in range(G):
        col_ptr[g, 1:] = torch.cumsum(torch.tensor(lens[g]), 0)
        for f, ln in enumerate(lens[g]):
            lo = int(col_ptr[g, f])
            row[g, lo:lo + ln] = torch.randperm(N, generator=gen)[:ln].sort().values.to(torch.int32)
            val[g, lo:lo + ln] = values(kind, ln, gen)
    fc = FeatureCodes(N, n, col_ptr, row, val, torch.zeros(G, dtype=torch.int64))
    _CACHE[(N, n, kind)] = fc
    return fc


def dense(fc) -> torch.Tensor:
    """fp32 [G, N, n]: the dense codes the lists came from (0 where a feature does not fire)."""
    out = torch.zeros(fc.n_models, fc.n_rows, fc.n)
    ptr = fc.host_ptr()
    for g in range(fc.n_models):
        for f in range(fc.n):
            lo, hi = ptr[g][f], ptr[g][f + 1]
            out[g, fc.row[g, lo:hi].long(), f] = fc.val[g, lo:hi]
    return out


def flags(N, K, seed=0) -> torch.Tensor:
    """int32 words [N] of K concepts with different base rates.  K >= 3: concept 1 has no positive and concept 2
    only positives; K = 32: bit 31 is a concept like the others."""
    gen = torch.Generator().manual_seed(31 * K + seed)
    rate = torch.linspace(0.05, 0.6, K)
    bits = torch.rand(N, K, generator=gen) < rate
    if K >= 3:
        bits[:, 1], bits[:, 2] = False, True
    from sparse_coding__amd.engine.value_order import concept_words

    return concept_words(bits)


def guard_pointers(fc):
    """``col_ptr`` with pointers past ``cap``, negative and non-monotone ones (n = 70 lists)."""
    cp = fc.col_ptr.clone()
    cp[0, 40] = cp[0, 39] - 3          # list 39 ends before it starts
    cp[0, 12] = cp[0, 9] + 5           # a pointer that jumps back into the 1000-entry list
    cp[1, 0] = -5
    cp[1, -1] = fc.cap + 1000
    cp[1, 20] = fc.cap + 9             # past the buffers in the middle: what follows is clipped to nothing
    return cp


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def same_lists(got, want):
    """(rows, values) of two sorts: the same integers and the same fp32 bit patterns (-0.0 is not +0.0)."""
    assert torch.equal(got[0].cpu(), want[0].cpu()), "rows differ"
    assert torch.equal(bits(got[1].cpu()), bits(want[1].cpu())), "values differ"


def same_auroc(got, want):
    """Two ``FeatureAuroc``: identical integers, and the fp64 AUROC they give (NaN where a concept has no positive
    or no negative, on both sides)."""
    got, want = got.to("cpu"), want.to("cpu")
    assert got.n_rows == want.n_rows
    for k in ("u2", "pos_in", "cnt", "n_pos"):
        a, b = getattr(got, k), getattr(want, k)
        assert a.dtype == b.dtype and torch.equal(a, b), k
    a, b = got.auroc(), want.auroc()
    assert a.dtype == torch.float64 and torch.equal(a.isnan(), b.isnan())
    assert torch.equal(a.nan_to_num(nan=-1.0), b.nan_to_num(nan=-1.0))
