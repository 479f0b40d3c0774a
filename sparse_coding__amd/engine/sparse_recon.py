"""Truncated and ablated reconstruction error of an ensemble from its sparse codes: the result type, the
fp64 torch oracle and the device route.

Per model g and row r: ``x`` is the row as the decoder sees it (bf16: what ``prepare()`` returns), the row's
CSR entries are ``(col_e, c_e)`` with ``c_e > 0``, ``D[g]`` is the unit-norm dictionary (the bf16 shadow on the
device route), and the reconstruction from an entry set S is ``sum_{e in S} c_e D[g, col_e]``.

- **Curve.**  Entries in *rank order* -- code descending, then column ascending -- and ``prefix_j`` the first
  ``min(j, L)`` of them: ``sse_prefix[g, j] = sum_rows |x - recon(prefix_j)|^2`` for j = 0 .. J.  j = 0 is
  ``sum |x|^2``; a row with L <= j contributes its final value.
- **Split.**  ``sse_full`` from all entries, and with a per-feature keep mask ``sse_keep`` from the entries
  with ``keep[g, col_e]`` and ``sse_rest`` from the others, each in the CSR's ascending column order.
- **FVU.**  Every sum divided by the total sum of squares about the mean of the same rows, from ``s1`` /
  ``s2`` in fp64 as ``evaluate()`` computes them.
- **Skip rule.**  That of ``ops.interference.active_capacity``: a row is left out whole, reads zeros and is
  counted in ``skipped[g]`` unless ``0 <= row_ptr[r] <= row_ptr[r + 1] <= cap``, ``L <= n`` and every column
  lies in ``[0, lim)``, lim = n or ``min(n, nactive[g])``.

``ops.sparse_recon.recon_curve`` / ``recon_split`` (``csrc/sparse_recon.hip``) compute the per-row values in
fp32 on the device; ``sparse_recon_reference`` computes them in fp64 torch (CPU included) and is what the
tests compare against.  Per batch the per-row values are summed with ``sum(1, dtype=float64)`` and added to
fp64 accumulators, so a pool fed in chunks of whole batches through ``state=`` gives the bits of one call.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, NamedTuple, Optional

import torch

from .interference import live_counts
from .sparse_codes import SparseCodes

MAX_KEPT = 64   # largest J of a curve


class ReconSkipped(RuntimeError):
    """Rows were left out of a ``ReconProfile``: their entries were not all stored, or not valid."""


def _div(a, b):
    return a / b.unsqueeze(-1) if a.dim() == 2 else a / b


@dataclass
class ReconProfile:
    """Raw sums of squared reconstruction errors over ``n_rows`` rows for G models and a curve of J + 1 points."""

    n_rows: int
    sse_prefix: torch.Tensor            # fp64 [G, J + 1]  sum over rows of |x - recon(prefix_j)|^2
    sse_full: torch.Tensor              # fp64 [G]         all entries, ascending column order
    sse_keep: Optional[torch.Tensor]    # fp64 [G] or None the entries of the kept features
    sse_rest: Optional[torch.Tensor]    # fp64 [G] or None the other entries
    rows_within: torch.Tensor           # int64 [G, J + 1] rows with at most j entries
    s1: torch.Tensor                    # fp64 [G, d]      sum of the rows
    s2: torch.Tensor                    # fp64 [G]         sum of their squares
    skipped: torch.Tensor               # int64 [G]        rows left out (entries not all stored, or invalid)

    @property
    def max_kept(self) -> int:
        return int(self.sse_prefix.shape[1]) - 1

    @property
    def variance(self) -> torch.Tensor:
        """fp64 [G]: total sum of squares about the mean of the rows."""
        return self.s2 - self.s1.pow(2).sum(-1) / self.n_rows

    @property
    def fvu_prefix(self) -> torch.Tensor:
        """fp64 [G, J + 1]: FVU when only the j largest codes of every row are kept."""
        return _div(self.sse_prefix, self.variance)

    @property
    def fvu_full(self) -> torch.Tensor:
        return self.sse_full / self.variance

    @property
    def fvu_keep(self) -> Optional[torch.Tensor]:
        return None if self.sse_keep is None else self.sse_keep / self.variance

    @property
    def fvu_rest(self) -> Optional[torch.Tensor]:
        return None if self.sse_rest is None else self.sse_rest / self.variance

    @property
    def kept_fraction(self) -> torch.Tensor:
        """fp64 [G, J + 1]: fraction of the rows whose whole reconstruction fits in j entries."""
        return self.rows_within.double() / self.n_rows

    def check(self) -> "ReconProfile":
        """Synchronises; raises ``ReconSkipped`` if any row was left out (the sums would cover fewer rows
        than the variance)."""
        sk = self.skipped.cpu()
        if bool((sk != 0).any()):
            raise ReconSkipped(f"{sk.tolist()} rows per model were skipped (of {self.n_rows}): their sparse codes "
                               "were not all stored -- encode with a larger budget, or budget=None")
        return self

    def merge(self, other: "ReconProfile") -> "ReconProfile":
        """The sums over the rows of both (same ensemble, same dictionaries, same keep mask)."""
        check_state(other, self.sse_prefix.shape[0], self.max_kept, self.sse_keep is not None, self.s1.shape[1])
        dev = self.sse_prefix.device
        add = lambda a, b: None if a is None else a + b.to(dev)
        return ReconProfile(self.n_rows + other.n_rows, add(self.sse_prefix, other.sse_prefix),
                            add(self.sse_full, other.sse_full), add(self.sse_keep, other.sse_keep),
                            add(self.sse_rest, other.sse_rest), add(self.rows_within, other.rows_within),
                            add(self.s1, other.s1), add(self.s2, other.s2), add(self.skipped, other.skipped))

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        sd = {"n_rows": torch.tensor(int(self.n_rows), dtype=torch.int64), "sse_prefix": self.sse_prefix,
              "sse_full": self.sse_full, "rows_within": self.rows_within, "s1": self.s1, "s2": self.s2,
              "skipped": self.skipped}
        if self.sse_keep is not None:
            sd.update(sse_keep=self.sse_keep, sse_rest=self.sse_rest)
        return sd

    def save(self, path):
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, map_location="cpu") -> "ReconProfile":
        sd = torch.load(path, map_location=map_location, weights_only=True)
        return cls(int(sd["n_rows"]), sd["sse_prefix"], sd["sse_full"], sd.get("sse_keep"), sd.get("sse_rest"),
                   sd["rows_within"], sd["s1"], sd["s2"], sd["skipped"])

    def to(self, device) -> "ReconProfile":
        mv = lambda t: None if t is None else t.to(device)
        return ReconProfile(self.n_rows, mv(self.sse_prefix), mv(self.sse_full), mv(self.sse_keep), mv(self.sse_rest),
                            mv(self.rows_within), mv(self.s1), mv(self.s2), mv(self.skipped))


def check_max_kept(max_kept) -> int:
    if isinstance(max_kept, bool) or int(max_kept) != max_kept or not 0 <= int(max_kept) <= MAX_KEPT:
        raise ValueError(f"max_kept must be an integer in 0..{MAX_KEPT}, got {max_kept!r}")
    return int(max_kept)


def check_state(state, G: int, J: int, keep: bool, d: Optional[int] = None):
    """Validate the ``state`` argument of a ``recon_profile`` call (the result of an earlier call)."""
    if not isinstance(state, ReconProfile):
        raise ValueError("state must be the ReconProfile of an earlier call")
    if tuple(state.sse_prefix.shape) != (G, J + 1) or tuple(state.sse_full.shape) != (G,) \
            or tuple(state.skipped.shape) != (G,) or (d is not None and tuple(state.s1.shape) != (G, d)):
        raise ValueError(f"state is for another ensemble or curve (sse_prefix {tuple(state.sse_prefix.shape)}, "
                         f"this one [{G}, {J + 1}])")
    if (state.sse_keep is not None) != keep:
        raise ValueError("state and this call must both have a keep mask, or neither")


# ---------------------------------------------------------------------- keep masks
def keep_words(mask: torch.Tensor) -> torch.Tensor:
    """Pack the per-feature keep mask ``mask`` (bool [G, n]) into uint32 words [G, ceil(n / 32)]: feature f
    is bit ``f & 31`` of word ``f >> 5``; the spare bits of the last word are 0."""
    if mask.dim() != 2 or mask.dtype != torch.bool:
        raise ValueError(f"the keep mask must be bool [G, n], got {mask.dtype} {tuple(mask.shape)}")
    G, n = mask.shape
    words = (n + 31) // 32
    bits = torch.zeros(G, words * 32, dtype=torch.int64, device=mask.device)
    bits[:, :n] = mask
    packed = (bits.view(G, words, 32) << torch.arange(32, device=mask.device)).sum(-1)
    packed = torch.where(packed >= 2 ** 31, packed - 2 ** 32, packed)  # the same 32 bits as a signed word
    return packed.to(torch.int32).view(torch.uint32).contiguous()


def keep_mask(words: torch.Tensor, n: int) -> torch.Tensor:
    """The bool [G, n] mask that ``keep_words`` packed."""
    w = words.view(torch.int32).to(torch.int64) if words.dtype == torch.uint32 else words.to(torch.int64)
    bits = (w.unsqueeze(-1) >> torch.arange(32, device=words.device)) & 1
    return bits.reshape(words.shape[0], -1)[:, :n].bool()


def _as_mask(keep, G: int, n: int) -> Optional[torch.Tensor]:
    """``keep`` (None, a bool [G, n] mask or packed words) as a bool mask."""
    if keep is None:
        return None
    if keep.dtype == torch.bool:
        if tuple(keep.shape) != (G, n):
            raise ValueError(f"the keep mask must be bool [{G}, {n}], got {tuple(keep.shape)}")
        return keep
    if keep.dtype not in (torch.uint32, torch.int32) or tuple(keep.shape) != (G, (n + 31) // 32):
        raise ValueError(f"keep words must be uint32 [{G}, {(n + 31) // 32}], got {keep.dtype} {tuple(keep.shape)}")
    return keep_mask(keep, n)


def _as_words(keep, G: int, n: int, device) -> Optional[torch.Tensor]:
    if keep is None:
        return None
    if keep.dtype == torch.bool:
        return keep_words(_as_mask(keep, G, n)).to(device)
    _as_mask(keep, G, n)  # (the shape check)
    return keep.to(device).contiguous()


# ---------------------------------------------------------------------- the fp64 oracle
class SparseRecon(NamedTuple):
    """What ``sparse_recon_reference`` returns.  ``*_rm`` / ``*_mm`` / ``*_cnt`` feed the tests' error bound:
    per value, ``sum_k |r_k| m_k`` and ``sum_k m_k^2`` with r the residual and ``m_k = |x_k| + sum_e c_e
    |D[col_e, k]|`` over the entries subtracted for that value, and the number of those entries."""

    curve: torch.Tensor       # fp64 [G, n_rows, J + 1]
    split: torch.Tensor       # fp64 [G, n_rows, 3]   full, keep, rest (the last two 0 without a mask)
    skipped: torch.Tensor     # int64 [G]
    curve_rm: torch.Tensor    # fp64 [G, n_rows, J + 1]
    curve_mm: torch.Tensor    # fp64 [G, n_rows, J + 1]
    curve_cnt: torch.Tensor   # int64 [G, n_rows, J + 1]
    split_rm: torch.Tensor    # fp64 [G, n_rows, 3]
    split_mm: torch.Tensor    # fp64 [G, n_rows, 3]
    split_cnt: torch.Tensor   # int64 [G, n_rows, 3]


def rank_order(col: torch.Tensor, val: torch.Tensor) -> torch.Tensor:
    """Positions of a row's entries in rank order: code descending, then column ascending."""
    by_col = torch.argsort(col, stable=True)
    return by_col[torch.argsort(val[by_col], descending=True, stable=True)]


def sparse_recon_reference(sparse_codes: SparseCodes, D: torch.Tensor, x: torch.Tensor, max_kept: int = 32,
                           keep=None, nactive=None, row0: int = 0, n_rows: Optional[int] = None) -> SparseRecon:
    """fp64 torch oracle of ``ops.sparse_recon.recon_curve`` / ``recon_split`` on the rows ``row0 .. row0 +
    n_rows - 1`` (default: all) of ``sparse_codes`` against the dictionaries ``D`` [G, n, d] and the rows ``x``
    ([n_rows, d] shared or [G, n_rows, d]: the window's rows), values read as they are (bf16 included) in
    fp64.  Same definitions, rank rule (code descending, then column ascending) and skip rule as the kernels;
    ``keep``: bool [G, n] or the packed words of ``keep_words``."""
    sc = sparse_codes
    G, n, cap = sc.n_models, sc.n, sc.cap
    J = check_max_kept(max_kept)
    if D.dim() != 3 or D.shape[0] != G or D.shape[1] != n:
        raise ValueError(f"D must be [{G}, {n}, d], got {tuple(D.shape)}")
    d = D.shape[2]
    n_rows = sc.n_rows - row0 if n_rows is None else int(n_rows)
    if row0 < 0 or n_rows < 0 or row0 + n_rows > sc.n_rows:
        raise ValueError(f"rows [{row0}, {row0 + n_rows}) outside [0, {sc.n_rows}]")
    if x.dim() not in (2, 3) or x.shape[-1] != d or x.shape[-2] != n_rows or (x.dim() == 3 and x.shape[0] != G):
        raise ValueError(f"x must be [{n_rows}, {d}] or [{G}, {n_rows}, {d}], got {tuple(x.shape)}")
    dev = D.device
    Dd, xd = D.double(), x.to(dev).double()
    mask = _as_mask(keep, G, n)
    mask = None if mask is None else mask.to(dev)
    lim = [n] * G
    if nactive is not None:
        lim = [min(n, max(0, int(v))) for v in torch.as_tensor(nactive).reshape(-1).tolist()]
        if len(lim) == 1:
            lim = lim * G
    f64 = dict(dtype=torch.float64, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)
    curve, curve_rm, curve_mm = (torch.zeros(G, n_rows, J + 1, **f64) for _ in range(3))
    split, split_rm, split_mm = (torch.zeros(G, n_rows, 3, **f64) for _ in range(3))
    curve_cnt, split_cnt = torch.zeros(G, n_rows, J + 1, **i64), torch.zeros(G, n_rows, 3, **i64)
    skipped = torch.zeros(G, **i64)
    ptr = sc.row_ptr.to(dev).tolist()
    steps = torch.arange(J + 1, device=dev)

    def one(xr, A, c):
        """(|r|^2, sum |r| m, sum m^2) after subtracting the atoms A [L, d] with codes c [L] from xr."""
        r = xr - (c.unsqueeze(1) * A).sum(0)
        m = xr.abs() + (c.unsqueeze(1) * A.abs()).sum(0)
        return (r * r).sum(), (r.abs() * m).sum(), (m * m).sum()

    for g in range(G):
        colg, valg = sc.col[g].to(dev).long(), sc.val[g].to(dev).double()
        for r in range(n_rows):
            lo, hi = ptr[g][row0 + r], ptr[g][row0 + r + 1]
            if lo < 0 or hi < lo or hi > cap or hi - lo > n:
                skipped[g] += 1
                continue
            j, c = colg[lo:hi], valg[lo:hi]
            if bool(((j < 0) | (j >= lim[g])).any()):
                skipped[g] += 1
                continue
            xr = xd[g, r] if xd.dim() == 3 else xd[r]
            L = hi - lo
            # ---- the curve: prefix sums over the first min(J, L) entries in rank order
            order = rank_order(j, c)[:J]
            A, cs = Dd[g, j[order]], c[order]
            T = int(order.numel())
            zero = torch.zeros(1, d, **f64)
            res = xr - torch.cat([zero, torch.cumsum(cs.unsqueeze(1) * A, 0)])            # [T + 1, d]
            mag = xr.abs() + torch.cat([zero, torch.cumsum(cs.unsqueeze(1) * A.abs(), 0)])
            at = steps.clamp(max=T)
            curve[g, r] = (res * res).sum(1)[at]
            curve_rm[g, r] = (res.abs() * mag).sum(1)[at]
            curve_mm[g, r] = (mag * mag).sum(1)[at]
            curve_cnt[g, r] = at
            # ---- the split, in the CSR's order
            Af = Dd[g, j]
            sets = [torch.ones(L, dtype=torch.bool, device=dev)]
            if mask is not None:
                sets += [mask[g, j], ~mask[g, j]]
            for s, sel in enumerate(sets):
                split[g, r, s], split_rm[g, r, s], split_mm[g, r, s] = one(xr, Af[sel], c[sel])
                split_cnt[g, r, s] = int(sel.sum())
    return SparseRecon(curve, split, skipped, curve_rm, curve_mm, curve_cnt, split_rm, split_mm, split_cnt)


# ---------------------------------------------------------------------- profiles
def _rows_within(sc: SparseCodes, J: int) -> torch.Tensor:
    L = sc.row_ptr[:, 1:] - sc.row_ptr[:, :-1]
    return (L.unsqueeze(-1) <= torch.arange(J + 1, device=L.device)).sum(1)


def _moments(x: torch.Tensor, G: int):
    """(s1 [G, d], s2 [G]) of the rows ``x`` in fp64, the sums ``evaluate()`` keeps (shared rows are summed
    once and the result is broadcast to the models)."""
    xf = x.double() if x.dim() == 3 else x.double().unsqueeze(0)
    return xf.sum(1).expand(G, -1), xf.pow(2).sum((1, 2)).expand(G)


def _start(state, G, J, keep, d, dev):
    f64 = dict(dtype=torch.float64, device=dev)
    if state is None:
        z = lambda *s: torch.zeros(*s, **f64)
        return ReconProfile(0, z(G, J + 1), z(G), z(G) if keep else None, z(G) if keep else None,
                            torch.zeros(G, J + 1, dtype=torch.int64, device=dev), z(G, d), z(G),
                            torch.zeros(G, dtype=torch.int64, device=dev))
    check_state(state, G, J, keep, d)
    cp = lambda t: None if t is None else t.to(dev, copy=True).contiguous()
    return ReconProfile(int(state.n_rows), cp(state.sse_prefix), cp(state.sse_full), cp(state.sse_keep),
                        cp(state.sse_rest), cp(state.rows_within), cp(state.s1), cp(state.s2), cp(state.skipped))


def recon_profile_reference(sparse_codes: SparseCodes, D: torch.Tensor, x: torch.Tensor, max_kept: int = 32,
                            keep=None, nactive=None, state: Optional[ReconProfile] = None) -> ReconProfile:
    """The ``ReconProfile`` of ``sparse_codes`` against ``D`` [G, n, d] and all its rows ``x`` from the fp64
    oracle (any device, any float dtype)."""
    sc = sparse_codes
    ref = sparse_recon_reference(sc, D, x, max_kept, keep, nactive)
    G, dev = sc.n_models, D.device
    acc = _start(state, G, check_max_kept(max_kept), keep is not None, D.shape[2], dev)
    s1, s2 = _moments(x.to(dev), G)
    ss = ref.split.sum(1)
    return ReconProfile(acc.n_rows + sc.n_rows, acc.sse_prefix + ref.curve.sum(1), acc.sse_full + ss[:, 0],
                        None if keep is None else acc.sse_keep + ss[:, 1],
                        None if keep is None else acc.sse_rest + ss[:, 2],
                        acc.rows_within + _rows_within(sc, acc.max_kept).to(dev), acc.s1 + s1, acc.s2 + s2,
                        acc.skipped + ref.skipped)


def recon_profile_fused(sparse_codes: SparseCodes, shadow: torch.Tensor, batches: Iterable[torch.Tensor],
                        max_kept: int = 32, keep=None, nactive=None,
                        state: Optional[ReconProfile] = None) -> ReconProfile:
    """The ``ReconProfile`` of ``sparse_codes`` against the bf16 dictionaries ``shadow`` [G, n, d] on the
    device.  ``batches`` yields the rows the decoder sees, batch by batch in the order of the CSR's rows
    (bf16 [B, d] shared or [G, B, d]; a batch may be overwritten once the next is asked for): per batch one
    ``recon_curve`` and one ``recon_split`` launch on the batch's row window, their per-row values summed in
    fp64, and the variance bookkeeping.  ``keep``: bool [G, n] or packed words.  Never synchronises."""
    from ..ops import sparse_recon as sr_ops

    sc = sparse_codes
    G, n, dev = sc.n_models, sc.n, shadow.device
    if shadow.dim() != 3 or tuple(shadow.shape[:2]) != (G, n):
        raise ValueError(f"the dictionaries must be [{G}, {n}, d], got {tuple(shadow.shape)}")
    J = check_max_kept(max_kept)
    live = live_counts(nactive, G, n, dev)
    words = _as_words(keep, G, n, dev)
    acc = _start(state, G, J, words is not None, shadow.shape[2], dev)
    twice = torch.zeros(G, device=dev, dtype=torch.int64)  # (the split launch counts the same skipped rows again)
    at = 0
    for x in batches:
        B = x.shape[-2]
        curve = sr_ops.recon_curve(sc.row_ptr, sc.col, sc.val, shadow, x, J, acc.skipped, row0=at, nactive=live)
        split = sr_ops.recon_split(sc.row_ptr, sc.col, sc.val, shadow, x, twice, keep=words, row0=at, nactive=live)
        acc.sse_prefix += curve.sum(1, dtype=torch.float64)
        ss = split.sum(1, dtype=torch.float64)
        acc.sse_full += ss[:, 0]
        if words is not None:
            acc.sse_keep += ss[:, 1]
            acc.sse_rest += ss[:, 2]
        s1, s2 = _moments(x, G)
        acc.s1 += s1
        acc.s2 += s2
        at += B
    if at != sc.n_rows:
        raise ValueError(f"the batches hold {at} rows, the sparse codes {sc.n_rows}")
    acc.rows_within += _rows_within(sc, J)
    acc.n_rows += sc.n_rows
    return acc


def top_features(sums: torch.Tensor, n_top: int, live=None) -> torch.Tensor:
    """bool [G, n]: the ``n_top`` features of every model with the largest ``sums`` [G, n] (the sum of a
    feature's codes), ties to the lower feature index; ``live``: features at or past ``live[g]`` are never
    ranked (masked ensembles)."""
    G, n = sums.shape
    if isinstance(n_top, bool) or int(n_top) != n_top or not 0 <= int(n_top) <= n:
        raise ValueError(f"n_top must be an integer in 0..{n}, got {n_top!r}")
    s = sums.double()
    alive = None
    if live is not None:
        live = torch.as_tensor(live).to(sums.device)
        alive = torch.arange(n, device=sums.device).unsqueeze(0) < live.reshape(-1, 1)
        s = torch.where(alive, s, torch.full_like(s, float("-inf")))
    order = torch.argsort(s, dim=1, descending=True, stable=True)
    mask = torch.zeros(G, n, dtype=torch.bool, device=sums.device)
    mask.scatter_(1, order[:, :int(n_top)], True)
    return mask if alive is None else mask & alive
