"""Per-feature label profiles from sparse codes: the result type, the torch oracle and the device route.

Every other analysis of the sparse codes asks about the codes alone, or about codes against dictionaries.  This
one relates a feature to what the rows ARE: ``labels`` gives every row of the pool an integer label -- the row's
token id, its position in the fragment, a concept flag -- and the profile is the group-by of every feature's
entries on it.  A negative label leaves the row out (padding, BOS).  With M kept rows, for model g and feature f:

- a **run** is the set of the feature's entries on rows with one label.  Per run: ``count`` (int32), ``max``
  (fp32) and ``sum`` (fp64): ``acc = acc + double(val)`` from 0.0 over the run's entries in ascending row order --
  strictly sequential, so the bits are those of a plain loop.
- per feature: ``n_entries`` (int64, its entries on kept rows), ``n_labels`` (int32, its runs), ``count_sq``
  (int64, the sum of ``count^2`` over its runs) and ``total`` (fp64): ``acc = acc + sum_run`` from 0.0 over the
  runs in ascending label.
- **top**: the ``m`` best runs (1 <= m <= 64) under ``rank_by``: "sum" -- the fp64 sum descending; "count" -- the
  count descending; then the label ascending.  ``top_label`` / ``top_count`` / ``top_sum`` / ``top_max``, all m
  slots written, empty slots ``(-1, 0, 0.0, 0.0)``.
- **skip rule** (that of ``by_feature``): a kept row with more than n entries or a column outside ``[0, lim)``,
  lim = n or ``min(n, nactive[g])``, is left out whole and counted in ``skipped[g]``.  The codes must be complete
  (``SparseCodes.check()``).

The device route puts the kept rows in label order first (a stable argsort, then ``SparseCodes.take_rows``): every
feature's list of the transposed codes (rows ascending) is then grouped by label for free, and one walk per list
(``csrc/label_profile.hip``) computes all of the above without a hash table and without a floating-point atomic.
The oracle computes the same from the unpermuted CSR with stable sorts.  All outputs are integers, copies of fp32
values or fp64 sums in a fixed order: the oracle compares with ``torch.equal``.  Means, shares, precision, recall
and entropy-like figures are derived from these in torch (``LabelProfile.share()`` ...), never on the device.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from ..ops.label_profile import RANKS, check_m, check_rank   # (plain Python: no kernel library is loaded)
from .feature_codes import _check_codes, _place, by_feature
from .interference import live_counts
from .sparse_codes import SparseCodes

LABEL_LIMIT = 2 ** 31 - 1     # labels are < this (the device keeps them in int32)


@dataclass
class LabelProfile:
    """Per feature of G models the ``m`` labels that carry its activations, with the totals they are shares of."""

    n_entries: torch.Tensor    # int64 [G, n]     entries of the feature on kept rows
    n_labels: torch.Tensor     # int32 [G, n]     distinct labels on which it fires
    count_sq: torch.Tensor     # int64 [G, n]     sum over its labels of count^2
    total: torch.Tensor        # fp64 [G, n]      sum of its codes (label by label, module docstring)
    top_label: torch.Tensor    # int32 [G, n, m]  best label first; -1: empty slot
    top_count: torch.Tensor    # int32 [G, n, m]  the feature's entries on that label
    top_sum: torch.Tensor      # fp64 [G, n, m]   the sum of its codes on that label
    top_max: torch.Tensor      # fp32 [G, n, m]   the largest of them
    skipped: torch.Tensor      # int64 [G]        kept rows left out by the skip rule
    n_rows: int                # kept rows M
    rank_by: str
    label_rows: Optional[torch.Tensor] = None   # int64 [L]  kept rows per label (with n_classes=L)

    _TENSORS = ("n_entries", "n_labels", "count_sq", "total", "top_label", "top_count", "top_sum", "top_max",
                "skipped")

    @property
    def n_models(self) -> int:
        return int(self.top_label.shape[0])

    @property
    def n(self) -> int:
        return int(self.top_label.shape[1])

    @property
    def m(self) -> int:
        return int(self.top_label.shape[2])

    # ------------------------------------------------------------------ derived views (fp64 torch, 0 where undefined)
    @staticmethod
    def _ratio(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
        num, den = num.double(), den.double()
        ok = den > 0
        return torch.where(ok, num / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(num))

    def share(self) -> torch.Tensor:
        """[G, n, m]: the part of the feature's total activation that falls on each of its top labels."""
        return self._ratio(self.top_sum, self.total.unsqueeze(-1).expand_as(self.top_sum))

    def precision(self) -> torch.Tensor:
        """[G, n, m]: of the rows on which the feature fires, the part that carries the label."""
        return self._ratio(self.top_count, self.n_entries.unsqueeze(-1).expand_as(self.top_count))

    def recall(self) -> torch.Tensor:
        """[G, n, m]: of the kept rows that carry the label, the part on which the feature fires.  Needs
        ``label_rows`` (``n_classes=``)."""
        if self.label_rows is None:
            raise ValueError("recall() needs the rows per label: build the profile with n_classes=")
        live = self.top_label >= 0
        rows = self.label_rows.to(self.top_label.device)[self.top_label.clamp(min=0).long()]
        return self._ratio(self.top_count, torch.where(live, rows, torch.zeros_like(rows)))

    def f1(self) -> torch.Tensor:
        """[G, n, m]: the harmonic mean of ``precision()`` and ``recall()``."""
        p, r = self.precision(), self.recall()
        return self._ratio(2 * p * r, p + r)

    def effective_labels(self) -> torch.Tensor:
        """[G, n]: ``n_entries^2 / count_sq``, the inverse Simpson index of the feature's rows over labels: 1 for
        a feature on one label, k for one spread evenly over k."""
        ne = self.n_entries.double()
        return self._ratio(ne * ne, self.count_sq)

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        sd = {k: getattr(self, k) for k in self._TENSORS}
        sd["n_rows"] = torch.tensor(int(self.n_rows), dtype=torch.int64)
        sd["rank_by"] = torch.tensor(RANKS.index(self.rank_by), dtype=torch.int64)
        if self.label_rows is not None:
            sd["label_rows"] = self.label_rows
        return sd

    def save(self, path):
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, map_location="cpu") -> "LabelProfile":
        sd = torch.load(path, map_location=map_location, weights_only=True)
        return cls(*(sd[k] for k in cls._TENSORS), int(sd["n_rows"]), RANKS[int(sd["rank_by"])], sd.get("label_rows"))

    def to(self, device) -> "LabelProfile":
        return LabelProfile(*(getattr(self, k).to(device) for k in self._TENSORS), self.n_rows, self.rank_by,
                            None if self.label_rows is None else self.label_rows.to(device))


# ---------------------------------------------------------------------- checks
def check_labels(sc: SparseCodes, labels: torch.Tensor, n_classes=None) -> Tuple[torch.Tensor, Optional[int]]:
    """``labels`` as int64 [n_rows] on the codes' device, and ``n_classes`` as an int.  Synchronises (one host
    read of the largest label)."""
    if not isinstance(labels, torch.Tensor) or labels.dtype not in (torch.int32, torch.int64) or labels.dim() != 1:
        raise ValueError("labels must be an int32 or int64 tensor [n_rows]")
    if labels.shape[0] != sc.n_rows:
        raise ValueError(f"labels must hold one label per row ({sc.n_rows}), got {labels.shape[0]}")
    if n_classes is not None:
        if isinstance(n_classes, bool) or int(n_classes) != n_classes or not 1 <= int(n_classes) <= LABEL_LIMIT:
            raise ValueError(f"n_classes must be an integer in 1..{LABEL_LIMIT}, got {n_classes!r}")
        n_classes = int(n_classes)
    labels = labels.to(sc.col.device, torch.int64)
    top = int(labels.max()) if labels.numel() else -1
    if top >= LABEL_LIMIT:
        raise ValueError(f"labels must be < 2^31 - 1, got {top}")
    if n_classes is not None and top >= n_classes:
        raise ValueError(f"labels must be < n_classes = {n_classes}, got {top}")
    return labels, n_classes


def _empty(G, n, m, dev):
    return (torch.zeros(G, n, dtype=torch.int64, device=dev), torch.zeros(G, n, dtype=torch.int32, device=dev),
            torch.zeros(G, n, dtype=torch.int64, device=dev), torch.zeros(G, n, dtype=torch.float64, device=dev),
            torch.full((G, n, m), -1, dtype=torch.int32, device=dev),
            torch.zeros(G, n, m, dtype=torch.int32, device=dev),
            torch.zeros(G, n, m, dtype=torch.float64, device=dev),
            torch.zeros(G, n, m, dtype=torch.float32, device=dev))


# ---------------------------------------------------------------------- the oracle
def _stepped_sum(group: torch.Tensor, pos: torch.Tensor, x: torch.Tensor, n_groups: int) -> torch.Tensor:
    """fp64 [n_groups]: per group ``acc = acc + x`` from 0.0 over its members in the order of ``pos`` (0, 1, ...
    inside every group): vectorised across the groups, stepped over the position."""
    acc = torch.zeros(n_groups, dtype=torch.float64, device=x.device)
    if x.numel() == 0:
        return acc
    order = torch.sort(pos, stable=True).indices
    ends = torch.cumsum(torch.bincount(pos), 0).tolist()
    lo = 0
    for hi in ends:
        at = order[lo:hi]                        # (one member per group: no index repeats)
        acc[group[at]] = acc[group[at]] + x[at]
        lo = hi
    return acc


def profile_entries_reference(feat: torch.Tensor, lab: torch.Tensor, val: torch.Tensor, n: int, m: int, rank_by: str):
    """The eight outputs ([n] and [n, m]) of ONE model from its entries in list order: ``feat`` int64 [E]
    non-decreasing, ``lab`` int64 [E] the entry's label, ``val`` fp32 [E].  A run is a maximal stretch of entries
    with one (feature, label)."""
    m, rank_by = check_m(m), check_rank(rank_by)
    dev = val.device
    out = tuple(t[0] for t in _empty(1, n, m, dev))
    E = feat.numel()
    if E == 0:
        return out
    head = torch.ones(E, dtype=torch.bool, device=dev)
    head[1:] = (feat[1:] != feat[:-1]) | (lab[1:] != lab[:-1])
    rid = torch.cumsum(head, 0) - 1                       # run of every entry
    start = torch.nonzero(head).flatten()
    R = start.numel()
    cnt = torch.bincount(rid, minlength=R)
    rfeat, rlab = feat[start], lab[start]
    rmax = torch.full((R,), float("-inf"), device=dev).scatter_reduce(0, rid, val, "amax")
    rsum = _stepped_sum(rid, torch.arange(E, device=dev) - start[rid], val.double(), R)
    n_labels = torch.bincount(rfeat, minlength=n)
    first = torch.cumsum(n_labels, 0) - n_labels
    total = _stepped_sum(rfeat, torch.arange(R, device=dev) - first[rfeat], rsum, n)
    count_sq = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, rfeat, cnt * cnt)
    o = torch.sort(rlab, stable=True).indices                                   # label ascending among equals
    key = rsum if rank_by == "sum" else cnt
    o = o[torch.sort(key[o], descending=True, stable=True).indices]
    o = o[torch.sort(rfeat[o], stable=True).indices]
    pf = rfeat[o]
    return (torch.bincount(feat, minlength=n), n_labels.to(torch.int32), count_sq, total,
            _place(pf, rlab[o], n, m, -1, torch.int32), _place(pf, cnt[o], n, m, 0, torch.int32),
            _place(pf, rsum[o], n, m, 0.0, torch.float64), _place(pf, rmax[o], n, m, 0.0, torch.float32))


def profile_lists_reference(col_ptr: torch.Tensor, row: torch.Tensor, val: torch.Tensor, lab: torch.Tensor,
                            m: int = 8, rank_by: str = "sum"):
    """Torch oracle of ``ops.label_profile.label_profile`` (any device) on the same inputs, with the kernel's
    guards: list f is ``[lo, hi)`` with ``lo = clamp(col_ptr[f], 0, cap)`` and ``hi = min(max(col_ptr[f + 1], lo),
    cap)``, and an entry whose row lies outside [0, M) is skipped.  Returns the tuple of eight."""
    G, n, cap, M, dev = col_ptr.shape[0], col_ptr.shape[1] - 1, row.shape[1], lab.shape[0], row.device
    outs = []
    for g in range(G):
        lo = col_ptr[g, :-1].clamp(0, cap)
        hi = torch.minimum(torch.maximum(col_ptr[g, 1:], lo), torch.full_like(lo, cap))
        ln = hi - lo
        k = int(ln.sum())
        feat = torch.repeat_interleave(torch.arange(n, device=dev), ln)
        at = torch.repeat_interleave(lo - (torch.cumsum(ln, 0) - ln), ln) + torch.arange(k, device=dev)
        r = row[g][at].long()
        ok = (r >= 0) & (r < M)
        feat, at, r = feat[ok], at[ok], r[ok]
        outs.append(profile_entries_reference(feat, lab[r].long(), val[g][at], n, m, rank_by))
    return tuple(torch.stack([o[i] for o in outs]) for i in range(8))


def label_profile_reference(sc: SparseCodes, labels: torch.Tensor, *, m: int = 8, rank_by: str = "sum",
                            n_classes=None, nactive=None) -> LabelProfile:
    """Torch oracle of ``label_profile`` (any device; this is what runs off the GPU), straight from the
    unpermuted CSR: the entries of the kept rows that pass the skip rule in a stable sort by (feature, label,
    row); run sums vectorised across runs and stepped sequentially over the position inside the run, in fp64 --
    the kernel's order."""
    m, rank_by = check_m(m), check_rank(rank_by)
    _check_codes(sc)
    labels, n_classes = check_labels(sc, labels, n_classes)
    sc.check()
    G, n, N, dev = sc.n_models, sc.n, sc.n_rows, sc.col.device
    live = live_counts(nactive, G, n, dev)
    lim = [n] * G if live is None else live.tolist()
    kept = labels >= 0
    skipped = torch.zeros(G, dtype=torch.int64, device=dev)
    outs = []
    for g in range(G):
        stored = int(sc.row_ptr[g, -1])
        rows, cols, vals = sc.entry_rows(g), sc.col[g, :stored].long(), sc.val[g, :stored]
        bad = (sc.row_ptr[g, 1:] - sc.row_ptr[g, :-1]) > n
        bad[rows[(cols < 0) | (cols >= lim[g])]] = True        # one bad column condemns the whole row
        skipped[g] = int((bad & kept).sum())
        use = kept[rows] & ~bad[rows]
        rows, cols, vals = rows[use], cols[use], vals[use]      # (row, column) ascending
        lab = labels[rows]
        o = torch.sort(lab, stable=True).indices
        o = o[torch.sort(cols[o], stable=True).indices]         # (feature, label, row) ascending
        outs.append(profile_entries_reference(cols[o], lab[o], vals[o], n, m, rank_by))
    out = tuple(torch.stack([o[i] for o in outs]) for i in range(8)) if G else _empty(0, n, m, dev)
    rows_per = None if n_classes is None else torch.bincount(labels[kept], minlength=n_classes)
    return LabelProfile(*out, skipped, int(kept.sum()), rank_by, rows_per)


# ---------------------------------------------------------------------- the routes
def label_profile(sc: SparseCodes, labels: torch.Tensor, *, m: int = 8, rank_by: str = "sum", n_classes=None,
                  nactive=None, waves: int = 4) -> LabelProfile:
    """The ``LabelProfile`` of the complete sparse codes ``sc`` under ``labels`` (int32 / int64 [sc.n_rows]; a
    negative label leaves the row out; labels are < 2^31 - 1, and < ``n_classes`` when that is given, which also
    adds ``label_rows`` for ``recall()``): per feature of every model its ``m`` (1..64) best labels by ``rank_by``
    ("sum" or "count") with their counts, fp64 sums and maxima (module docstring).  ``nactive``: live features
    per model of a masked ensemble.

    On a GPU: a stable argsort of the kept labels, ``sc.take_rows`` of the kept rows in that order,
    ``by_feature(nactive)`` and one ``sc_label_profile`` launch (``csrc/label_profile.hip``; ``waves``: its
    waves per block, the bits do not depend on it).  The label checks and ``take_rows`` synchronise; the
    transposition and the kernel do not.  Elsewhere ``label_profile_reference``."""
    if not sc.col.is_cuda:
        return label_profile_reference(sc, labels, m=m, rank_by=rank_by, n_classes=n_classes, nactive=nactive)
    from ..ops import label_profile as lp_ops

    m, rank_by = check_m(m), check_rank(rank_by)
    _check_codes(sc)
    labels, n_classes = check_labels(sc, labels, n_classes)
    G, n, dev = sc.n_models, sc.n, sc.col.device
    kept = torch.nonzero(labels >= 0).flatten()
    lab, order = torch.sort(labels[kept], stable=True)
    rows_per = None if n_classes is None else torch.bincount(lab, minlength=n_classes)
    taken = sc.take_rows(kept[order])
    M = taken.n_rows
    if M == 0 or G == 0:
        return LabelProfile(*_empty(G, n, m, dev), torch.zeros(G, dtype=torch.int64, device=dev), M, rank_by,
                            rows_per)
    fc = by_feature(taken, nactive)
    out = lp_ops.label_profile(fc.col_ptr, fc.row, fc.val, lab.to(torch.int32).contiguous(), m, rank_by, waves=waves)
    return LabelProfile(*out, fc.skipped, M, rank_by, rows_per)
