"""Expected interference of an ensemble: the result type and the fp64 torch oracle.

The activity-weighted capacity of Scherlis et al. 2022 (reference big_sweep.py:44-58): on a row, active
feature a with code c_a gets ``c_a / sum_b cos^2(a, b) c_b`` over the row's active features b, and the
expected interference of a feature is the mean of that value over the rows on which it fires.  A row
needs only the Gram matrix of its own active atoms, so the sparse codes of ``encode_sparse`` are the
natural input: ``CodeAnalyses.interference`` (``engine/analysis.py``) runs one
``ops.interference.active_capacity`` launch over them on the fused engines (``interference_fused``);
``active_capacity_reference`` computes the same sums in fp64 torch (CPU included) and is what the tests
compare against and what the analytic / eager engines run (``interference_reference``).

Per-entry capacities are quantised to multiples of 2^-32 and summed as int64, so the per-feature sums
are the same bits every run and under any split of the pool.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch

from .sparse_codes import SparseCodes

QUANTUM = 2.0 ** -32     # one unit of ``qsum``
NORM2_FLOOR = 1e-16      # clamp of a squared row norm (the reference clamps the norm at 1e-8)
TOTAL_FLOOR = 1e-8       # clamp of a row's total (reference :53)


class InterferenceSkipped(RuntimeError):
    """Rows were left out of an ``Interference``: their entries were not all stored, or not valid."""


@dataclass
class Interference:
    """Raw per-feature sums of the activity-weighted capacity over ``n_rows`` rows, G models, n features."""

    n_rows: int
    qsum: torch.Tensor       # int64 [G, n]  sum over the feature's entries of llrint(capacity * 2^32)
    count: torch.Tensor      # int64 [G, n]  entries (rows on which the feature fires) that were summed
    skipped: torch.Tensor    # int64 [G]     rows left out (entries not all stored, or an invalid column)
    capacity: torch.Tensor   # fp64 [G, n]   static capacity of the dictionary (``capacity_per_feature_lowrank``)

    @property
    def expected(self) -> torch.Tensor:
        """fp64 [G, n]: mean activity-weighted capacity over the rows on which the feature fires
        (``calc_expected_interference``); a feature that never fires reads 0."""
        return self.qsum.double() * QUANTUM / self.count.clamp(min=1).double()

    def per_model(self, g: int):
        """(expected, capacity, count) of model ``g``."""
        return self.expected[g], self.capacity[g], self.count[g]

    def check(self) -> "Interference":
        """Synchronises; raises ``InterferenceSkipped`` if any row was left out."""
        sk = self.skipped.cpu()
        if bool((sk != 0).any()):
            raise InterferenceSkipped(f"{sk.tolist()} rows per model were skipped (of {self.n_rows}): their sparse "
                                      "codes were not all stored -- encode with a larger budget, or budget=None")
        return self

    def merge(self, other: "Interference") -> "Interference":
        """The sums over the rows of both (same ensemble, same dictionaries).  Integer adds: merging the
        chunks of a pool in any order gives the bits of one call on the whole pool."""
        check_state(other, *self.qsum.shape)
        dev = self.qsum.device
        return Interference(self.n_rows + other.n_rows, self.qsum + other.qsum.to(dev),
                            self.count + other.count.to(dev), self.skipped + other.skipped.to(dev), self.capacity)

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        return {"n_rows": torch.tensor(int(self.n_rows), dtype=torch.int64), "qsum": self.qsum,
                "count": self.count, "skipped": self.skipped, "capacity": self.capacity}

    def save(self, path):
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, map_location="cpu") -> "Interference":
        sd = torch.load(path, map_location=map_location, weights_only=True)
        return cls(int(sd["n_rows"]), sd["qsum"], sd["count"], sd["skipped"], sd["capacity"])

    def to(self, device) -> "Interference":
        return Interference(self.n_rows, self.qsum.to(device), self.count.to(device), self.skipped.to(device),
                            self.capacity.to(device))


def check_state(state, G: int, n: int):
    """Validate the ``state`` argument of an ``interference`` call (the result of an earlier call)."""
    if not isinstance(state, Interference):
        raise ValueError("state must be the Interference of an earlier call")
    if tuple(state.qsum.shape) != (G, n) or tuple(state.count.shape) != (G, n) or tuple(state.skipped.shape) != (G,):
        raise ValueError(f"state is for another ensemble (qsum {tuple(state.qsum.shape)}, this one [{G}, {n}])")


class ActiveCapacity(NamedTuple):
    """What ``active_capacity_reference`` returns; the last three fields feed the tests' error bound."""

    entry_cap: torch.Tensor     # fp64 [G, cap]  capacity of every stored entry of a row that was not skipped, else 0
    qsum: torch.Tensor          # int64 [G, n]
    count: torch.Tensor         # int64 [G, n]
    skipped: torch.Tensor       # int64 [G]
    entry_total: torch.Tensor   # fp64 [G, cap]  the entry's total, sum_b cos^2(a, b) c_b
    entry_csum: torch.Tensor    # fp64 [G, cap]  the sum of the codes of the entry's row
    entry_len: torch.Tensor     # int64 [G, cap] the number of entries of the entry's row


def active_capacity_reference(sparse_codes: SparseCodes, D: torch.Tensor, nactive=None, row0: int = 0,
                              n_rows: Optional[int] = None) -> ActiveCapacity:
    """fp64 torch oracle of ``ops.interference.active_capacity`` on the rows ``row0 .. row0 + n_rows - 1``
    (default: all) of ``sparse_codes`` against the dictionaries ``D`` [G, n, d], whose values are read as
    they are (bf16 included) in fp64.  Same definitions, skip rule and quantisation as the kernel:
    ``cos^2(a, b) = G_ab^2 / (max(|d_a|^2, 1e-16) max(|d_b|^2, 1e-16))``, ``cos^2(a, a) := 1``,
    ``cap_a = c_a / max(total_a, 1e-8)``, ``q_a = round-half-even(cap_a 2^32)``; a row is skipped when its
    pointers are outside [0, cap] or decreasing, it has more than n entries, or a column is outside
    [0, n) / [0, ``nactive[g]``)."""
    sc = sparse_codes
    G, n, cap = sc.n_models, sc.n, sc.cap
    if D.dim() != 3 or D.shape[0] != G or D.shape[1] != n:
        raise ValueError(f"D must be [{G}, {n}, d], got {tuple(D.shape)}")
    n_rows = sc.n_rows - row0 if n_rows is None else int(n_rows)
    if row0 < 0 or n_rows < 0 or row0 + n_rows > sc.n_rows:
        raise ValueError(f"rows [{row0}, {row0 + n_rows}) outside [0, {sc.n_rows}]")
    dev = D.device
    Dd = D.double()
    norm2 = (Dd * Dd).sum(-1).clamp(min=NORM2_FLOOR)
    lim = [n] * G
    if nactive is not None:
        lim = [min(n, max(0, int(v))) for v in torch.as_tensor(nactive).reshape(-1).tolist()]
    entry_cap = torch.zeros(G, cap, dtype=torch.float64, device=dev)
    entry_total = torch.zeros(G, cap, dtype=torch.float64, device=dev)
    entry_csum = torch.zeros(G, cap, dtype=torch.float64, device=dev)
    entry_len = torch.zeros(G, cap, dtype=torch.int64, device=dev)
    qsum = torch.zeros(G, n, dtype=torch.int64, device=dev)
    count = torch.zeros(G, n, dtype=torch.int64, device=dev)
    skipped = torch.zeros(G, dtype=torch.int64, device=dev)
    ptr = sc.row_ptr.to(dev).tolist()
    for g in range(G):
        colg, valg = sc.col[g].to(dev).long(), sc.val[g].to(dev).double()
        for r in range(row0, row0 + n_rows):
            lo, hi = ptr[g][r], ptr[g][r + 1]
            if lo < 0 or hi < lo or hi > cap or hi - lo > n:
                skipped[g] += 1
                continue
            if hi == lo:
                continue
            j, c = colg[lo:hi], valg[lo:hi]
            if bool(((j < 0) | (j >= lim[g])).any()):
                skipped[g] += 1
                continue
            A = Dd[g, j]
            gram = A @ A.T
            cos2 = gram * gram / (norm2[g, j].unsqueeze(1) * norm2[g, j].unsqueeze(0))
            cos2.fill_diagonal_(1.0)
            total = cos2 @ c
            cp = c / total.clamp(min=TOTAL_FLOOR)
            entry_cap[g, lo:hi], entry_total[g, lo:hi] = cp, total
            entry_csum[g, lo:hi], entry_len[g, lo:hi] = c.sum(), hi - lo
            qsum[g].index_add_(0, j, torch.round(cp * 2.0 ** 32).to(torch.int64))
            count[g].index_add_(0, j, torch.ones_like(j))
    return ActiveCapacity(entry_cap, qsum, count, skipped, entry_total, entry_csum, entry_len)


def live_counts(nactive, G: int, n: int, device) -> Optional[torch.Tensor]:
    """``nactive`` (None, an int, or one count per model) as an int32 [G] tensor on ``device``, or None."""
    if nactive is None:
        return None
    t = torch.as_tensor(nactive, device=device).to(torch.int32).reshape(-1)
    if t.numel() == 1:
        t = t.expand(G)
    if t.numel() != G:
        raise ValueError(f"nactive must hold one count per model ({G}), got {t.numel()}")
    return t.clamp(0, n).contiguous()


def interference_reference(sparse_codes: SparseCodes, D: torch.Tensor, nactive=None,
                           state: Optional[Interference] = None) -> Interference:
    """The ``Interference`` of ``sparse_codes`` against the dictionaries ``D`` [G, n, d] from the fp64 oracle
    (any device, any float dtype), merged into ``state`` when one is continued."""
    from ..eval.metrics import capacity_per_feature_lowrank

    ref = active_capacity_reference(sparse_codes.to(D.device), D, nactive)
    out = Interference(sparse_codes.n_rows, ref.qsum, ref.count, ref.skipped, capacity_per_feature_lowrank(D, nactive))
    return out if state is None else state.merge(out)


def interference_fused(sparse_codes: SparseCodes, shadow: torch.Tensor, nactive=None,
                       state: Optional[Interference] = None) -> Interference:
    """The ``Interference`` of ``sparse_codes`` against the bf16 dictionaries ``shadow`` [G, n, d] on the
    device: ``row_norm2``, one ``active_capacity`` launch over all rows, and the static capacity from
    ``eval.metrics.capacity_per_feature_lowrank`` (taken from ``state`` when one is continued).  Never
    synchronises."""
    from ..eval.metrics import capacity_per_feature_lowrank
    from ..ops import interference as ic_ops

    sc = sparse_codes
    G, n, dev = sc.n_models, sc.n, shadow.device
    if tuple(shadow.shape[:2]) != (G, n):
        raise ValueError(f"the dictionaries must be [{G}, {n}, d], got {tuple(shadow.shape)}")
    live = live_counts(nactive, G, n, dev)
    if state is None:
        qsum = torch.zeros(G, n, device=dev, dtype=torch.int64)
        count = torch.zeros(G, n, device=dev, dtype=torch.int64)
        skipped = torch.zeros(G, device=dev, dtype=torch.int64)
        capacity = capacity_per_feature_lowrank(shadow, live)
        seen = 0
    else:
        check_state(state, G, n)
        qsum, count = state.qsum.to(dev, copy=True).contiguous(), state.count.to(dev, copy=True).contiguous()
        skipped, capacity = state.skipped.to(dev, copy=True).contiguous(), state.capacity.to(dev)
        seen = int(state.n_rows)
    ic_ops.active_capacity(sc.row_ptr, sc.col, sc.val, shadow, ic_ops.row_norm2(shadow), qsum, count, skipped,
                           nactive=live)
    return Interference(seen + sc.n_rows, qsum, count, skipped, capacity)
