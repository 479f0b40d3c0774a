"""Value-ordered feature lists: quantiles, strata, histograms and the exact AUROC of every (feature, concept)
pair -- the result types, the torch oracles and the device routes.

``FeatureCodes.by_value()`` orders every feature's list by the value of its codes: a ``ValueOrdered`` with the
fields of the ``FeatureCodes`` it came from, the same ``col_ptr``, and ``row`` / ``val`` holding every list at its
own positions in value order (``ops.value_order.sort_lists``, ``csrc/value_order.hip``, on a GPU;
``sort_lists_reference`` elsewhere).  With the lists contiguous and sorted, the whole buffer of a model is sorted
by (feature, key): quantiles and strata are index arithmetic, a histogram is one ``searchsorted``, and the AUROC
of a feature's activation as a detector of a concept is one walk with integer sums
(``ops.value_order.list_auroc``).

- **Order**: key ascending, then row ascending.  The key is the order-preserving map of the fp32 bit pattern
  (``float_keys``): a total order on all bit patterns in which -0.0 comes before +0.0.  Rows are distinct in a
  list, so the order is unique.  The sort is stable on the input, whose rows ascend.
- **Lists**: those of ``ops.value_order.stored_ptr``: the running maximum of ``col_ptr`` clipped to the buffers,
  which for the ``col_ptr`` of a complete ``FeatureCodes`` is ``col_ptr`` itself.
- **AUROC**: every row of the pool counts; a row on which the feature does not fire scores 0, and stored codes
  are taken to be > 0, which ``encode_sparse`` guarantees.  Ties are equal fp32 values.

All outputs are integers, copies of fp32 values, or one fp64 division of integers: the oracles compare with
``torch.equal``.  Neither the order nor the rank sums can be merged across chunks of rows: a pool is given whole.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from ..ops.value_order import MAX_CONCEPTS, check_concepts, stored_ptr   # (plain Python: no kernel library is loaded)
from .feature_codes import FeatureCodes, FeatureCodesSkipped, by_feature, feature_codes_reference
from .sparse_codes import SparseCodes

_M32 = 0xFFFFFFFF


def float_keys(val: torch.Tensor) -> torch.Tensor:
    """int64 keys in [0, 2^32) of fp32 values: ordered as unsigned integers they order the values, -0.0 before
    +0.0, negative NaNs first and positive NaNs last (``order_key`` of ``csrc/common.h``)."""
    u = val.contiguous().view(torch.int32).to(torch.int64) & _M32
    return torch.where(u >= 0x80000000, u ^ _M32, u | 0x80000000)


def concept_words(positives: torch.Tensor) -> torch.Tensor:
    """The flag words int32 [N] of ``positives`` bool [N, K], K <= 32: bit k of word r is ``positives[r, k]``."""
    if positives.dim() != 2 or positives.dtype != torch.bool:
        raise ValueError("positives must be a bool tensor [N, K]")
    K = check_concepts(positives.shape[1])
    w = (positives.to(torch.int64) << torch.arange(K, device=positives.device)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def check_flags(flags: torch.Tensor, n_rows: int, n_concepts=None, device=None) -> Tuple[torch.Tensor, int]:
    """``flags`` as contiguous int32 words [n_rows] on ``device`` and the number of concepts: a bool [N, K] matrix
    is packed (``concept_words``), int32 words come with ``n_concepts`` (default 32)."""
    if not isinstance(flags, torch.Tensor):
        raise ValueError("flags must be int32 words [N] or a bool tensor [N, K]")
    if flags.dtype == torch.bool:
        K = check_concepts(flags.shape[1] if flags.dim() == 2 else 0)
        if n_concepts is not None and check_concepts(n_concepts) != K:
            raise ValueError(f"n_concepts = {n_concepts} but flags holds {K} concepts")
        flags = concept_words(flags)
    else:
        K = check_concepts(MAX_CONCEPTS if n_concepts is None else n_concepts)
        if flags.dtype != torch.int32 or flags.dim() != 1:
            raise ValueError("flags must be int32 words [N] or a bool tensor [N, K]")
    if flags.shape[0] != n_rows:
        raise ValueError(f"flags must hold one word per row ({n_rows}), got {flags.shape[0]}")
    if n_rows >= 2 ** 31:
        raise ValueError(f"auroc needs N < 2^31 (got N={n_rows})")
    return flags.to(flags.device if device is None else device).contiguous(), K


def concept_counts(flags: torch.Tensor, n_concepts: int) -> torch.Tensor:
    """int64 [K]: the rows whose word has bit k set."""
    return ((flags.to(torch.int64).unsqueeze(1) >> torch.arange(n_concepts, device=flags.device)) & 1).sum(0)


# ---------------------------------------------------------------------- result types
@dataclass
class FeatureAuroc:
    """The rank sums of every (feature, concept) pair of G models over a pool of ``n_rows`` rows."""

    u2: torch.Tensor       # int64 [G, n, K]  over the positives of the list: 2 #{smaller negatives} + #{equal ones}
    pos_in: torch.Tensor   # int32 [G, n, K]  positives among the rows on which the feature fires
    cnt: torch.Tensor      # int64 [G, n]     rows on which the feature fires: the stored length of its list
    n_pos: torch.Tensor    # int64 [K]        positives of the pool
    n_rows: int

    _TENSORS = ("u2", "pos_in", "cnt", "n_pos")

    def num2(self) -> torch.Tensor:
        """int64 [G, n, K]: twice the number of (positive, negative) pairs of the pool that the feature's
        activation orders correctly, ties counting half.  A row outside the list scores 0, below every stored
        code: each positive of the list beats every negative outside it, and the positives outside tie with
        the negatives outside."""
        pos_in = self.pos_in.to(torch.int64)
        out_neg = (self.n_rows - self.n_pos) - (self.cnt.unsqueeze(-1) - pos_in)    # negatives outside the list
        return self.u2 + 2 * pos_in * out_neg + (self.n_pos - pos_in) * out_neg

    def auroc(self) -> torch.Tensor:
        """fp64 [G, n, K]: ``num2 / (2 P (N - P))``, one division of integers; NaN for a concept with no
        positive or no negative.  An empty list reads exactly 0.5."""
        den = 2 * self.n_pos * (self.n_rows - self.n_pos)
        return self.num2().to(torch.float64) / den.to(torch.float64).masked_fill(den == 0, float("nan"))

    def best(self, m: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(feature int64 [G, K, m], auroc fp64 [G, K, m]): per model and concept the ``m`` features with the
        largest AUROC, AUROC descending, then feature ascending."""
        a = self.auroc().transpose(1, 2)
        if isinstance(m, bool) or int(m) != m or not 1 <= int(m) <= a.shape[-1]:
            raise ValueError(f"m must be an integer in 1..{a.shape[-1]}, got {m!r}")
        top, feat = torch.sort(a, dim=-1, descending=True, stable=True)
        return feat[..., :int(m)], top[..., :int(m)]

    def state_dict(self):
        sd = {k: getattr(self, k) for k in self._TENSORS}
        sd["n_rows"] = torch.tensor(int(self.n_rows), dtype=torch.int64)
        return sd

    def save(self, path):
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, map_location="cpu") -> "FeatureAuroc":
        sd = torch.load(path, map_location=map_location, weights_only=True)
        return cls(*(sd[k] for k in cls._TENSORS), int(sd["n_rows"]))

    def to(self, device) -> "FeatureAuroc":
        return FeatureAuroc(*(getattr(self, k).to(device) for k in self._TENSORS), self.n_rows)


@dataclass
class ValueOrdered:
    """Feature-major codes of G models with n features over ``n_rows`` rows, every list in value order.

    The list of feature ``f`` of model ``g`` is ``row/val[g, col_ptr[g, f] : col_ptr[g, f + 1]]``, key ascending,
    then row ascending (module docstring): the smallest code first.  ``col_ptr`` and ``skipped`` are those of the
    ``FeatureCodes`` the lists came from.  The methods are torch index arithmetic on the device and never
    synchronise."""

    n_rows: int
    n: int
    col_ptr: torch.Tensor   # int64 [G, n + 1]
    row: torch.Tensor       # int32 [G, cap]
    val: torch.Tensor       # fp32 [G, cap]
    skipped: torch.Tensor   # int64 [G]  rows left out by the skip rule of ``by_feature``

    @property
    def cap(self) -> int:
        return int(self.row.shape[1])

    @property
    def n_models(self) -> int:
        return int(self.col_ptr.shape[0])

    def counts(self) -> torch.Tensor:
        """Entries of every feature, int64 [G, n] on the device."""
        return self.col_ptr[:, 1:] - self.col_ptr[:, :-1]

    def check(self) -> "ValueOrdered":
        """Synchronises; raises ``FeatureCodesSkipped`` if any row was skipped or any entry dropped."""
        FeatureCodes(self.n_rows, self.n, self.col_ptr, self.row, self.val, self.skipped).check()
        return self

    def bounds(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(lo, hi) int64 [G, n]: the stored part of every list."""
        b = stored_ptr(self.col_ptr, self.cap)
        return b[:, :-1], b[:, 1:]

    def _take(self, pos: torch.Tensor, live: torch.Tensor, fill_row: int, fill_val: float):
        """``row`` / ``val`` at the positions ``pos`` [G, ...] where ``live``, the fills elsewhere."""
        G = self.n_models
        if self.cap == 0:
            return (torch.full(pos.shape, fill_row, dtype=torch.int32, device=pos.device),
                    torch.full(pos.shape, fill_val, dtype=torch.float32, device=pos.device))
        at = pos.clamp(min=0, max=self.cap - 1).reshape(G, -1)
        r = torch.gather(self.row, 1, at).view(pos.shape)
        v = torch.gather(self.val, 1, at).view(pos.shape)
        return (torch.where(live, r, torch.full_like(r, fill_row)), torch.where(live, v, torch.full_like(v, fill_val)))

    def quantiles(self, Q: int) -> torch.Tensor:
        """fp32 [G, n, Q + 1]: entry k is the list's value at sorted position ``(k (L - 1)) // Q`` (integer
        arithmetic; k = 0 the minimum, k = Q the maximum); NaN for an empty list."""
        if isinstance(Q, bool) or int(Q) != Q or int(Q) < 1:
            raise ValueError(f"Q must be a positive integer, got {Q!r}")
        lo, hi = self.bounds()
        L = (hi - lo).unsqueeze(-1)
        k = torch.arange(int(Q) + 1, device=lo.device)
        pos = lo.unsqueeze(-1) + (k * (L - 1).clamp(min=0)) // int(Q)
        return self._take(pos, (L > 0).expand_as(pos), 0, float("nan"))[1]

    def strata(self, n_strata: int, per_stratum: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(rows int32, vals fp32) [G, n, S, r]: stratum s of a list of L entries covers the sorted positions
        ``[s L // S, (s + 1) L // S)``; of its m positions it lists those at offsets ``(j m) // r``, j < r, when
        m >= r, otherwise all m; empty slots read (-1, 0.0).  Stratum S - 1 holds the largest codes."""
        for name, x in (("n_strata", n_strata), ("per_stratum", per_stratum)):
            if isinstance(x, bool) or int(x) != x or int(x) < 1:
                raise ValueError(f"{name} must be a positive integer, got {x!r}")
        S, r = int(n_strata), int(per_stratum)
        lo, hi = self.bounds()
        L = (hi - lo).view(*lo.shape, 1, 1)
        s = torch.arange(S, device=lo.device).view(1, 1, S, 1)
        j = torch.arange(r, device=lo.device).view(1, 1, 1, r)
        a = (s * L) // S
        m = ((s + 1) * L) // S - a
        off = torch.where(m >= r, (j * m) // r, j.expand_as(j * m))
        return self._take(lo.view(*lo.shape, 1, 1) + a + off, (j < m) | (m >= r), -1, 0.0)

    def composite(self) -> torch.Tensor:
        """int64 [G, cap]: ``feature 2^32 + key`` of every position, non-decreasing along a model's buffer
        (positions before the first list read feature -1, the tail reads feature n)."""
        b = stored_ptr(self.col_ptr, self.cap)
        p = torch.arange(self.cap, device=b.device).expand(self.n_models, -1).contiguous()
        feat = torch.searchsorted(b, p, right=True) - 1
        return (feat << 32) + float_keys(self.val)

    def histogram(self, edges: torch.Tensor) -> torch.Tensor:
        """int64 [G, n, H]: per list the entries with ``edges[b] <= v < edges[b + 1]`` in key order, which for
        the positive codes of ``encode_sparse`` is the order of the values.  ``edges``: fp32 [H + 1], ascending.
        One ``torch.searchsorted`` of composite (feature, key) queries per model buffer."""
        if edges.dim() != 1 or edges.dtype != torch.float32 or edges.shape[0] < 2:
            raise ValueError("edges must be fp32 [H + 1] with H >= 1")
        dev, G, n = self.row.device, self.n_models, self.n
        q = (torch.arange(n, device=dev).unsqueeze(1) << 32) + float_keys(edges.to(dev)).unsqueeze(0)   # [n, H + 1]
        at = torch.searchsorted(self.composite(), q.reshape(1, -1).expand(G, -1).contiguous())
        at = at.view(G, n, -1)
        return at[..., 1:] - at[..., :-1]

    def auroc(self, flags: torch.Tensor, n_concepts=None, *, kernels: Optional[bool] = None, **kw) -> FeatureAuroc:
        """The ``FeatureAuroc`` of every feature against the concepts of ``flags``: int32 words [n_rows] whose bit
        k says that the row is a positive of concept k (``n_concepts`` of them, default 32), or a bool [n_rows,
        K] matrix.  Every row of the pool counts: a row on which the feature does not fire scores 0, and stored
        codes are taken to be > 0, which ``encode_sparse`` guarantees.  (An entry whose row lies outside the pool
        is left out of the walk's sums but stays in ``cnt``; ``by_feature`` writes none.)  One ``sc_list_auroc``
        launch when the lists are on a GPU (``kw``: its ``waves``; never synchronises),
        ``list_auroc_reference`` elsewhere or with ``kernels=False``."""
        dev = self.row.device
        flags, K = check_flags(flags, self.n_rows, n_concepts, dev)
        if self.row.is_cuda if kernels is None else kernels:
            from ..ops import value_order as vo_ops

            pos_in, u2 = vo_ops.list_auroc(self.col_ptr.contiguous(), self.row, self.val, flags, K, **kw)
        else:
            if kw:
                raise TypeError(f"auroc: {sorted(kw)} are keywords of the device route")
            pos_in, u2 = list_auroc_reference(self.col_ptr, self.row, self.val, flags, K)
        lo, hi = self.bounds()
        return FeatureAuroc(u2, pos_in, hi - lo, concept_counts(flags, K), self.n_rows)

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        return {"n_rows": torch.tensor(int(self.n_rows), dtype=torch.int64),
                "n": torch.tensor(int(self.n), dtype=torch.int64),
                "col_ptr": self.col_ptr, "row": self.row, "val": self.val, "skipped": self.skipped}

    def save(self, path):
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, map_location="cpu") -> "ValueOrdered":
        sd = torch.load(path, map_location=map_location, weights_only=True)
        return cls(int(sd["n_rows"]), int(sd["n"]), sd["col_ptr"], sd["row"], sd["val"], sd["skipped"])

    def to(self, device) -> "ValueOrdered":
        return ValueOrdered(self.n_rows, self.n, self.col_ptr.to(device), self.row.to(device), self.val.to(device),
                            self.skipped.to(device))


# ---------------------------------------------------------------------- oracles
def _stored_entries(b: torch.Tensor):
    """(positions int64 [E], features int64 [E]) of the stored entries of one model with list bounds ``b``."""
    ln = b[1:] - b[:-1]
    feat = torch.repeat_interleave(torch.arange(ln.numel(), device=b.device), ln)
    return int(b[0]) + torch.arange(feat.numel(), device=b.device), feat


def sort_lists_reference(col_ptr: torch.Tensor, row: torch.Tensor, val: torch.Tensor,
                         cap_out: Optional[int] = None, out=None):
    """Torch oracle of ``ops.value_order.sort_lists`` (any device; this is what runs off the GPU): a stable
    ``torch.sort`` of the composite int64 keys ``feature 2^32 + key`` of the stored entries of every model.
    ``cap_out``: entries per model the output holds (default ``cap``); ``out``: buffers to fill instead."""
    G, cap = row.shape
    if out is None:
        cap_out = cap if cap_out is None else int(cap_out)
        out = (torch.zeros(G, cap_out, dtype=torch.int32, device=row.device),
               torch.zeros(G, cap_out, dtype=torch.float32, device=row.device))
    vrow, vval = out
    b = stored_ptr(col_ptr, min(cap, vrow.shape[1]))
    for g in range(G):
        at, feat = _stored_entries(b[g])
        order = torch.sort((feat << 32) + float_keys(val[g][at]), stable=True).indices
        vrow[g, at] = row[g][at][order]
        vval[g, at] = val[g][at][order]
    return vrow, vval


def list_auroc_reference(col_ptr: torch.Tensor, vrow: torch.Tensor, vval: torch.Tensor, flags: torch.Tensor,
                         n_concepts: int):
    """Torch oracle of ``ops.value_order.list_auroc`` (any device) on the same inputs: ``(pos_in int32, u2
    int64)``, [G, n, K].  Per model the stored entries with a row in [0, N), their tie runs (a new run where the
    feature changes or the fp32 value differs from the entry before), and exclusive cumulative counts of the
    negatives: a positive adds the count at its run's start plus the count at its run's end, both taken from its
    list's start."""
    K = check_concepts(n_concepts)
    G, cap = vrow.shape
    n, N, dev = col_ptr.shape[1] - 1, flags.shape[0], vrow.device
    b = stored_ptr(col_ptr, cap)
    pos_in = torch.zeros(G, n, K, dtype=torch.int64, device=dev)
    u2 = torch.zeros(G, n, K, dtype=torch.int64, device=dev)
    bits = (flags.to(torch.int64).unsqueeze(1) >> torch.arange(K, device=dev)) & 1       # [N, K]
    for g in range(G):
        at, feat = _stored_entries(b[g])
        r = vrow[g][at].long()
        ok = (r >= 0) & (r < N)
        at, feat, r = at[ok], feat[ok], r[ok]
        E = feat.numel()
        if E == 0:
            continue
        v = vval[g][at]
        head = torch.ones(E, dtype=torch.bool, device=dev)
        head[1:] = (feat[1:] != feat[:-1]) | (v[1:] != v[:-1])
        start = torch.nonzero(head).flatten()
        rid = torch.cumsum(head, 0) - 1
        end = torch.cat([start[1:], torch.tensor([E], device=dev)])
        first = torch.searchsorted(feat, feat)                        # where the entry's list starts
        p = bits[r]                                                   # [E, K]
        cn = torch.zeros(E + 1, K, dtype=torch.int64, device=dev)
        cn[1:] = torch.cumsum(1 - p, 0)
        term = p * (cn[start[rid]] + cn[end[rid]] - 2 * cn[first])
        pos_in[g].index_add_(0, feat, p)
        u2[g].index_add_(0, feat, term)
    return pos_in.to(torch.int32), u2


def auroc_dense_reference(dense: torch.Tensor, flags: torch.Tensor, n_concepts: int):
    """Brute force by the definition, O(N^2) per feature, for small cases: from dense codes [G, N, n] over all N
    rows, ``num2[g, f, k]`` = over the positive rows i and the negative rows j of concept k, ``2 [c_j < c_i] +
    [c_j == c_i]`` (int64 [G, n, K]), and the AUROC ``num2 / (2 P (N - P))`` in fp64 (NaN when P = 0 or P = N)."""
    K = check_concepts(n_concepts)
    G, N, n = dense.shape
    bits = (flags.to(torch.int64).unsqueeze(1) >> torch.arange(K, device=flags.device)) & 1   # [N, K]
    num2 = torch.zeros(G, n, K, dtype=torch.int64)
    for g in range(G):
        for f in range(n):
            c = dense[g, :, f]
            w = 2 * (c[None, :] < c[:, None]).long() + (c[None, :] == c[:, None]).long()      # [i, j]
            num2[g, f] = (bits * (w @ (1 - bits))).sum(0)
    P = bits.sum(0)
    den = 2 * P * (N - P)
    return num2, num2.double() / den.double().masked_fill(den == 0, float("nan"))


def _sorted_lists(fc):
    """Per (g, f) the list as Python tuples (key, row, value) in ``sorted()`` order."""
    ptr, keys = fc.host_ptr(), float_keys(fc.val).tolist()
    rows, vals = fc.row.tolist(), fc.val.tolist()
    return [[sorted(zip(keys[g][lo:hi], rows[g][lo:hi], vals[g][lo:hi]))
             for lo, hi in zip(ptr[g][:-1], ptr[g][1:])] for g in range(fc.n_models)]


def quantiles_reference(fc, Q: int) -> torch.Tensor:
    """``ValueOrdered.quantiles`` in plain Python loops over ``sorted()``, from lists in any order."""
    out = torch.full((fc.n_models, fc.n, Q + 1), float("nan"), dtype=torch.float32)
    for g, lists in enumerate(_sorted_lists(fc)):
        for f, items in enumerate(lists):
            for k in range(Q + 1 if items else 0):
                out[g, f, k] = items[(k * (len(items) - 1)) // Q][2]
    return out


def strata_reference(fc, n_strata: int, per_stratum: int):
    """``ValueOrdered.strata`` in plain Python loops over ``sorted()``, from lists in any order."""
    S, r = n_strata, per_stratum
    rows = torch.full((fc.n_models, fc.n, S, r), -1, dtype=torch.int32)
    vals = torch.zeros(fc.n_models, fc.n, S, r, dtype=torch.float32)
    for g, lists in enumerate(_sorted_lists(fc)):
        for f, items in enumerate(lists):
            L = len(items)
            for s in range(S):
                part = items[s * L // S:(s + 1) * L // S]
                m = len(part)
                picks = [part[(j * m) // r] for j in range(r)] if m >= r else part
                for j, (_, row, v) in enumerate(picks):
                    rows[g, f, s, j], vals[g, f, s, j] = row, v
    return rows, vals


# ---------------------------------------------------------------------- the routes
def by_value(fc: FeatureCodes, *, kernels: Optional[bool] = None, **kw) -> ValueOrdered:
    """``FeatureCodes.by_value``: the segmented sort of ``csrc/value_order.hip`` when the lists are on a GPU
    (keyword ``waves`` of ``ops.value_order.sort_lists``; never synchronises), ``sort_lists_reference`` elsewhere
    or with ``kernels=False``."""
    if fc.row.is_cuda if kernels is None else kernels:
        from ..ops import value_order as vo_ops

        vrow, vval = vo_ops.sort_lists(fc.col_ptr.contiguous(), fc.row, fc.val, **kw)
    else:
        if kw:
            raise TypeError(f"by_value: {sorted(kw)} are keywords of the device route")
        vrow, vval = sort_lists_reference(fc.col_ptr, fc.row, fc.val)
    return ValueOrdered(fc.n_rows, fc.n, fc.col_ptr, vrow, vval, fc.skipped)


def value_order(sparse_codes: SparseCodes, nactive=None, *, kernels: Optional[bool] = None) -> ValueOrdered:
    """``by_feature(nactive)`` then ``by_value()``: the kernels when the codes are on a GPU, the oracles elsewhere
    or with ``kernels=False``."""
    if sparse_codes.col.is_cuda if kernels is None else kernels:
        return by_value(by_feature(sparse_codes, nactive), kernels=True)
    return by_value(feature_codes_reference(sparse_codes, nactive), kernels=False)


def feature_auroc(sparse_codes: SparseCodes, flags: torch.Tensor, n_concepts=None, nactive=None, *,
                  kernels: Optional[bool] = None) -> FeatureAuroc:
    """The ``FeatureAuroc`` of the complete sparse codes ``sparse_codes`` against ``flags`` (``ValueOrdered.auroc``).
    Synchronises once (``SparseCodes.check()``: ``SparseCodesOverflow`` if entries were dropped).  A row the skip
    rule of ``by_feature`` leaves out counts as one on which no feature fires."""
    sparse_codes.check()
    return value_order(sparse_codes, nactive, kernels=kernels).auroc(flags, n_concepts, kernels=kernels)
