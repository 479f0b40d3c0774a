"""Sparse codes of an ensemble: the per-model CSR result type and its torch oracle.

``FusedSAEEnsemble.encode_sparse`` fills a ``SparseCodes`` from the bf16 codes of the grouped encoder
launch with the two streaming kernels of ``ops/sparse_codes.py``; ``FusedTopKEnsemble.encode_sparse``
builds the same object from the select's picks.  ``sparse_codes_reference`` computes it from any iterable
of dense code tensors in plain torch (CPU included) and is what the tests compare against.  An entry is
a strictly positive code; all fields are exact, so every comparison is ``torch.equal``.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, Optional, Sequence, Tuple

import torch


class SparseCodesOverflow(RuntimeError):
    """The buffers of a ``SparseCodes`` were too small: entries past ``cap`` were dropped."""


@dataclass
class SparseCodes:
    """Per-model CSR over the ``n_rows`` rows of one ``encode_sparse`` call, for G models with n features.

    Row ``i`` of model ``g`` holds the entries ``row_ptr[g, i] .. row_ptr[g, i + 1] - 1`` of ``col[g]`` /
    ``val[g]``, in ascending column order.  ``row_ptr`` always carries the TRUE counts: when the buffers
    were too small (``row_ptr[g, -1] > cap``) the entries at positions ``>= cap`` are missing, the kept
    prefix is exact, and ``overflow()`` / ``check()`` report it.  The unused tail of the buffers holds
    ``(0, 0.0)``."""

    n_rows: int
    n: int
    row_ptr: torch.Tensor   # int64 [G, n_rows + 1]
    col: torch.Tensor       # int32 [G, cap]
    val: torch.Tensor       # fp32 [G, cap]

    @property
    def cap(self) -> int:
        """Entries per model the buffers hold."""
        return int(self.col.shape[1])

    @property
    def n_models(self) -> int:
        return int(self.row_ptr.shape[0])

    # ------------------------------------------------------------------ counts and overflow
    def nnz(self) -> torch.Tensor:
        """True number of entries of every model, int64 [G] on the device (no synchronisation)."""
        return self.row_ptr[:, -1]

    def overflow(self) -> torch.Tensor:
        """bool [G] on the device: the model has more entries than the buffers hold."""
        return self.row_ptr[:, -1] > self.cap

    def check(self) -> "SparseCodes":
        """Synchronises; raises ``SparseCodesOverflow`` if any model lost entries."""
        over = self.overflow().cpu()
        if bool(over.any()):
            nnz = self.nnz().cpu().tolist()
            raise SparseCodesOverflow(f"sparse codes overflowed their buffers (cap = {self.cap} entries per model, "
                                      f"true counts {nnz}): encode with a larger budget, or budget=None")
        return self

    def _bounds(self, g: int) -> torch.Tensor:
        """Row pointers of model ``g`` clipped to the entries that are stored."""
        return self.row_ptr[g].clamp(max=self.cap)

    def entry_rows(self, g: int) -> torch.Tensor:
        """Row of every stored entry of model ``g``, int64 [stored]."""
        b = self._bounds(g)
        return torch.repeat_interleave(torch.arange(self.n_rows, device=b.device), b[1:] - b[:-1])

    # ------------------------------------------------------------------ views
    def row(self, g: int, i: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(cols int32, vals fp32) of row ``i`` of model ``g`` (the stored part of it)."""
        if not 0 <= i < self.n_rows:
            raise IndexError(f"row {i} outside [0, {self.n_rows})")
        lo, hi = (int(t) for t in self._bounds(g)[i:i + 2])
        return self.col[g, lo:hi], self.val[g, lo:hi]

    def to_dense(self, g: int, rows: slice = slice(None), dtype=torch.float32) -> torch.Tensor:
        """Dense codes [len(rows), n] of model ``g`` (``dtype`` fp32 or bf16; both hold the values exactly
        when the codes came from bf16 kernels)."""
        lo, hi, step = rows.indices(self.n_rows)
        if step != 1:
            raise ValueError("rows must be a contiguous slice")
        hi = max(hi, lo)
        b = self._bounds(g)
        e0, e1 = int(b[lo]), int(b[hi])
        r = self.entry_rows(g)[e0:e1] - lo
        out = torch.zeros(hi - lo, self.n, dtype=torch.float32, device=self.val.device)
        out[r, self.col[g, e0:e1].long()] = self.val[g, e0:e1]
        return out.to(dtype)

    def feature_entries(self, g: int, f: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(rows int64, vals fp32) on which feature ``f`` of model ``g`` fires, rows ascending."""
        if not 0 <= f < self.n:
            raise IndexError(f"feature {f} outside [0, {self.n})")
        stored = int(self._bounds(g)[-1])
        hit = self.col[g, :stored] == f
        return self.entry_rows(g)[hit], self.val[g, :stored][hit]

    def by_feature(self, nactive=None, **kw):
        """The feature-major transposition of these codes, an ``engine.feature_codes.FeatureCodes``: per model
        and feature the rows on which it fires, ascending, with their codes -- ``feature_entries`` for every
        feature at once, each a slice.  Rows whose entries are not all stored (overflowed buffers) or not valid
        (a column outside [0, n), or [0, ``nactive[g]``) for masked ensembles) are left out whole and counted in
        ``skipped``.  The kernels of ``csrc/feature_codes.hip`` when the tensors are on a GPU (never
        synchronises; ``kw``: their launch geometry), the torch oracle elsewhere."""
        from . import feature_codes as fc

        return fc.by_feature(self, nactive, **kw)

    def by_value(self, nactive=None):
        """``by_feature(nactive).by_value()``: every feature's list in value order, an
        ``engine.value_order.ValueOrdered`` with its ``quantiles``, ``histogram``, ``strata`` and ``auroc``."""
        return self.by_feature(nactive).by_value()

    def coactivation(self, other: Optional["SparseCodes"] = None, **kw):
        """The best co-activation partners of every feature of every model among the features of every model of
        ``other`` (default: these codes themselves), an ``engine.coactivation.CoActivation``: which features
        fire on the same rows, and how correlated their codes are (keywords ``m``, ``score``, ``min_both``,
        ``exclude_self``, ``nactive_a``, ``nactive_b`` of ``engine.coactivation.coactivation``).  Both sides
        cover the same rows.  The kernels of ``csrc/coactivation.hip`` when the tensors are on a GPU (never
        synchronises), the torch oracle elsewhere.  There is no ``state=``: a pool is given whole."""
        from . import coactivation as co

        return co.coactivation(self, other, **kw)

    def ridge_probes(self, flags: torch.Tensor, n_concepts=None, **kw):
        """Ridge probes on the whole code of every model for up to 32 concepts at once, an
        ``engine.probe.LinearProbes``: exactly ``RidgeClassifier(alpha)`` per (model, concept) -- weights,
        intercept, and the exact AUROC of the scores over the fit rows and the held-out rows.  ``flags``: int32
        words [n_rows] (bit k: the row is a positive of concept k) or a bool [n_rows, K] matrix (keywords
        ``alpha``, ``fit_rows``, ``max_iter``, ``tol``, ``nactive`` of ``engine.probe.ridge_probes``).  The kernels
        of ``csrc/probe.hip`` when the tensors are on a GPU, the torch oracle elsewhere."""
        from . import probe as pb

        return pb.ridge_probes(self, flags, n_concepts, **kw)

    def logistic_probes(self, flags: torch.Tensor, n_concepts=None, **kw):
        """Logistic-regression probes on the whole code of every model for up to 32 concepts at once, an
        ``engine.probe.LogisticProbes``: exactly ``LogisticRegression(C=C)`` per (model, concept) -- weights,
        intercept, and the exact AUROC of the logits over the fit rows and the held-out rows.  ``flags`` as in
        ``ridge_probes`` (keywords ``C``, ``fit_rows``, ``max_iter``, ``cg_iter``, ``tol``, ``early_stop``,
        ``nactive`` of ``engine.probe.logistic_probes``).  The kernels of ``csrc/probe.hip`` when the tensors are
        on a GPU, the torch oracle elsewhere."""
        from . import probe as pb

        return pb.logistic_probes(self, flags, n_concepts, **kw)

    def to_torch_csr(self, g: int) -> torch.Tensor:
        """Model ``g`` as a ``torch.sparse_csr_tensor`` [n_rows, n] (fp32 values, int64 indices)."""
        self.check()
        stored = int(self.row_ptr[g, -1])
        return torch.sparse_csr_tensor(self.row_ptr[g], self.col[g, :stored].long(), self.val[g, :stored],
                                       size=(self.n_rows, self.n))

    # ------------------------------------------------------------------ rows in, rows out
    def narrow_rows(self, lo: int, hi: int) -> "SparseCodes":
        """Rows ``lo .. hi - 1`` as a ``SparseCodes`` of their own (row pointers rebased, buffers sized to
        the largest model).  Synchronises; needs complete codes (``check()``)."""
        if not 0 <= lo <= hi <= self.n_rows:
            raise ValueError(f"rows [{lo}, {hi}) outside [0, {self.n_rows}]")
        self.check()
        G, dev = self.n_models, self.col.device
        start, end = self.row_ptr[:, lo], self.row_ptr[:, hi]
        cap = int((end - start).max()) if G else 0
        src = start.unsqueeze(1) + torch.arange(cap, device=dev)
        live = src < end.unsqueeze(1)
        src = torch.where(live, src, torch.zeros_like(src))
        col = torch.where(live, self.col.gather(1, src), torch.zeros((), dtype=torch.int32, device=dev)) \
            if cap else self.col[:, :0].clone()
        val = torch.where(live, self.val.gather(1, src), torch.zeros((), device=dev)) \
            if cap else self.val[:, :0].clone()
        return SparseCodes(hi - lo, self.n, (self.row_ptr[:, lo:hi + 1] - start.unsqueeze(1)).contiguous(),
                           col.contiguous(), val.contiguous())

    def take_rows(self, index: torch.Tensor, **kw) -> "SparseCodes":
        """Rows ``index`` (int64 [M], each in [0, n_rows), duplicates allowed) as a ``SparseCodes`` over M rows:
        row ``i`` of the result is row ``index[i]`` of these codes, columns and values copied bit for bit, in
        order.  The new ``row_ptr`` is a device cumsum of the gathered row lengths and ``cap`` is exactly the
        largest model's new entry count.  Needs complete codes; the one synchronisation is that of ``check()``
        (its host copy also carries the new counts and the index check).  The ``sc_csr_take_rows`` kernel of
        ``csrc/label_profile.hip`` when the tensors are on a GPU (``kw``: its ``waves``), ``take_rows_reference``
        elsewhere.  ``narrow_rows(lo, hi)`` equals ``take_rows(arange(lo, hi))``."""
        index = _check_index(index, self.row_ptr.device)
        if not self.col.is_cuda:
            if kw:
                raise TypeError(f"take_rows: {sorted(kw)} are keywords of the device route")
            return take_rows_reference(self, index)
        from ..ops import sparse_codes as sc_ops

        out_ptr, cap = _taken_row_ptr(self, index)
        col, val = sc_ops.take_rows(self.row_ptr.contiguous(), self.col, self.val, index, out_ptr, cap, **kw)
        return SparseCodes(int(index.shape[0]), self.n, out_ptr, col, val)

    def label_profile(self, labels: torch.Tensor, **kw):
        """Per feature of every model the labels that carry its activations, an
        ``engine.label_profile.LabelProfile``: ``labels`` int32 / int64 [n_rows] gives every row a label (a token
        id, a position, a concept; negative: the row is left out), and the profile holds per feature its ``m``
        best labels with their counts, fp64 sums and maxima, and the totals that turn them into shares,
        precision and recall (keywords ``m``, ``rank_by``, ``n_classes``, ``nactive`` of
        ``engine.label_profile.label_profile``).  The kernels of ``csrc/label_profile.hip`` when the tensors are
        on a GPU, the torch oracle elsewhere."""
        from . import label_profile as lp

        return lp.label_profile(self, labels, **kw)

    def attribution(self, D: torch.Tensor, x: torch.Tensor, **kw):
        """What every feature of every model does for the reconstruction of the rows ``x`` ([n_rows, d] shared or
        [G, n_rows, d], as the decoder sees them) from the unit-norm dictionaries ``D`` [G, n, d], an
        ``engine.attribution.Attribution``: the exact rise of the squared error when the feature is removed
        (``delta_sse``), the least-squares rescale of its codes and how often its firing makes a row worse
        (keywords ``nactive``, ``feature_codes``, ``state``, ``return_proj`` of ``engine.attribution.attribution``).
        The kernels of ``csrc/attribution.hip`` when the tensors are on a GPU (never synchronises), the torch
        oracle elsewhere."""
        from . import attribution as at

        return at.attribution(self, D, x, **kw)

    @classmethod
    def cat(cls, parts: Sequence["SparseCodes"]) -> "SparseCodes":
        """The rows of ``parts`` one after the other (same models, same width).  Synchronises; needs
        complete codes."""
        parts = list(parts)
        if not parts:
            raise ValueError("SparseCodes.cat needs at least one part")
        G, n, dev = parts[0].n_models, parts[0].n, parts[0].col.device
        for p in parts:
            if p.n_models != G or p.n != n:
                raise ValueError("SparseCodes.cat: parts of different ensembles")
            p.check()
        counts = torch.stack([p.nnz().to(dev) for p in parts])              # [P, G]
        offs = torch.cumsum(counts, 0) - counts                              # where each part's entries start
        total = counts.sum(0)
        cap = int(total.max())
        col = torch.zeros(G, cap, dtype=torch.int32, device=dev)
        val = torch.zeros(G, cap, dtype=torch.float32, device=dev)
        ptrs = [torch.zeros(G, 1, dtype=torch.int64, device=dev)]
        counts_h, offs_h = counts.tolist(), offs.tolist()
        for i, p in enumerate(parts):
            for g in range(G):
                k, o = counts_h[i][g], offs_h[i][g]
                col[g, o:o + k] = p.col[g, :k].to(dev)
                val[g, o:o + k] = p.val[g, :k].to(dev)
            ptrs.append(p.row_ptr[:, 1:].to(dev) + offs[i].unsqueeze(1))
        return cls(sum(p.n_rows for p in parts), n, torch.cat(ptrs, dim=1).contiguous(), col, val)

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        return {"n_rows": torch.tensor(int(self.n_rows), dtype=torch.int64),
                "n": torch.tensor(int(self.n), dtype=torch.int64),
                "row_ptr": self.row_ptr, "col": self.col, "val": self.val}

    def save(self, path):
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, map_location="cpu") -> "SparseCodes":
        sd = torch.load(path, map_location=map_location, weights_only=True)
        return cls(int(sd["n_rows"]), int(sd["n"]), sd["row_ptr"], sd["col"], sd["val"])

    def to(self, device) -> "SparseCodes":
        return SparseCodes(self.n_rows, self.n, self.row_ptr.to(device), self.col.to(device), self.val.to(device))


def _check_index(index, device) -> torch.Tensor:
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1:
        raise ValueError("index must be an int64 tensor [M]")
    return index.to(device).contiguous()


def _taken_row_ptr(sc: SparseCodes, index: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """``(row_ptr int64 [G, M + 1], cap)`` of ``sc.take_rows(index)``: the cumsum of the gathered row lengths on
    the device, and the largest model's new entry count.  One host copy carries the overflow flags of ``check()``,
    the new counts and the index check."""
    G, N, M, dev = sc.n_models, sc.n_rows, int(index.shape[0]), sc.row_ptr.device
    if N == 0 and M:
        raise IndexError("take_rows: codes without rows have no row to take")
    safe = index.clamp(0, max(N - 1, 0))
    bad = ((index < 0) | (index >= N)).any().to(torch.int64).view(1)
    out_ptr = torch.zeros(G, M + 1, dtype=torch.int64, device=dev)
    out_ptr[:, 1:] = torch.cumsum(sc.row_ptr[:, safe + 1] - sc.row_ptr[:, safe], 1)
    host = torch.cat([sc.row_ptr[:, -1], out_ptr[:, -1], bad]).cpu()   # the one synchronisation
    if bool((host[:G] > sc.cap).any()):
        sc.check()   # raises SparseCodesOverflow
    if int(host[-1]):
        raise IndexError(f"take_rows: index values must lie in [0, {N})")
    return out_ptr, (int(host[G:2 * G].max()) if G else 0)


def take_rows_reference(sc: SparseCodes, index: torch.Tensor) -> SparseCodes:
    """Torch oracle of ``SparseCodes.take_rows`` (any device; this is what runs off the GPU)."""
    index = _check_index(index, sc.row_ptr.device)
    out_ptr, cap = _taken_row_ptr(sc, index)
    G, dev = sc.n_models, sc.row_ptr.device
    col = torch.zeros(G, cap, dtype=torch.int32, device=dev)
    val = torch.zeros(G, cap, dtype=torch.float32, device=dev)
    for g in range(G):
        ln = out_ptr[g, 1:] - out_ptr[g, :-1]
        k = int(out_ptr[g, -1])
        src = torch.repeat_interleave(sc.row_ptr[g, index] - out_ptr[g, :-1], ln) + torch.arange(k, device=dev)
        col[g, :k] = sc.col[g][src]
        val[g, :k] = sc.val[g][src]
    return SparseCodes(int(index.shape[0]), sc.n, out_ptr, col, val)


def check_budget(budget, n_rows: int, n: int) -> Optional[int]:
    """Entries per model for ``budget`` entries per row (``None`` stays ``None``: size exactly)."""
    if budget is None:
        return None
    if isinstance(budget, bool) or int(budget) != budget or int(budget) < 0:
        raise ValueError(f"budget must be a non-negative integer number of entries per row or None, got {budget!r}")
    return min(n_rows * int(budget), n_rows * n)


def sparse_codes_reference(code_batches: Iterable[torch.Tensor], cap: Optional[int] = None) -> SparseCodes:
    """Torch oracle: the ``SparseCodes`` of the dense code tensors ``code_batches`` (each [G, B, n], any
    float dtype, B may vary), from ``nonzero`` on ``c > 0`` in row-major order.  ``cap``: entries per
    model the buffers hold (default: the largest model's count); entries at positions ``>= cap`` are
    dropped and ``row_ptr`` keeps the true counts."""
    cols, vals, counts = None, None, []
    n_rows = 0
    G = n = dev = None
    for c in code_batches:
        if c.dim() != 3:
            raise ValueError(f"codes must be [G, B, n], got {tuple(c.shape)}")
        if G is None:
            G, _, n = c.shape
            dev = c.device
            cols, vals = [[] for _ in range(G)], [[] for _ in range(G)]
        elif c.shape[0] != G or c.shape[2] != n:
            raise ValueError("batches of different ensembles")
        pos = c > 0
        counts.append(pos.sum(-1, dtype=torch.int64))
        for g in range(G):
            cols[g].append(torch.nonzero(pos[g])[:, 1].to(torch.int32))  # (row-major: rows, then columns ascending)
            vals[g].append(c[g][pos[g]].float())
        n_rows += c.shape[1]
    if G is None:
        raise ValueError("sparse_codes_reference needs at least one batch of codes")
    counts = torch.cat(counts, dim=1)
    row_ptr = torch.zeros(G, n_rows + 1, dtype=torch.int64, device=dev)
    row_ptr[:, 1:] = torch.cumsum(counts, 1)
    if cap is None:
        cap = int(row_ptr[:, -1].max())
    cap = int(cap)
    if cap < 0:
        raise ValueError(f"cap must be >= 0, got {cap}")
    col = torch.zeros(G, cap, dtype=torch.int32, device=dev)
    val = torch.zeros(G, cap, dtype=torch.float32, device=dev)
    for g in range(G):
        cg, vg = torch.cat(cols[g])[:cap], torch.cat(vals[g])[:cap]
        col[g, :cg.numel()] = cg
        val[g, :vg.numel()] = vg
    return SparseCodes(n_rows, n, row_ptr, col, val)


def sparse_codes_from_picks(batches, k, n: int, cap: Optional[int] = None):
    """The ``SparseCodes`` of top-k picks: ``batches`` yields (idx int [G, B, kmax], val fp32 [G, B, kmax])
    per batch, slots at or past ``k[g]`` are padding.  A pick is an entry when its value is positive; each
    row's entries are sorted by column with torch ops on the pick buffers (no dense codes).  With ``cap``
    given nothing here synchronises; entries at positions ``>= cap`` are dropped.  ``cap=None``: the
    batches are walked once, one synchronisation reads the totals, and the buffers are sized exactly.
    Equals ``sparse_codes_reference`` on ``engine.topk_stats.dense_codes_from_picks`` of the same picks."""
    rows_keys, rows_vals, rows_cnt = [], [], []
    for idx, val in batches:
        G, B, kmax = idx.shape
        dev = idx.device
        kk = torch.as_tensor(k, device=dev).reshape(-1)
        keep = (torch.arange(kmax, device=dev).view(1, 1, kmax) < kk.view(G, 1, 1)) & (val > 0)
        key = torch.where(keep, idx.to(torch.int32), torch.full((), n, dtype=torch.int32, device=dev))
        key, order = torch.sort(key, dim=-1, stable=True)          # kept picks first, by column
        rows_keys.append(key)
        rows_vals.append(torch.gather(val.float(), -1, order))
        rows_cnt.append(keep.sum(-1, dtype=torch.int64))
    if not rows_keys:
        raise ValueError("sparse_codes_from_picks needs at least one batch of picks")
    key, v, cnt = torch.cat(rows_keys, 1), torch.cat(rows_vals, 1), torch.cat(rows_cnt, 1)
    G, N, kmax = key.shape
    dev = key.device
    row_ptr = torch.zeros(G, N + 1, dtype=torch.int64, device=dev)
    row_ptr[:, 1:] = torch.cumsum(cnt, 1)
    if cap is None:
        cap = int(row_ptr[:, -1].max())  # the one synchronisation
    slot = torch.arange(kmax, device=dev)
    dest = row_ptr[:, :-1].unsqueeze(-1) + slot
    live = (slot < cnt.unsqueeze(-1)) & (dest < cap)
    dest = torch.where(live, dest, torch.full((), cap, dtype=torch.int64, device=dev)).reshape(G, -1)
    # dropped and padding slots all land in one spare position past the buffers, cut off below
    col = torch.zeros(G, cap + 1, dtype=torch.int32, device=dev).scatter_(1, dest, key.reshape(G, -1))
    out = torch.zeros(G, cap + 1, dtype=torch.float32, device=dev).scatter_(1, dest, v.reshape(G, -1))
    return SparseCodes(N, n, row_ptr, col[:, :cap].contiguous(), out[:, :cap].contiguous())
