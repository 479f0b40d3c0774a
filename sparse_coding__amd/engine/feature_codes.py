"""Feature-major sparse codes of an ensemble and the example fragments of every feature: the result types,
their torch oracles and the device route.

``SparseCodes.by_feature()`` transposes the per-model CSR into a ``FeatureCodes``: per model and feature the
rows on which the feature fires, ascending, with their codes (``ops.feature_codes.by_feature``,
``csrc/feature_codes.hip``, on a GPU; ``feature_codes_reference`` elsewhere).  With the rows read as
fragments of ``fragment_len`` consecutive rows (token ``i % L`` of fragment ``i // L``),
``FeatureCodes.fragment_examples`` picks per feature the fragments with the largest maximum code and a
hash sample of the fragments on which it fires, and ``FeatureCodes.fragment_acts`` gathers their activation
records: what auto-interpretation needs, without a dense code tensor.

All outputs are integers, copies of fp32 values or maxima of them: the oracles compare with ``torch.equal``.

- **Skip rule** (that of ``ops.interference.active_capacity``): a row is left out whole and counted in
  ``skipped[g]`` unless ``0 <= row_ptr[r] <= row_ptr[r + 1] <= cap``, it has at most n entries and every
  column lies in ``[0, lim)``, lim = n or ``min(n, nactive[g])``.
- **Top fragments**: maximum descending, then fragment ascending; empty slots ``(-1, 0.0)``.  Codes are
  positive.
- **Random fragments**: the active fragments with the smallest ``key = mix32(h0 ^ uint32(frag))``,
  ``h0 = mix32(uint32(seed) + 0x9E3779B9 * uint32(g n + f + 1))``, key ascending, empty slots ``-1``.
  ``mix32`` is a bijection of uint32, so the order within a feature is strict, the first k slots are a sample
  of size k, and a list with at most ``n_random`` active fragments returns all of them.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from ..ops.feature_codes import MAX_K, check_fragments, check_k   # (plain Python: no kernel library is loaded)
from .interference import live_counts
from .sparse_codes import SparseCodes

_M32 = 0xFFFFFFFF


class FeatureCodesSkipped(RuntimeError):
    """Rows were left out of a ``FeatureCodes`` (their entries were not all stored, or not valid), or its
    buffers were too small for the entries of the rows that passed."""


# ---------------------------------------------------------------------- the hash
def _mul32(x: torch.Tensor, c: int) -> torch.Tensor:
    """``x * c mod 2^32`` for int64 ``x`` in [0, 2^32), without leaving the int64 range."""
    lo = (x & 0xFFFF) * c
    hi = (((x >> 16) * c) & 0xFFFF) << 16
    return (lo + hi) & _M32


def mix32(x: torch.Tensor) -> torch.Tensor:
    """The 32-bit mixer of the random-fragment sample on int64 tensors holding uint32 values."""
    x = x & _M32
    x = (x ^ (x >> 16)) & _M32
    x = _mul32(x, 0x7FEB352D)
    x = (x ^ (x >> 15)) & _M32
    x = _mul32(x, 0x846CA68B)
    x = (x ^ (x >> 16)) & _M32
    return x


def fragment_keys(list_id: torch.Tensor, frag: torch.Tensor, seed: int = 0) -> torch.Tensor:
    """Sample keys (int64 holding uint32) of the fragments ``frag`` for the lists ``list_id = g * n + f``."""
    h0 = mix32((int(seed) & _M32) + _mul32((list_id.to(torch.int64) + 1) & _M32, 0x9E3779B9))
    return mix32((h0 ^ (frag.to(torch.int64) & _M32)) & _M32)


# ---------------------------------------------------------------------- result types
@dataclass
class FragmentExamples:
    """Example fragments of every feature of G models: what ``FeatureCodes.fragment_examples`` returns."""

    n_frags: torch.Tensor     # int64 [G, n]       distinct fragments on which the feature fires
    top_frag: torch.Tensor    # int32 [G, n, Kt]   largest maximum first, then the lower fragment; -1: empty
    top_max: torch.Tensor     # fp32 [G, n, Kt]    their maxima; 0.0: empty
    rand_frag: torch.Tensor   # int32 [G, n, Kr]   the hash sample, key ascending; -1: empty
    fragment_len: int
    seed: int

    def to(self, device) -> "FragmentExamples":
        return FragmentExamples(self.n_frags.to(device), self.top_frag.to(device), self.top_max.to(device),
                                self.rand_frag.to(device), self.fragment_len, self.seed)


@dataclass
class FeatureCodes:
    """Feature-major (CSC) codes of G models with n features over ``n_rows`` rows.

    The list of feature ``f`` of model ``g`` is ``row/val[g, col_ptr[g, f] : col_ptr[g, f + 1]]``, rows
    ascending.  ``col_ptr`` carries the true counts of the rows that passed the skip rule; entries at positions
    past the buffers are missing (``check()`` reports it).  The unused tail holds ``(0, 0.0)``."""

    n_rows: int
    n: int
    col_ptr: torch.Tensor   # int64 [G, n + 1]
    row: torch.Tensor       # int32 [G, cap]
    val: torch.Tensor       # fp32 [G, cap]
    skipped: torch.Tensor   # int64 [G]  rows left out by the skip rule

    @property
    def cap(self) -> int:
        return int(self.row.shape[1])

    @property
    def n_models(self) -> int:
        return int(self.col_ptr.shape[0])

    def counts(self) -> torch.Tensor:
        """Entries of every feature, int64 [G, n] on the device (no synchronisation)."""
        return self.col_ptr[:, 1:] - self.col_ptr[:, :-1]

    def check(self) -> "FeatureCodes":
        """Synchronises; raises ``FeatureCodesSkipped`` if any row was skipped or any entry dropped."""
        sk = self.skipped.cpu()
        if bool((sk != 0).any()):
            raise FeatureCodesSkipped(f"{sk.tolist()} rows per model were skipped (of {self.n_rows}): their sparse "
                                      "codes were not all stored -- encode with a larger budget, or budget=None")
        tot = self.col_ptr[:, -1].cpu()
        if bool((tot > self.cap).any()):
            raise FeatureCodesSkipped(f"the buffers hold {self.cap} entries per model, the lists {tot.tolist()}")
        return self

    def feature(self, g: int, f: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(rows int64, vals fp32) on which feature ``f`` of model ``g`` fires, rows ascending: a slice of the
        stored lists (what ``SparseCodes.feature_entries`` computes with a scan).  The first call copies
        ``col_ptr`` to the host (one synchronisation) and keeps the copy; ``host_ptr(refresh=True)`` reads it
        again after the buffers were refilled in place."""
        if not 0 <= f < self.n:
            raise IndexError(f"feature {f} outside [0, {self.n})")
        lo, hi = self.host_ptr()[g][f:f + 2]
        return self.row[g, lo:hi].long(), self.val[g, lo:hi]

    def host_ptr(self, refresh: bool = False):
        """``col_ptr`` clipped to the stored entries, as nested lists on the host (cached)."""
        if refresh or getattr(self, "_host_ptr", None) is None:
            b = self.col_ptr.clamp(min=0, max=self.cap)
            self._host_ptr = torch.cummax(b, 1).values.tolist()
        return self._host_ptr

    def entry_features(self, g: int) -> torch.Tensor:
        """Feature of every stored entry of model ``g``, int64 [stored]."""
        b = self.col_ptr[g].clamp(min=0, max=self.cap)
        return torch.repeat_interleave(torch.arange(self.n, device=b.device), (b[1:] - b[:-1]).clamp(min=0))

    def to_sparse_codes(self) -> SparseCodes:
        """The row-major ``SparseCodes`` these lists came from (buffers of the same size).  Synchronises."""
        G, dev, cap = self.n_models, self.row.device, self.cap
        row_ptr = torch.zeros(G, self.n_rows + 1, dtype=torch.int64, device=dev)
        col = torch.zeros(G, cap, dtype=torch.int32, device=dev)
        val = torch.zeros(G, cap, dtype=torch.float32, device=dev)
        for g in range(G):
            feats = self.entry_features(g)
            k = feats.numel()
            rows = self.row[g, :k].long()
            order = torch.sort(rows, stable=True).indices   # (features ascending inside a row: the lists' order)
            row_ptr[g, 1:] = torch.cumsum(torch.bincount(rows, minlength=self.n_rows), 0)
            col[g, :k] = feats[order].to(torch.int32)
            val[g, :k] = self.val[g, :k][order]
        return SparseCodes(self.n_rows, self.n, row_ptr, col, val)

    # ------------------------------------------------------------------ example fragments
    def fragment_examples(self, fragment_len: int = 64, n_top: int = 20, n_random: int = 20,
                          seed: int = 0) -> FragmentExamples:
        """Per feature the ``n_top`` fragments with the largest maximum code and a hash sample of ``n_random``
        fragments on which it fires (module docstring), rows read as fragments of ``fragment_len``.  One kernel
        launch on a GPU (``ops.feature_codes.fragment_examples``, never synchronises), the oracle elsewhere."""
        if self.row.is_cuda:
            from ..ops import feature_codes as fc_ops

            out = fc_ops.fragment_examples(self.col_ptr, self.row, self.val, self.n_rows, fragment_len, n_top,
                                           n_random, seed)
            return FragmentExamples(*out, int(fragment_len), int(seed))
        return fragment_examples_reference(self, fragment_len, n_top, n_random, seed)

    def fragment_acts(self, frags: torch.Tensor, features: slice = slice(None), fragment_len: int = 64
                      ) -> torch.Tensor:
        """Activation records fp32 [G, F, K, L] of the features ``features`` (a contiguous slice, F of them) on
        the fragments ``frags`` int32 [G, F, K]: the feature's code on every row of the fragment, 0 where it does
        not fire, all zeros for a slot of -1 or a fragment that does not exist."""
        f0, f1, step = features.indices(self.n)
        if step != 1:
            raise ValueError("features must be a contiguous slice")
        f1 = max(f1, f0)
        if frags.dim() != 3 or frags.shape[1] != f1 - f0:
            raise ValueError(f"frags must be int32 [G, {f1 - f0}, K], got {tuple(frags.shape)}")
        if self.row.is_cuda:
            from ..ops import feature_codes as fc_ops

            return fc_ops.fragment_acts(self.col_ptr, self.row, self.val, self.n_rows, fragment_len,
                                        frags.contiguous(), f0)
        return fragment_acts_reference(self, fragment_len, frags, f0)

    def by_value(self, **kw):
        """These lists in value order, an ``engine.value_order.ValueOrdered``: every list ordered by the key of
        its codes ascending, then row ascending, at its own positions -- what quantiles, strata, histograms and
        the per-feature AUROC are read from.  One launch of the segmented sort of ``csrc/value_order.hip`` on a
        GPU (``kw``: its ``waves``; never synchronises), the oracle elsewhere."""
        from . import value_order as vo

        return vo.by_value(self, **kw)

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        return {"n_rows": torch.tensor(int(self.n_rows), dtype=torch.int64),
                "n": torch.tensor(int(self.n), dtype=torch.int64),
                "col_ptr": self.col_ptr, "row": self.row, "val": self.val, "skipped": self.skipped}

    def save(self, path):
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, map_location="cpu") -> "FeatureCodes":
        sd = torch.load(path, map_location=map_location, weights_only=True)
        return cls(int(sd["n_rows"]), int(sd["n"]), sd["col_ptr"], sd["row"], sd["val"], sd["skipped"])

    def to(self, device) -> "FeatureCodes":
        return FeatureCodes(self.n_rows, self.n, self.col_ptr.to(device), self.row.to(device), self.val.to(device),
                            self.skipped.to(device))


# ---------------------------------------------------------------------- checks
def _check_codes(sc: SparseCodes):
    if sc.row_ptr.dtype != torch.int64 or sc.col.dtype != torch.int32 or sc.val.dtype != torch.float32:
        raise ValueError(f"sparse codes must be (int64, int32, fp32), got ({sc.row_ptr.dtype}, {sc.col.dtype}, "
                         f"{sc.val.dtype})")
    if sc.n_rows >= 2 ** 31 or sc.cap >= 2 ** 31:
        raise ValueError(f"by_feature needs N < 2^31 and cap < 2^31 (got N={sc.n_rows}, cap={sc.cap})")


# ---------------------------------------------------------------------- oracles
def feature_codes_reference(sparse_codes: SparseCodes, nactive=None, cap_out: Optional[int] = None) -> FeatureCodes:
    """Torch oracle of the transposition (any device): the entries of the rows that pass the skip rule, in a
    stable ``torch.sort`` on their column.  ``cap_out``: entries per model the buffers hold (default: those of
    ``sparse_codes``); entries at positions ``>= cap_out`` are dropped and ``col_ptr`` keeps the true counts."""
    sc = sparse_codes
    _check_codes(sc)
    G, n, N, cap, dev = sc.n_models, sc.n, sc.n_rows, sc.cap, sc.col.device
    cap_out = cap if cap_out is None else int(cap_out)
    if cap_out < 0:
        raise ValueError(f"cap_out must be >= 0, got {cap_out}")
    live = live_counts(nactive, G, n, dev)
    lim = [n] * G if live is None else live.tolist()
    col_ptr = torch.zeros(G, n + 1, dtype=torch.int64, device=dev)
    row = torch.zeros(G, cap_out, dtype=torch.int32, device=dev)
    val = torch.zeros(G, cap_out, dtype=torch.float32, device=dev)
    skipped = torch.zeros(G, dtype=torch.int64, device=dev)
    for g in range(G):
        lo, hi = sc.row_ptr[g, :-1], sc.row_ptr[g, 1:]
        ok = (lo >= 0) & (hi >= lo) & (hi <= cap) & (hi - lo <= n)
        r = torch.nonzero(ok).flatten()
        ln = (hi - lo)[r]
        start = torch.cumsum(ln, 0) - ln
        rows = torch.repeat_interleave(r, ln)
        e = torch.repeat_interleave(lo[r] - start, ln) + torch.arange(int(ln.sum()), device=dev)
        cols = sc.col[g][e].long()
        bad = torch.zeros(N, dtype=torch.bool, device=dev)
        bad[rows[(cols < 0) | (cols >= lim[g])]] = True   # one bad column condemns the whole row
        ok &= ~bad
        keep = ~bad[rows]
        rows, e, cols = rows[keep], e[keep], cols[keep]
        skipped[g] = N - int(ok.sum())
        order = torch.sort(cols, stable=True).indices
        col_ptr[g, 1:] = torch.cumsum(torch.bincount(cols, minlength=n), 0)
        k = min(int(order.numel()), cap_out)
        row[g, :k] = rows[order][:k].to(torch.int32)
        val[g, :k] = sc.val[g][e[order][:k]]
    return FeatureCodes(N, n, col_ptr, row, val, skipped)


def _place(feat, value, n, K, fill, dtype):
    """``out[f, j]`` = the j-th of the (already ordered) values of feature f, j < K; ``fill`` elsewhere."""
    out = torch.full((n, K), fill, dtype=dtype, device=feat.device)
    first = torch.cumsum(torch.bincount(feat, minlength=n), 0) - torch.bincount(feat, minlength=n)
    pos = torch.arange(feat.numel(), device=feat.device) - first[feat]
    sel = pos < K
    out[feat[sel], pos[sel]] = value[sel].to(dtype)
    return out


def fragment_examples_reference(fc: FeatureCodes, fragment_len: int = 64, n_top: int = 20, n_random: int = 20,
                                seed: int = 0) -> FragmentExamples:
    """Torch oracle of ``ops.feature_codes.fragment_examples`` (any device): per (feature, fragment) the maximum
    of the stored entries, then stable sorts for the two orders.  The hash is computed in int64."""
    n_frag = check_fragments(fc.n_rows, fragment_len)
    L, Kt, Kr = int(fragment_len), check_k("n_top", n_top), check_k("n_random", n_random)
    G, n, dev = fc.n_models, fc.n, fc.row.device
    n_frags = torch.zeros(G, n, dtype=torch.int64, device=dev)
    top_frag = torch.full((G, n, Kt), -1, dtype=torch.int32, device=dev)
    top_max = torch.zeros(G, n, Kt, dtype=torch.float32, device=dev)
    rand_frag = torch.full((G, n, Kr), -1, dtype=torch.int32, device=dev)
    for g in range(G):
        feats = fc.entry_features(g)
        k = feats.numel()
        frag = fc.row[g, :k].long() // L
        pair, inv = torch.unique(feats * max(n_frag, 1) + frag, return_inverse=True)   # (sorted: feature, fragment)
        mx = torch.full((pair.numel(),), float("-inf"), device=dev).scatter_reduce(0, inv, fc.val[g, :k], "amax")
        pf, pfrag = pair // max(n_frag, 1), pair % max(n_frag, 1)
        n_frags[g] = torch.bincount(pf, minlength=n)
        o = torch.sort(mx, descending=True, stable=True).indices      # fragments stay ascending among equals
        o = o[torch.sort(pf[o], stable=True).indices]
        top_frag[g] = _place(pf[o], pfrag[o], n, Kt, -1, torch.int32)
        top_max[g] = _place(pf[o], mx[o], n, Kt, 0.0, torch.float32)
        key = fragment_keys(g * n + pf, pfrag, seed)
        o = torch.sort(key, stable=True).indices
        o = o[torch.sort(pf[o], stable=True).indices]
        rand_frag[g] = _place(pf[o], pfrag[o], n, Kr, -1, torch.int32)
    return FragmentExamples(n_frags, top_frag, top_max, rand_frag, L, int(seed))


def fragment_acts_reference(fc: FeatureCodes, fragment_len: int, frags: torch.Tensor, f0: int = 0) -> torch.Tensor:
    """Torch oracle of ``ops.feature_codes.fragment_acts`` (any device): ``out[g, f, k, t]`` is the code of
    feature ``f0 + f`` on row ``frags[g, f, k] * L + t``, looked up in the stored lists."""
    n_frag = check_fragments(fc.n_rows, fragment_len)
    L, G, N, dev = int(fragment_len), fc.n_models, fc.n_rows, fc.row.device
    if frags.dim() != 3 or frags.shape[0] != G or frags.dtype != torch.int32:
        raise ValueError(f"frags must be int32 [{G}, features, K], got {frags.dtype} {tuple(frags.shape)}")
    nf, K = frags.shape[1:]
    if f0 < 0 or f0 + nf > fc.n:
        raise ValueError(f"features [{f0}, {f0 + nf}) outside [0, {fc.n}]")
    out = torch.zeros(G, nf, K, L, dtype=torch.float32, device=dev)
    fr = frags.to(dev).long()
    for g in range(G):
        feats = fc.entry_features(g)
        k = feats.numel()
        if k == 0:
            continue
        have = feats * N + fc.row[g, :k].long()       # ascending: features, then rows
        live = (fr[g] >= 0) & (fr[g] < n_frag)
        want = (torch.arange(f0, f0 + nf, device=dev).view(nf, 1, 1) * N + fr[g].clamp(0).unsqueeze(-1) * L
                + torch.arange(L, device=dev))
        at = torch.searchsorted(have, want.reshape(-1)).clamp(max=k - 1).view(nf, K, L)
        hit = (have[at] == want) & live.unsqueeze(-1)
        out[g] = torch.where(hit, fc.val[g, :k][at], torch.zeros((), device=dev))
    return out


# ---------------------------------------------------------------------- the routes
def by_feature(sparse_codes: SparseCodes, nactive=None, **kw) -> FeatureCodes:
    """``SparseCodes.by_feature``: the kernels when the codes are on a GPU (keywords ``segment_rows``,
    ``lds_bins``, ``rows_per_block`` of ``ops.feature_codes.by_feature``; never synchronises), the oracle
    elsewhere."""
    sc = sparse_codes
    _check_codes(sc)
    if not sc.col.is_cuda:
        if kw:
            raise TypeError(f"by_feature: {sorted(kw)} are keywords of the device route")
        return feature_codes_reference(sc, nactive)
    from ..ops import feature_codes as fc_ops

    live = live_counts(nactive, sc.n_models, sc.n, sc.col.device)
    col_ptr, row, val, skipped = fc_ops.by_feature(sc.row_ptr.contiguous(), sc.col, sc.val, sc.n, nactive=live, **kw)
    return FeatureCodes(sc.n_rows, sc.n, col_ptr, row, val, skipped)


def feature_examples(sparse_codes: SparseCodes, nactive=None, fragment_len: int = 64, n_top: int = 20,
                     n_random: int = 20, seed: int = 0):
    """(``FeatureCodes``, ``FragmentExamples``) of ``sparse_codes``: what the engines' ``feature_examples``
    return after their ``encode_sparse``."""
    check_fragments(sparse_codes.n_rows, fragment_len)
    fc = by_feature(sparse_codes, nactive)
    return fc, fc.fragment_examples(fragment_len, n_top, n_random, seed)
