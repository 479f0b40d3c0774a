"""Python front-end for the per-feature kernels over top-k picks (``csrc/topk_stats.hip``)."""

from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .topk import SlotLists

MAX_TOPK = 32


def _picks(idx: torch.Tensor, val: torch.Tensor, k: torch.Tensor, what: str):
    if idx.dim() != 3 or idx.dtype != torch.int32 or not idx.is_contiguous():
        raise ValueError(f"{what} needs contiguous int32 picks idx [G, B, kmax]")
    G, B, kmax = idx.shape
    if val.dtype != torch.float32 or tuple(val.shape) != (G, B, kmax) or not val.is_contiguous() \
            or val.device != idx.device:
        raise ValueError(f"{what}: val must be contiguous fp32 [{G}, {B}, {kmax}] on the picks' device")
    if k.dtype != torch.int32 or k.numel() != G or not k.is_contiguous() or k.device != idx.device:
        raise ValueError(f"{what}: k must be int32 [{G}] on the picks' device")
    if G < 1 or B < 1 or kmax < 1:
        raise ValueError(f"{what} needs G, B, kmax >= 1 (got {G}, {B}, {kmax})")
    return G, B, kmax


def pick_counts(idx: torch.Tensor, val: torch.Tensor, k: torch.Tensor, counts: torch.Tensor,
                step_dev: Optional[torch.Tensor] = None, every: int = 0) -> torch.Tensor:
    """counts int64 [G, n] += the fire counts of the picks ``idx`` / ``val`` [G, B, kmax] with per-model
    ``k`` (int32 [G]): slot s of a row counts for feature idx[g, b, s] iff s < min(k[g], kmax) and
    val > 0 (a pick clamped to 0 by the ReLU is not a firing; the padded slots never count).  Exact
    (integer adds).  ``step_dev`` (device int32 [1]) with ``every`` > 0: the launch does nothing unless
    ``step_dev % every == 0``, decided on the device.  Nothing here synchronises; graph-capturable."""
    G, B, kmax = _picks(idx, val, k, "pick_counts")
    if counts.dim() != 2 or counts.shape[0] != G or counts.dtype != torch.int64 or not counts.is_contiguous() \
            or counts.device != idx.device:
        raise ValueError(f"counts must be contiguous int64 [{G}, n] on the picks' device")
    n = counts.shape[1]
    if not 1 <= n <= 32768:
        raise ValueError(f"pick_counts needs 1 <= n <= 32768 (got {n})")
    every = int(every)
    if every < 0:
        raise ValueError(f"every must be >= 0 (got {every})")
    if step_dev is not None and (step_dev.dtype != torch.int32 or step_dev.numel() != 1
                                 or step_dev.device != idx.device):
        raise ValueError("step_dev must be an int32 scalar on the picks' device")
    rc = _lib.lib().sc_topk_pick_counts(_lib.ptr(idx), _lib.ptr(val), _lib.ptr(k), _lib.ptr(counts), G, B, n, kmax,
                                        _lib.ptr(step_dev), every, _lib.stream_handle())
    _lib.check(rc, "sc_topk_pick_counts")
    return counts


def pick_stats(lists: SlotLists, val: torch.Tensor, acc: torch.Tensor, mx: torch.Tensor,
               top_vals: Optional[torch.Tensor], top_rows: Optional[torch.Tensor], row0: int):
    """Fold one batch of picks into the running per-feature statistics, in place.  ``lists``: the sorted
    slot lists of ALL G models of the batch (``SlotLists(G, ...)`` after ``slot_lists``); ``val`` fp32
    [G, B, kmax] the picked values; only ``val > 0`` entries take part.  ``acc`` fp64 [G, 5, n]: the count
    and the sums of c .. c^4; ``mx`` fp32 [G, n]: max(mx, 0, largest value); ``top_vals`` fp32 /
    ``top_rows`` int64 [G, n, K] (1 <= K <= 32, or both None): the running top-K lists under ``col_topk``'s
    contract (value descending then row ascending, strictly positive values, empty slots (0.0, -1));
    the batch's global rows are ``row0 .. row0 + B - 1`` and batches must come in increasing ``row0``.
    Bit-reproducible (no floating-point atomics); nothing here synchronises; graph-capturable."""
    G, B, n, kmax = lists.Gs, lists.B, lists.n, lists.kmax
    dev = lists.perm.device
    if val.dtype != torch.float32 or tuple(val.shape) != (G, B, kmax) or not val.is_contiguous() or val.device != dev:
        raise ValueError(f"val must be contiguous fp32 [{G}, {B}, {kmax}] on the lists' device")
    if acc.dtype != torch.float64 or tuple(acc.shape) != (G, 5, n) or not acc.is_contiguous() or acc.device != dev:
        raise ValueError(f"acc must be contiguous fp64 [{G}, 5, {n}] on the lists' device")
    if mx.dtype != torch.float32 or tuple(mx.shape) != (G, n) or not mx.is_contiguous() or mx.device != dev:
        raise ValueError(f"mx must be contiguous fp32 [{G}, {n}] on the lists' device")
    K = 0
    if (top_vals is None) != (top_rows is None):
        raise ValueError("top_vals and top_rows go together")
    if top_vals is not None:
        if top_vals.dim() != 3:
            raise ValueError(f"top_vals must be fp32 [{G}, {n}, K]")
        K = top_vals.shape[2]
        if not 1 <= K <= MAX_TOPK:
            raise ValueError(f"pick_stats needs 1 <= K <= {MAX_TOPK} (got {K})")
        for name, t, dt in (("top_vals", top_vals, torch.float32), ("top_rows", top_rows, torch.int64)):
            if t.dtype != dt or tuple(t.shape) != (G, n, K) or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{name} must be contiguous {dt} [{G}, {n}, {K}] on the lists' device")
    row0 = int(row0)
    if row0 < 0:
        raise ValueError(f"row0 must be >= 0 (got {row0})")
    rc = _lib.lib().sc_topk_pick_stats(_lib.ptr(lists.perm), _lib.ptr(lists.offs), _lib.ptr(val), _lib.ptr(acc),
                                       _lib.ptr(mx), _lib.ptr(top_vals), _lib.ptr(top_rows), G, B, n, kmax, K, row0,
                                       lists.perm.numel(), _lib.stream_handle())
    _lib.check(rc, "sc_topk_pick_stats")
