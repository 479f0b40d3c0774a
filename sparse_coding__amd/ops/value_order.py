"""Python front-end for the value-order kernels (``csrc/value_order.hip``)."""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._args import INT32_MAX, WAVES, _buffer, _lists, check_waves, out_buffers  # noqa: F401 (WAVES is public)

MAX_CONCEPTS = 32         # concepts per flag word: one per bit of an int32


def check_concepts(n_concepts) -> int:
    if isinstance(n_concepts, bool) or int(n_concepts) != n_concepts or not 1 <= int(n_concepts) <= MAX_CONCEPTS:
        raise ValueError(f"n_concepts must be an integer in 1..{MAX_CONCEPTS}, got {n_concepts!r}")
    return int(n_concepts)


def stored_ptr(col_ptr: torch.Tensor, lim: int) -> torch.Tensor:
    """The list bounds the value-order routes use, int64 [G, n + 1]: the running maximum of ``col_ptr`` clipped to
    ``[0, lim]`` (``FeatureCodes.host_ptr`` on the device).  List f is ``[b[f], b[f + 1])``: the lists are
    disjoint and inside the first ``lim`` positions whatever ``col_ptr`` holds.  Plain torch, no synchronisation."""
    return torch.cummax(col_ptr.clamp(min=0, max=int(lim)), 1).values.contiguous()


def sort_lists(col_ptr: torch.Tensor, row: torch.Tensor, val: torch.Tensor, *,
               out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, waves: Optional[int] = None):
    """Every list of feature-major codes (``col_ptr`` int64 [G, n + 1], ``row`` int32 / ``val`` fp32 [G, cap], rows
    ascending in a list, as ``by_feature`` writes them) ordered by value: returns ``(vrow, vval)``, int32 / fp32
    [G, cap_out], holding every list at its own positions ordered by the key of its codes ascending -- the
    order-preserving map of the fp32 bit pattern, a total order on all bit patterns (-0.0 before +0.0) -- then by
    row ascending.  Rows are distinct in a list: the result is unique, the same bits every run and for every
    ``waves`` (waves per block, 1, 2 or 4; default 4).

    The lists are those of ``stored_ptr(col_ptr, min(cap, cap_out))``: entries at positions past either buffer are
    left out and the stored part of every list is sorted.  ``out``: the ``(vrow, vval)`` buffers to fill (default:
    zeros of ``cap`` entries; positions in no list are not written, so the tail keeps (0, 0.0)); they must not
    be the inputs.  One launch, one wave per list, and one [G, cap, 2] int32 scratch buffer; nothing synchronises
    and everything is graph-capturable."""
    G, n, cap, dev, row_, val_ = _lists(col_ptr, row, val)
    waves = check_waves(waves, 4)
    if out is None:
        vrow = torch.zeros(G, cap, device=dev, dtype=torch.int32)
        vval = torch.zeros(G, cap, device=dev, dtype=torch.float32)
    else:
        vrow, vval = out
        if vrow.dim() != 2:
            raise ValueError(f"out must be (vrow int32 [{G}, cap_out], vval fp32 [{G}, cap_out])")
        _buffer("out vrow", vrow, torch.int32, (G, vrow.shape[1]), dev)
        _buffer("out vval", vval, torch.float32, (G, vrow.shape[1]), dev)
        if vrow.data_ptr() == row.data_ptr() or vval.data_ptr() == val.data_ptr():
            raise ValueError("sort_lists does not work in place: out must not be the inputs")
    ocap = vrow.shape[1]
    if cap > INT32_MAX or ocap > INT32_MAX:
        raise ValueError(f"sort_lists needs cap < 2^31 and cap_out < 2^31 (got {cap}, {ocap})")
    if min(cap, ocap) == 0 or G == 0:
        return vrow, vval
    ptr = stored_ptr(col_ptr, min(cap, ocap))
    tmp = torch.empty(G, cap, 2, device=dev, dtype=torch.int32)
    rc = _lib.lib().sc_list_sort_by_value(_lib.ptr(ptr), _lib.ptr(row_), _lib.ptr(val_), _lib.ptr(vrow),
                                          _lib.ptr(vval), _lib.ptr(tmp), G, n, cap, ocap, waves,
                                          _lib.stream_handle())
    _lib.check(rc, "sc_list_sort_by_value")
    return vrow, vval


def list_auroc(col_ptr: torch.Tensor, vrow: torch.Tensor, vval: torch.Tensor, flags: torch.Tensor, n_concepts: int,
               *, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, waves: Optional[int] = None):
    """The rank sums of every value-ordered list (``col_ptr`` int64 [G, n + 1], ``vrow`` int32 / ``vval`` fp32
    [G, cap], as ``sort_lists`` writes them) against ``n_concepts`` = K (1..32) concepts: bit k of ``flags`` int32
    [N] at row r says that row r is a positive of concept k (bit 31 included).  Returns ``(pos_in int32, u2
    int64)``, [G, n, K] each: the positives among the list's rows, and the sum over them of ``2 #{negative rows of
    the list with a smaller value} + #{negative rows of the list with an equal value}``.  Ties are equal fp32
    values; integer sums, the same bits every run and for every ``waves``.

    The lists are those of ``stored_ptr(col_ptr, cap)``; an entry whose row lies outside [0, N) is skipped.
    ``out``: the two buffers to fill, every slot is written.  One launch, one wave per list; nothing
    synchronises."""
    G, n, cap, dev, row_, val_ = _lists(col_ptr, vrow, vval)
    K, waves = check_concepts(n_concepts), check_waves(waves, 4)
    if flags.dim() != 1 or flags.shape[0] < 1:
        raise ValueError("flags must be int32 [N] with N >= 1")
    N = flags.shape[0]
    _buffer("flags", flags, torch.int32, (N,), dev)
    if N > INT32_MAX or cap > INT32_MAX:
        raise ValueError(f"list_auroc needs N < 2^31 and cap < 2^31 (got N={N}, cap={cap})")
    out = out_buffers((("pos_in", torch.int32, (G, n, K)), ("u2", torch.int64, (G, n, K))), out, dev)
    if G == 0:
        return out
    ptr = stored_ptr(col_ptr, cap)
    rc = _lib.lib().sc_list_auroc(_lib.ptr(ptr), _lib.ptr(row_), _lib.ptr(val_), _lib.ptr(flags), _lib.ptr(out[0]),
                                  _lib.ptr(out[1]), G, n, cap, N, K, waves, _lib.stream_handle())
    _lib.check(rc, "sc_list_auroc")
    return out
