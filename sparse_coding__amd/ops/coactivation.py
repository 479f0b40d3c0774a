"""Python front-end for the co-activation kernels (``csrc/coactivation.hip``)."""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._args import INT32_MAX, _buffer, _lists, out_buffers

MAX_M = 32                # most partners per (source feature, target model)
MAX_COLS = 16384          # widest target model: 64 KiB of int32 accumulators for one wave
MAX_LDS = 65536           # bytes of accumulators per block
MAX_WAVES = 4
SCORES = ("pearson", "cosine", "jaccard")


def check_m(m) -> int:
    if isinstance(m, bool) or int(m) != m or not 0 <= int(m) <= MAX_M:
        raise ValueError(f"m must be an integer in 0..{MAX_M}, got {m!r}")
    return int(m)


def check_score(score) -> str:
    if score not in SCORES:
        raise ValueError(f"score must be one of {SCORES}, got {score!r}")
    return score


def check_min_both(min_both) -> int:
    if isinstance(min_both, bool) or int(min_both) != min_both or not 1 <= int(min_both) <= INT32_MAX:
        raise ValueError(f"min_both must be an integer >= 1, got {min_both!r}")
    return int(min_both)


def check_width(n_b) -> int:
    if isinstance(n_b, bool) or int(n_b) != n_b or int(n_b) < 1:
        raise ValueError(f"n_b must be a positive integer, got {n_b!r}")
    if int(n_b) > MAX_COLS:
        raise ValueError(f"co-activation needs a target of at most {MAX_COLS} features, got {n_b}")
    return int(n_b)


def geometry(n_b: int, use_dot: bool, window: Optional[int] = None, waves: Optional[int] = None) -> Tuple[int, int]:
    """(window, waves) of a launch: the target columns one walk accumulates (8 bytes of LDS each for the dot
    instantiation, 4 for the count one) and the waves per block, so a block stays within 64 KiB."""
    per = 8 if use_dot else 4
    if window is None:
        window = min(n_b, MAX_LDS // per)
    window = int(window)
    if window < 1 or window * per > MAX_LDS:
        raise ValueError(f"window must be in 1..{MAX_LDS // per}, got {window}")
    window = min(window, n_b)
    if waves is None:
        waves = max(1, min(MAX_WAVES, MAX_LDS // (window * per)))
    waves = int(waves)
    if waves < 1 or waves > MAX_WAVES or waves * window * per > MAX_LDS:
        raise ValueError(f"waves must be in 1..{MAX_WAVES} with waves * window * {per} <= {MAX_LDS}, got {waves}")
    return window, waves


def list_moments(col_ptr: torch.Tensor, row: torch.Tensor, val: torch.Tensor):
    """Per list of feature-major codes (``col_ptr`` int64 [G, n + 1], ``row`` int32 / ``val`` fp32 [G, cap]):
    ``(cnt int32 [G, n], s1 fp64 [G, n], s2 fp64 [G, n])``, the stored entries of the list, the sum of its codes
    and the sum of their squares.  The fp64 sums run in a fixed order (per lane the entries lane, lane + 64, ...
    ascending, then the xor butterfly 1 .. 32): the same bits every run.  One launch, one wave per list, every
    element is written; nothing synchronises."""
    G, n, cap, dev, row_, val_ = _lists(col_ptr, row, val)
    cnt = torch.empty(G, n, device=dev, dtype=torch.int32)
    s1 = torch.empty(G, n, device=dev, dtype=torch.float64)
    s2 = torch.empty(G, n, device=dev, dtype=torch.float64)
    rc = _lib.lib().sc_list_moments(_lib.ptr(col_ptr), _lib.ptr(val_), _lib.ptr(cnt), _lib.ptr(s1), _lib.ptr(s2),
                                    G, n, cap, _lib.stream_handle())
    _lib.check(rc, "sc_list_moments")
    return cnt, s1, s2


def coactivation_topm(a_col_ptr: torch.Tensor, a_row: torch.Tensor, a_val: torch.Tensor, b_row_ptr: torch.Tensor,
                      b_col: torch.Tensor, b_val: torch.Tensor, n_b: int, shift_a: torch.Tensor,
                      scale_a: torch.Tensor, cnt_a: torch.Tensor, shift_b: torch.Tensor, scale_b: torch.Tensor,
                      cnt_b: torch.Tensor, m: int, mode: str, min_both: int = 1, exclude_self: bool = False,
                      nactive_b: Optional[torch.Tensor] = None, *, out=None, window: Optional[int] = None,
                      waves: Optional[int] = None):
    """The ``m`` best co-activation partners of every source feature among the features of every target model.

    Source: feature-major lists ``a_col_ptr`` int64 [Ga, n_a + 1], ``a_row`` int32 / ``a_val`` fp32 [Ga, capa]
    (rows ascending in a list, as ``by_feature`` writes them).  Target: CSR codes ``b_row_ptr`` int64
    [Gb, N + 1], ``b_col`` int32 / ``b_val`` fp32 [Gb, capb] of models with ``n_b`` features over the same N
    rows.  ``shift_*`` / ``scale_*`` fp32 and ``cnt_*`` int32 are per feature, [Ga, n_a] and [Gb, n_b].

    Returns ``(partner int32, score fp32, both int32, dot fp32)``, [Ga, Gb, n_a, m] each.  For (g, h, f) and
    column j, ``both`` counts the rows on which both fire and ``dot`` is the fp32 sum of ``a_r * b_r`` over them
    in ascending row order (``fmaf`` from 0).  ``mode`` "pearson" / "cosine": score = ``((dot - shift_a shift_b)
    scale_a) scale_b`` in unfused fp32 (the two differ only in the vectors the caller passes); "jaccard": ``both
    / (cnt_a + cnt_b - both)``; -0.0 reads +0.0.  Candidates are the columns with ``both >= min_both``, without
    column f itself when ``exclude_self`` and g == h (pass it only when the target IS the source).  The m best:
    score descending, then column ascending; empty slots read (-1, 0.0, 0, 0.0).  A target row is left out whole
    unless its pointers are ordered and within ``capb``, it has at most ``n_b`` entries and every column lies in
    [0, lim), lim = ``n_b`` or ``min(n_b, nactive_b[h])``: the skip rule of ``by_feature``, whose ``skipped``
    counts those rows.

    There is no ``state=``: the m best of a sum cannot be merged across chunks of rows, so a pool is given
    whole.  ``out``: the four buffers to fill.  ``window`` / ``waves``: target columns per walk and waves per
    block (default: as many as 64 KiB of LDS hold; a model wider than the window is walked once per window).
    One launch, one wave per (g, f, h); every slot is written; nothing synchronises."""
    Ga, n_a, capa, dev, a_row_, a_val_ = _lists(a_col_ptr, a_row, a_val)
    n_b = check_width(n_b)
    m, mode, min_both = check_m(m), check_score(mode), check_min_both(min_both)
    if b_row_ptr.dim() != 2 or b_row_ptr.dtype != torch.int64 or not b_row_ptr.is_contiguous() \
            or b_row_ptr.shape[1] < 2 or b_row_ptr.device != dev:
        raise ValueError("b_row_ptr must be contiguous int64 [Gb, N + 1] with N >= 1 on the source's device")
    Gb, N = b_row_ptr.shape[0], b_row_ptr.shape[1] - 1
    if b_col.dim() != 2 or b_col.shape[0] != Gb:
        raise ValueError(f"b_col must be int32 [{Gb}, cap]")
    capb = b_col.shape[1]
    _buffer("b_col", b_col, torch.int32, (Gb, capb), dev)
    _buffer("b_val", b_val, torch.float32, (Gb, capb), dev)
    if N > INT32_MAX or capa > INT32_MAX or capb > INT32_MAX:
        raise ValueError(f"co-activation needs N < 2^31 and cap < 2^31 (got N={N}, caps {capa}, {capb})")
    if Ga * n_a * Gb > INT32_MAX or Ga * Gb * n_a * max(m, 1) > 2 ** 40:
        raise ValueError("co-activation: too many (source feature, target model) pairs for one launch")
    for name, t, dt, shape in (("shift_a", shift_a, torch.float32, (Ga, n_a)),
                               ("scale_a", scale_a, torch.float32, (Ga, n_a)),
                               ("cnt_a", cnt_a, torch.int32, (Ga, n_a)),
                               ("shift_b", shift_b, torch.float32, (Gb, n_b)),
                               ("scale_b", scale_b, torch.float32, (Gb, n_b)),
                               ("cnt_b", cnt_b, torch.int32, (Gb, n_b))):
        _buffer(name, t, dt, shape, dev)
    if nactive_b is not None:
        _buffer("nactive_b", nactive_b, torch.int32, (Gb,), dev)
    use_dot = mode != "jaccard"
    window, waves = geometry(n_b, use_dot, window, waves)
    shape = (Ga, Gb, n_a, m)
    if out is not None:
        partner, score, both, dot = out  # (four buffers: any other length fails here, as an unpacking does)
    partner, score, both, dot = out_buffers((("partner", torch.int32, shape), ("score", torch.float32, shape),
                                             ("both", torch.int32, shape), ("dot", torch.float32, shape)), out, dev)
    if m == 0:
        return partner, score, both, dot
    if capb == 0:  # (no entry is stored: only empty rows pass the skip rule and no entry is read)
        b_col, b_val = b_row_ptr.new_zeros(Gb, 1, dtype=torch.int32), b_row_ptr.new_zeros(Gb, 1, dtype=torch.float32)
    rc = _lib.lib().sc_coactivation_topm(
        _lib.ptr(a_col_ptr), _lib.ptr(a_row_), _lib.ptr(a_val_), _lib.ptr(b_row_ptr), _lib.ptr(b_col),
        _lib.ptr(b_val), _lib.ptr(nactive_b), _lib.ptr(shift_a), _lib.ptr(scale_a), _lib.ptr(cnt_a),
        _lib.ptr(shift_b), _lib.ptr(scale_b), _lib.ptr(cnt_b), _lib.ptr(partner), _lib.ptr(score), _lib.ptr(both),
        _lib.ptr(dot), Ga, n_a, capa, Gb, n_b, N, N + 1, capb, m, int(use_dot), min_both, int(bool(exclude_self)),
        window, waves, _lib.stream_handle())
    _lib.check(rc, "sc_coactivation_topm")
    return partner, score, both, dot
