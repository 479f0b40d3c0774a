"""Python front-end for the label-profile kernel (``csrc/label_profile.hip``)."""

from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._args import INT32_MAX, WAVES, _buffer, _lists, check_waves, out_buffers  # noqa: F401 (WAVES is public)

MAX_M = 64                # most runs kept per feature: one slot per lane
RANKS = ("sum", "count")


def check_m(m) -> int:
    if isinstance(m, bool) or int(m) != m or not 1 <= int(m) <= MAX_M:
        raise ValueError(f"m must be an integer in 1..{MAX_M}, got {m!r}")
    return int(m)


def check_rank(rank_by) -> str:
    if rank_by not in RANKS:
        raise ValueError(f"rank_by must be one of {RANKS}, got {rank_by!r}")
    return rank_by


def label_profile(col_ptr: torch.Tensor, row: torch.Tensor, val: torch.Tensor, lab: torch.Tensor, m: int = 8,
                  rank_by: str = "sum", *, waves: int = 4, out: Optional[tuple] = None):
    """The label profile of every list of feature-major codes (``col_ptr`` int64 [G, n + 1], ``row`` int32 /
    ``val`` fp32 [G, cap], rows ascending in a list, as ``by_feature`` writes them) over M rows whose labels are
    ``lab`` int32 [M], non-decreasing.  Equal labels are then adjacent in every list; a maximal stretch of entries
    with one label is a run.

    Returns ``(n_entries int64, n_labels int32, count_sq int64, total fp64)``, [G, n] each, and ``(top_label
    int32, top_count int32, top_sum fp64, top_max fp32)``, [G, n, m] each, as one tuple of eight.  Per run:
    its entries, the largest of its codes, and the sum of its codes in fp64, ``acc = acc + double(val)`` from 0.0
    over the entries in list order.  Per list: its entries, its runs, the sum of the squared run counts and
    ``total``, ``acc = acc + sum_run`` from 0.0 over the runs in list order.  The ``m`` (1..64) best runs under
    ``rank_by``: "sum" -- the fp64 sum descending, "count" -- the count descending; then the label ascending.
    All m slots are written; empty slots read (-1, 0, 0.0, 0.0).

    List bounds are clipped to [0, cap]; an entry whose row lies outside [0, M) is skipped; a ``lab`` that is not
    sorted only gives more runs.  ``waves``: waves per block, 1, 2 or 4 -- the bits do not depend on it.
    ``out``: the eight buffers to fill.  One launch, one wave per list; nothing synchronises."""
    G, n, cap, dev, row_, val_ = _lists(col_ptr, row, val)
    m, rank_by, waves = check_m(m), check_rank(rank_by), check_waves(waves)
    if lab.dim() != 1 or lab.shape[0] < 1:
        raise ValueError("lab must be int32 [M] with M >= 1")
    M = lab.shape[0]
    _buffer("lab", lab, torch.int32, (M,), dev)
    if M > INT32_MAX or cap > INT32_MAX:
        raise ValueError(f"label_profile needs M < 2^31 and cap < 2^31 (got M={M}, cap={cap})")
    spec = (("n_entries", torch.int64, (G, n)), ("n_labels", torch.int32, (G, n)), ("count_sq", torch.int64, (G, n)),
            ("total", torch.float64, (G, n)), ("top_label", torch.int32, (G, n, m)),
            ("top_count", torch.int32, (G, n, m)), ("top_sum", torch.float64, (G, n, m)),
            ("top_max", torch.float32, (G, n, m)))
    out = out_buffers(spec, out, dev)
    rc = _lib.lib().sc_label_profile(_lib.ptr(col_ptr), _lib.ptr(row_), _lib.ptr(val_), _lib.ptr(lab),
                                     *(_lib.ptr(t) for t in out), G, n, cap, M, m, RANKS.index(rank_by), waves,
                                     _lib.stream_handle())
    _lib.check(rc, "sc_label_profile")
    return out
