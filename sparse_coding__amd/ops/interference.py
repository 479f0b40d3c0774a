"""Python front-end for the interference kernels (``csrc/interference.hip``)."""

from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._args import _buffer, _dictionary


def row_norm2(D: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``norm2[g, f] = sum_k D[g, f, k]^2`` in fp32 for the bf16 dictionary ``D`` [G, n, d], summed in the
    fixed order the kernel's header gives: the same bits every run.  Nothing here synchronises; the
    launch is graph-capturable."""
    G, n, d = _dictionary(D, "row_norm2")
    if out is None:
        out = torch.empty(G, n, device=D.device, dtype=torch.float32)
    _buffer("norm2", out, torch.float32, (G, n), D.device)
    rc = _lib.lib().sc_row_norm2(_lib.ptr(D), _lib.ptr(out), G, n, d, _lib.stream_handle())
    _lib.check(rc, "sc_row_norm2")
    return out


def active_capacity(row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, D: torch.Tensor,
                    norm2: torch.Tensor, qsum: torch.Tensor, count: torch.Tensor, skipped: torch.Tensor, *,
                    row0: int = 0, n_rows: Optional[int] = None, nactive: Optional[torch.Tensor] = None,
                    entry_cap: Optional[torch.Tensor] = None):
    """Add the activity-weighted capacities of rows ``row0 .. row0 + n_rows - 1`` of the CSR codes
    (``row_ptr`` int64 [G, >= row0 + n_rows + 1], ``col`` int32 [G, cap], ``val`` fp32 [G, cap]) against
    the bf16 dictionary ``D`` [G, n, d] with squared row norms ``norm2`` fp32 [G, n]:

    every entry a of a row gets ``cap_a = c_a / max(sum_b cos^2(a, b) c_b, 1e-8)`` over the row's entries b
    (fp32 Gram on the matrix unit, ``cos^2(a, a) := 1``); ``qsum[g, col_a] += llrint(cap_a * 2^32)`` and
    ``count[g, col_a] += 1`` (int64 [G, n], integer atomics: the same bits every run and under any split
    of the rows), and ``entry_cap`` (fp32 [G, cap], optional) receives ``cap_a`` at the entry's position.

    A row whose entries are not all stored (``row_ptr`` outside [0, cap], or decreasing), or with a column
    outside [0, n) -- [0, ``nactive[g]``) when ``nactive`` int32 [G] is given -- contributes nothing and
    adds 1 to ``skipped[g]`` (int64 [G]); nothing is read or written out of bounds whatever the buffers
    hold.  Nothing here synchronises; the launch is graph-capturable."""
    G, n, d = _dictionary(D, "active_capacity")
    dev = D.device
    if row_ptr.dim() != 2 or row_ptr.dtype != torch.int64 or row_ptr.shape[0] != G or not row_ptr.is_contiguous() \
            or row_ptr.device != dev:
        raise ValueError(f"row_ptr must be contiguous int64 [{G}, *] on the dictionary's device")
    row0 = int(row0)
    n_rows = row_ptr.shape[1] - 1 - row0 if n_rows is None else int(n_rows)
    if row0 < 0 or n_rows < 0 or row_ptr.shape[1] < row0 + n_rows + 1:
        raise ValueError(f"row_ptr holds {row_ptr.shape[1]} entries per model, rows {row0} .. {row0 + n_rows} "
                         "are needed")
    if col.dim() != 2 or col.shape[0] != G:
        raise ValueError(f"col must be int32 [{G}, cap]")
    cap = col.shape[1]
    _buffer("col", col, torch.int32, (G, cap), dev)
    _buffer("val", val, torch.float32, (G, cap), dev)
    _buffer("norm2", norm2, torch.float32, (G, n), dev)
    _buffer("qsum", qsum, torch.int64, (G, n), dev)
    _buffer("count", count, torch.int64, (G, n), dev)
    _buffer("skipped", skipped, torch.int64, (G,), dev)
    if nactive is not None:
        _buffer("nactive", nactive, torch.int32, (G,), dev)
    if entry_cap is not None:
        _buffer("entry_cap", entry_cap, torch.float32, (G, cap), dev)
    if cap == 0:  # (no entry is stored: the kernel's skip rule with nothing to launch over)
        lo, hi = row_ptr[:, row0: row0 + n_rows], row_ptr[:, row0 + 1: row0 + n_rows + 1]
        skipped += ((lo < 0) | (hi > 0) | (hi < lo)).sum(1)
        return qsum, count, skipped
    rc = _lib.lib().sc_active_capacity(_lib.ptr(row_ptr), _lib.ptr(col), _lib.ptr(val), _lib.ptr(D),
                                       _lib.ptr(norm2), _lib.ptr(nactive), _lib.ptr(qsum), _lib.ptr(count),
                                       _lib.ptr(skipped), _lib.ptr(entry_cap), G, n_rows, n, d, row_ptr.shape[1],
                                       row0, cap, _lib.stream_handle())
    _lib.check(rc, "sc_active_capacity")
    return qsum, count, skipped
