"""Python front-end for the sparse reconstruction kernels (``csrc/sparse_recon.hip``)."""

from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .interference import _buffer

MAX_KEPT = 64   # largest J of ``recon_curve``


def _dictionary(D: torch.Tensor, what: str):
    if D.dim() != 3 or D.dtype != torch.bfloat16 or not D.is_contiguous() or D.data_ptr() % 16:
        raise ValueError(f"{what} needs a contiguous, 16-byte aligned bf16 dictionary [G, n, d]")
    G, n, d = D.shape
    if G < 1 or n < 1 or d < 64 or d > 1024 or d % 64:
        raise ValueError(f"{what} needs d % 64 == 0 and 64 <= d <= 1024 (got n={n}, d={d})")
    return G, n, d


def _rows(what, row_ptr, col, val, D, x, skipped, row0, n_rows, nactive):
    """The checks both launches share; returns (G, n, d, cap, row0, n_rows, x_stride, col, val)."""
    G, n, d = _dictionary(D, what)
    dev = D.device
    if row_ptr.dim() != 2 or row_ptr.dtype != torch.int64 or row_ptr.shape[0] != G or not row_ptr.is_contiguous() \
            or row_ptr.device != dev:
        raise ValueError(f"row_ptr must be contiguous int64 [{G}, *] on the dictionary's device")
    if x.dim() not in (2, 3) or x.dtype != torch.bfloat16 or not x.is_contiguous() or x.data_ptr() % 16 \
            or x.device != dev or x.shape[-1] != d or (x.dim() == 3 and x.shape[0] != G):
        raise ValueError(f"x must be contiguous, 16-byte aligned bf16 [rows, {d}] or [{G}, rows, {d}] on the "
                         "dictionary's device")
    row0 = int(row0)
    n_rows = x.shape[-2] if n_rows is None else int(n_rows)
    if n_rows != x.shape[-2]:
        raise ValueError(f"x holds {x.shape[-2]} rows, the window has {n_rows}")
    if row0 < 0 or n_rows < 0 or row_ptr.shape[1] < row0 + n_rows + 1:
        raise ValueError(f"row_ptr holds {row_ptr.shape[1]} entries per model, rows {row0} .. {row0 + n_rows} "
                         "are needed")
    if col.dim() != 2 or col.shape[0] != G:
        raise ValueError(f"col must be int32 [{G}, cap]")
    cap = col.shape[1]
    _buffer("col", col, torch.int32, (G, cap), dev)
    _buffer("val", val, torch.float32, (G, cap), dev)
    _buffer("skipped", skipped, torch.int64, (G,), dev)
    if nactive is not None:
        _buffer("nactive", nactive, torch.int32, (G,), dev)
    if cap == 0:  # (no entry is stored: the kernel's skip rule passes only rows 0 .. 0 and reads no entry;
        #            the placeholders stand in for the empty buffers' null pointers)
        col, val = row_ptr.new_zeros(1, dtype=torch.int32), row_ptr.new_zeros(1, dtype=torch.float32)
    return G, n, d, cap, row0, n_rows, (x.shape[1] * d if x.dim() == 3 else 0), col, val


def recon_curve(row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, D: torch.Tensor, x: torch.Tensor,
                max_kept: int, skipped: torch.Tensor, *, row0: int = 0, n_rows: Optional[int] = None,
                nactive: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Truncation curve of every row of a window of CSR codes: ``out[g, r, j]`` (fp32 [G, n_rows, J + 1],
    J = ``max_kept`` in 0..64) is ``|x - sum_{e in prefix_j} c_e D[g, col_e]|^2`` for the first ``min(j, L)``
    entries of CSR row ``row0 + r`` in rank order (code descending, then column ascending), the atoms
    subtracted in that order in fp32; ``j = 0`` is ``|x|^2`` and a row with fewer than j entries repeats its
    last value.  ``x`` holds the window's rows as the decoder sees them: bf16 [n_rows, d] shared by the
    models or [G, n_rows, d]; ``D`` is the unit-norm bf16 dictionary [G, n, d], d % 64 == 0, 64 <= d <= 1024.

    A row whose entries are not all stored (``row_ptr`` outside [0, cap], or decreasing), or with a column
    outside [0, n) -- [0, ``nactive[g]``) when ``nactive`` int32 [G] is given -- is written as zeros and
    adds 1 to ``skipped[g]`` (int64 [G]); nothing is read or written out of bounds whatever the buffers
    hold.  The same bits every run.  Nothing here synchronises; the launch is graph-capturable."""
    G, n, d, cap, row0, n_rows, xs, col, val = _rows("recon_curve", row_ptr, col, val, D, x, skipped, row0, n_rows,
                                                     nactive)
    if isinstance(max_kept, bool) or int(max_kept) != max_kept or not 0 <= int(max_kept) <= MAX_KEPT:
        raise ValueError(f"max_kept must be an integer in 0..{MAX_KEPT}, got {max_kept!r}")
    J = int(max_kept)
    if out is None:
        out = torch.empty(G, n_rows, J + 1, device=D.device, dtype=torch.float32)
    _buffer("out", out, torch.float32, (G, n_rows, J + 1), D.device)
    if n_rows == 0:
        return out
    rc = _lib.lib().sc_recon_curve(_lib.ptr(row_ptr), _lib.ptr(col), _lib.ptr(val), _lib.ptr(D), _lib.ptr(x),
                                   _lib.ptr(nactive), _lib.ptr(out), _lib.ptr(skipped), G, n_rows, n, d, J,
                                   row_ptr.shape[1], row0, cap, xs, _lib.stream_handle())
    _lib.check(rc, "sc_recon_curve")
    return out


def recon_split(row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, D: torch.Tensor, x: torch.Tensor,
                skipped: torch.Tensor, *, keep: Optional[torch.Tensor] = None, row0: int = 0,
                n_rows: Optional[int] = None, nactive: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Squared reconstruction error of every row of a window of CSR codes from all its entries, from the
    entries of the kept features and from the others: ``out[g, r]`` (fp32 [G, n_rows, 3]) is (full, keep,
    rest), each residual subtracting its atoms in the order the CSR stores them (ascending column).
    ``keep``: packed bits uint32 [G, ceil(n / 32)] (``engine.sparse_recon.keep_words``; int32 words of the
    same bits are taken too); without it columns 1 and 2 are written 0.  Arguments, skip rule and guarantees
    as ``recon_curve``."""
    G, n, d, cap, row0, n_rows, xs, col, val = _rows("recon_split", row_ptr, col, val, D, x, skipped, row0, n_rows,
                                                     nactive)
    if keep is not None:
        words = (n + 31) // 32
        if keep.dtype not in (torch.uint32, torch.int32) or tuple(keep.shape) != (G, words) \
                or not keep.is_contiguous() or keep.device != D.device:
            raise ValueError(f"keep must be contiguous uint32 [{G}, {words}] on the dictionary's device")
    if out is None:
        out = torch.empty(G, n_rows, 3, device=D.device, dtype=torch.float32)
    _buffer("out", out, torch.float32, (G, n_rows, 3), D.device)
    if n_rows == 0:
        return out
    rc = _lib.lib().sc_recon_split(_lib.ptr(row_ptr), _lib.ptr(col), _lib.ptr(val), _lib.ptr(D), _lib.ptr(x),
                                   _lib.ptr(nactive), _lib.ptr(keep), _lib.ptr(out), _lib.ptr(skipped), G, n_rows,
                                   n, d, row_ptr.shape[1], row0, cap, xs, _lib.stream_handle())
    _lib.check(rc, "sc_recon_split")
    return out
