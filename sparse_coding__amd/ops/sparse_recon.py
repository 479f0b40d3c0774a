"""Python front-end for the sparse reconstruction kernels (``csrc/sparse_recon.hip``)."""

from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._args import _buffer, _rows

MAX_KEPT = 64   # largest J of ``recon_curve``


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
