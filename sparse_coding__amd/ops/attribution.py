"""Python front-end for the attribution kernels (``csrc/attribution.hip``)."""

from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._args import INT32_MAX, WAVES, _buffer, _lists, _rows, check_waves, out_buffers  # noqa: F401 (WAVES is public)


def residual_proj(row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, D: torch.Tensor, x: torch.Tensor,
                  skipped: torch.Tensor, *, row0: int = 0, n_rows: Optional[int] = None,
                  nactive: Optional[torch.Tensor] = None, proj: Optional[torch.Tensor] = None,
                  sse_row: Optional[torch.Tensor] = None):
    """Final residual and per-entry projections of a window of CSR codes: returns ``(proj, sse_row)``.  For row
    ``row0 + r`` of model g with entries ``(col_e, c_e)``, ``res = x - sum_e c_e D[g, col_e]`` accumulated in fp32
    in CSR order exactly as ``recon_split`` does; ``sse_row[g, r]`` (fp32 [G, n_rows]) is ``|res|^2`` -- the bits
    of ``recon_split(...)[g, r, 0]`` -- and ``proj[g, e]`` (fp32 [G, cap], aligned with ``col`` / ``val``) is
    ``<res, D[g, col_e]>``: per lane ``s = fma(res_i, a_i, s)`` over the lane's elements ascending from 0, then the
    xor butterfly 1, 2, 4, 8, 16, 32.  Arguments and skip rule as ``recon_split``; a skipped row writes
    ``sse_row`` 0, adds 1 to ``skipped[g]`` and stores nothing into ``proj``.

    ``proj``: the buffer to write into (default: zeros); only the positions of the entries of the window's valid
    rows are written, so one buffer serves every window of a pool.  The same bits every run.  Nothing here
    synchronises; the launch is graph-capturable."""
    G, n, d, cap, row0, n_rows, xs, col_, val_ = _rows("residual_proj", row_ptr, col, val, D, x, skipped, row0,
                                                       n_rows, nactive)
    dev = D.device
    if proj is None:
        proj = torch.zeros(G, cap, device=dev, dtype=torch.float32)
    _buffer("proj", proj, torch.float32, (G, cap), dev)
    if sse_row is None:
        sse_row = torch.empty(G, n_rows, device=dev, dtype=torch.float32)
    _buffer("sse_row", sse_row, torch.float32, (G, n_rows), dev)
    if n_rows == 0:
        return proj, sse_row
    pj = proj if cap else row_ptr.new_zeros(1, dtype=torch.float32)  # (cap 0: no entry, nothing is stored)
    rc = _lib.lib().sc_residual_proj(_lib.ptr(row_ptr), _lib.ptr(col_), _lib.ptr(val_), _lib.ptr(D), _lib.ptr(x),
                                     _lib.ptr(nactive), _lib.ptr(pj), _lib.ptr(sse_row), _lib.ptr(skipped), G,
                                     n_rows, n, d, row_ptr.shape[1], row0, cap, xs, _lib.stream_handle())
    _lib.check(rc, "sc_residual_proj")
    return proj, sse_row


def attr_list_sums(col_ptr: torch.Tensor, frow: torch.Tensor, fval: torch.Tensor, row_ptr: torch.Tensor,
                   col: torch.Tensor, proj: torch.Tensor, norm2: torch.Tensor, missing: torch.Tensor, *,
                   waves: int = 4, out: Optional[tuple] = None):
    """The raw attribution sums of every list of feature-major codes (``col_ptr`` int64 [G, n + 1], ``frow`` int32
    / ``fval`` fp32 [G, fcap], as ``by_feature`` writes them) built from the CSR ``row_ptr`` int64 [G, N + 1] /
    ``col`` int32 [G, cap], with the projections ``proj`` fp32 [G, cap] of ``residual_proj`` and the squared atom
    norms ``norm2`` fp32 [G, n] of ``row_norm2``.  Returns ``(cnt int64, A fp64, P1 fp64, C2 fp64, n_harm int64,
    min_delta fp32, max_delta fp32)``, [G, n] each: with p the projection found at the entry's CSR position (a
    binary search for column f in the entry's row) and ``delta = 2 p + c norm2[g, f]`` in fp64, ``A = sum c p``,
    ``P1 = sum p``, ``C2 = sum c^2``, ``n_harm`` the entries with ``delta < 0`` and the extrema of ``delta``
    rounded to fp32 (0.0 for an empty list).  Order of the fp64 sums: entry i of a list goes to lane ``i % 64``, a
    lane adds its entries ascending from 0.0, then the xor butterfly 1, 2, 4, 8, 16, 32.

    List bounds are clipped to [0, fcap]; an entry whose row lies outside [0, N), whose row pointers are not
    ``0 <= lo <= hi <= cap`` or whose column is not found is left out and adds 1 to ``missing[g]`` (int64 [G]).
    ``waves``: waves per block, 1, 2 or 4 -- the bits do not depend on it.  ``out``: the seven buffers to fill.
    One launch, one wave per list; nothing synchronises."""
    G, n, fcap, dev, frow_, fval_ = _lists(col_ptr, frow, fval)
    waves = check_waves(waves)
    if row_ptr.dim() != 2 or row_ptr.dtype != torch.int64 or row_ptr.shape[0] != G or row_ptr.shape[1] < 1 \
            or not row_ptr.is_contiguous() or row_ptr.device != dev:
        raise ValueError(f"row_ptr must be contiguous int64 [{G}, N + 1] on the lists' device")
    N = row_ptr.shape[1] - 1
    if col.dim() != 2 or col.shape[0] != G:
        raise ValueError(f"col must be int32 [{G}, cap]")
    cap = col.shape[1]
    _buffer("col", col, torch.int32, (G, cap), dev)
    _buffer("proj", proj, torch.float32, (G, cap), dev)
    _buffer("norm2", norm2, torch.float32, (G, n), dev)
    _buffer("missing", missing, torch.int64, (G,), dev)
    if N > INT32_MAX or fcap > INT32_MAX:
        raise ValueError(f"attr_list_sums needs N < 2^31 and fcap < 2^31 (got N={N}, fcap={fcap})")
    if cap == 0:  # (no entry is stored: every search is over an empty range and reads nothing)
        col, proj = row_ptr.new_zeros(G, 1, dtype=torch.int32), row_ptr.new_zeros(G, 1, dtype=torch.float32)
    spec = (("cnt", torch.int64), ("A", torch.float64), ("P1", torch.float64), ("C2", torch.float64),
            ("n_harm", torch.int64), ("min_delta", torch.float32), ("max_delta", torch.float32))
    out = out_buffers([(name, dt, (G, n)) for name, dt in spec], out, dev)
    rc = _lib.lib().sc_attr_list_sums(_lib.ptr(col_ptr), _lib.ptr(frow_), _lib.ptr(fval_), _lib.ptr(row_ptr),
                                      _lib.ptr(col), _lib.ptr(proj), _lib.ptr(norm2), *(_lib.ptr(t) for t in out),
                                      _lib.ptr(missing), G, n, fcap, N, N + 1, cap, waves, _lib.stream_handle())
    _lib.check(rc, "sc_attr_list_sums")
    return out
