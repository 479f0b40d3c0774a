"""Python front-end for the sparse-export kernels (``csrc/sparse_codes.hip``)."""

from __future__ import annotations

import torch

from . import _lib


def _codes(c: torch.Tensor, what: str):
    if c.dim() != 3 or c.dtype != torch.bfloat16 or not c.is_contiguous() or c.data_ptr() % 16:
        raise ValueError(f"{what} needs contiguous, 16-byte aligned bf16 codes [G, B, n]")
    G, B, n = c.shape
    if G < 1 or B < 128 or B % 128 or n < 128 or n % 128:
        raise ValueError(f"{what} needs B % 128 == 0 and n % 128 == 0 (got B={B}, n={n})")
    return G, B, n


def code_row_counts(c: torch.Tensor, nnz: torch.Tensor) -> torch.Tensor:
    """``nnz`` int32 [G, B] <- the number of strictly positive codes in every row of the bf16 codes ``c``
    [G, B, n] (``-0.0``, ``+0.0``, negative values and NaN do not count).  Every element of ``nnz`` is
    written.  Exact; nothing here synchronises; the launch is graph-capturable."""
    G, B, n = _codes(c, "code_row_counts")
    if nnz.dtype != torch.int32 or tuple(nnz.shape) != (G, B) or not nnz.is_contiguous() or nnz.device != c.device:
        raise ValueError(f"nnz must be contiguous int32 [{G}, {B}] on the codes' device")
    rc = _lib.lib().sc_code_row_counts(_lib.ptr(c), _lib.ptr(nnz), G, B, n, _lib.stream_handle())
    _lib.check(rc, "sc_code_row_counts")
    return nnz


def code_compact(c: torch.Tensor, row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, row0: int = 0):
    """Write the strictly positive codes of every row of ``c`` [G, B, n] (bf16), in ascending column order,
    to ``col`` int32 [G, cap] / ``val`` fp32 [G, cap] (the code widened, exact): row ``r`` of model ``g``
    goes to position ``row_ptr[g, row0 + r]`` onwards, ``row_ptr`` int64 [G, >= row0 + B + 1].  An entry
    whose position is not in [0, cap) is dropped: nothing is written past ``cap`` and the other entries
    are unchanged by the overflow.  Bit-reproducible (no atomics); nothing here synchronises; the launch
    is graph-capturable."""
    G, B, n = _codes(c, "code_compact")
    row0 = int(row0)
    if row_ptr.dim() != 2 or row_ptr.dtype != torch.int64 or row_ptr.shape[0] != G or not row_ptr.is_contiguous() \
            or row_ptr.device != c.device:
        raise ValueError(f"row_ptr must be contiguous int64 [{G}, *] on the codes' device")
    if row0 < 0 or row_ptr.shape[1] < row0 + B + 1:
        raise ValueError(f"row_ptr holds {row_ptr.shape[1]} entries per model, rows {row0} .. {row0 + B} are needed")
    if col.dim() != 2 or col.shape[0] != G:
        raise ValueError(f"col must be int32 [{G}, cap]")
    cap = col.shape[1]
    for name, t, dt in (("col", col, torch.int32), ("val", val, torch.float32)):
        if t.dtype != dt or tuple(t.shape) != (G, cap) or not t.is_contiguous() or t.device != c.device:
            raise ValueError(f"{name} must be contiguous {dt} [{G}, {cap}] on the codes' device")
    if cap == 0:  # (no room for any entry: all of them are dropped)
        return col, val
    rc = _lib.lib().sc_code_compact(_lib.ptr(c), _lib.ptr(row_ptr), _lib.ptr(col), _lib.ptr(val), G, B, n,
                                    row_ptr.shape[1], row0, cap, _lib.stream_handle())
    _lib.check(rc, "sc_code_compact")
    return col, val


def extend_row_ptr(row_ptr: torch.Tensor, nnz: torch.Tensor, row0: int = 0) -> torch.Tensor:
    """``row_ptr[:, row0 + 1 .. row0 + B] = row_ptr[:, row0] + cumsum(nnz)`` in int64, on the device and
    without a synchronisation: the pointers ``code_compact`` needs for the batch whose counts are ``nnz``."""
    B = nnz.shape[1]
    out = row_ptr[:, row0 + 1: row0 + B + 1]
    torch.add(torch.cumsum(nnz, dim=1, dtype=torch.int64), row_ptr[:, row0: row0 + 1], out=out)
    return row_ptr


def take_rows(row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, index: torch.Tensor,
              out_ptr: torch.Tensor, cap_out: int, waves: int = 4):
    """Gather rows of CSR codes: returns ``(col int32 [G, cap_out], val fp32 [G, cap_out])`` in which the entries
    of output row ``i`` of model ``g``, the entries of input row ``index[i]`` in order and bit for bit, start at
    ``out_ptr[g, i]``.  ``row_ptr`` int64 [G, N + 1], ``col`` int32 / ``val`` fp32 [G, cap]; ``index`` int64 [M];
    ``out_ptr`` int64 [G, M + 1], the cumsum of the gathered row lengths (the caller's, on the device).  The
    unused tail of the buffers holds (0, 0.0).

    The kernel (``sc_csr_take_rows``, ``csrc/label_profile.hip``: one wave per (model, output row)) checks every
    bound again: an index outside [0, N) or a row that fails ``0 <= row_ptr[r] <= row_ptr[r + 1] <= cap`` is
    written as empty, a row never reaches into the next one's positions and nothing is written at or past
    ``cap_out``.  Nothing here synchronises; the launch is graph-capturable."""
    if row_ptr.dim() != 2 or row_ptr.dtype != torch.int64 or not row_ptr.is_contiguous() or row_ptr.shape[1] < 2:
        raise ValueError("row_ptr must be contiguous int64 [G, N + 1] with N >= 1")
    G, N, dev = row_ptr.shape[0], row_ptr.shape[1] - 1, row_ptr.device
    if col.dim() != 2 or col.shape[0] != G:
        raise ValueError(f"col must be int32 [{G}, cap]")
    cap = col.shape[1]
    for name, t, dt in (("col", col, torch.int32), ("val", val, torch.float32)):
        if t.dtype != dt or tuple(t.shape) != (G, cap) or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be contiguous {dt} [{G}, {cap}] on the pointers' device")
    if index.dim() != 1 or index.dtype != torch.int64 or not index.is_contiguous() or index.device != dev:
        raise ValueError("index must be contiguous int64 [M] on the codes' device")
    M = index.shape[0]
    if out_ptr.dtype != torch.int64 or tuple(out_ptr.shape) != (G, M + 1) or not out_ptr.is_contiguous() \
            or out_ptr.device != dev:
        raise ValueError(f"out_ptr must be contiguous int64 [{G}, {M + 1}] on the codes' device")
    cap_out, waves = int(cap_out), int(waves)
    if cap_out < 0:
        raise ValueError(f"cap_out must be >= 0, got {cap_out}")
    if waves not in (1, 2, 4):
        raise ValueError(f"waves must be 1, 2 or 4, got {waves!r}")
    ocol = torch.zeros(G, cap_out, device=dev, dtype=torch.int32)
    oval = torch.zeros(G, cap_out, device=dev, dtype=torch.float32)
    if G == 0 or M == 0 or cap == 0 or cap_out == 0:   # (nothing to copy)
        return ocol, oval
    rc = _lib.lib().sc_csr_take_rows(_lib.ptr(row_ptr), _lib.ptr(col), _lib.ptr(val), _lib.ptr(index),
                                     _lib.ptr(out_ptr), _lib.ptr(ocol), _lib.ptr(oval), G, N, N + 1, cap, M, cap_out,
                                     waves, _lib.stream_handle())
    _lib.check(rc, "sc_csr_take_rows")
    return ocol, oval
