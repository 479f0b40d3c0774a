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
