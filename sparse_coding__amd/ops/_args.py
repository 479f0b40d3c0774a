"""Argument checks the sparse-code front-ends share: buffers, CSR codes, feature-major lists, dictionaries,
waves per block and ``out=`` tuples.  Every message is part of the front-ends' contract (tests match on them)."""

from __future__ import annotations

import torch

INT32_MAX = 2 ** 31 - 1
WAVES = (1, 2, 4)         # waves per block of the one-wave-per-list kernels


def _buffer(name: str, t: torch.Tensor, dtype, shape, device):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{name} must be contiguous {dtype} {list(shape)} on the dictionary's device")


def check_waves(waves, default=None) -> int:
    if waves is None and default is not None:
        waves = default
    if waves not in WAVES:
        raise ValueError(f"waves must be one of {WAVES}, got {waves!r}")
    return int(waves)


def out_buffers(spec, out, device) -> tuple:
    """The ``out=`` buffers of a launch as a tuple: ``spec`` holds one ``(name, dtype, shape)`` per buffer; ``out``
    None allocates them, anything else must hold exactly these buffers."""
    if out is None:
        return tuple(torch.empty(shape, device=device, dtype=dt) for _, dt, shape in spec)
    if len(out) != len(spec):
        raise ValueError(f"out must hold the {len(spec)} buffers {[s[0] for s in spec]}")
    for t, (name, dt, shape) in zip(out, spec):
        _buffer(f"out {name}", t, dt, shape, device)
    return tuple(out)


def _dictionary(D: torch.Tensor, what: str, step: int = 32, max_d=None):
    """(G, n, d) of the bf16 dictionary ``D``: ``d`` a multiple of ``step``, at least ``step`` and at most ``max_d``."""
    if D.dim() != 3 or D.dtype != torch.bfloat16 or not D.is_contiguous() or D.data_ptr() % 16:
        raise ValueError(f"{what} needs a contiguous, 16-byte aligned bf16 dictionary [G, n, d]")
    G, n, d = D.shape
    if G < 1 or n < 1 or d < step or d % step or (max_d is not None and d > max_d):
        need = f"d % {step} == 0" + ("" if max_d is None else f" and {step} <= d <= {max_d}")
        raise ValueError(f"{what} needs {need} (got n={n}, d={d})")
    return G, n, d


def _csr(row_ptr, col, val, nactive):
    if row_ptr.dim() != 2 or row_ptr.dtype != torch.int64 or not row_ptr.is_contiguous() or row_ptr.shape[1] < 2:
        raise ValueError("row_ptr must be contiguous int64 [G, N + 1] with N >= 1")
    G, dev = row_ptr.shape[0], row_ptr.device
    if col.dim() != 2 or col.shape[0] != G:
        raise ValueError(f"col must be int32 [{G}, cap]")
    cap = col.shape[1]
    _buffer("col", col, torch.int32, (G, cap), dev)
    _buffer("val", val, torch.float32, (G, cap), dev)
    if nactive is not None:
        _buffer("nactive", nactive, torch.int32, (G,), dev)
    N = row_ptr.shape[1] - 1
    if N > INT32_MAX or cap > INT32_MAX:
        raise ValueError(f"by_feature needs N < 2^31 and cap < 2^31 (got N={N}, cap={cap})")
    return G, N, cap, dev


def _lists(col_ptr, row, val):
    if col_ptr.dim() != 2 or col_ptr.dtype != torch.int64 or not col_ptr.is_contiguous() or col_ptr.shape[1] < 2:
        raise ValueError("col_ptr must be contiguous int64 [G, n + 1]")
    G, n, dev = col_ptr.shape[0], col_ptr.shape[1] - 1, col_ptr.device
    if row.dim() != 2 or row.shape[0] != G:
        raise ValueError(f"row must be int32 [{G}, cap]")
    cap = row.shape[1]
    _buffer("row", row, torch.int32, (G, cap), dev)
    _buffer("val", val, torch.float32, (G, cap), dev)
    if cap == 0:
        row, val = col_ptr.new_zeros(G, 1, dtype=torch.int32), col_ptr.new_zeros(G, 1, dtype=torch.float32)
    return G, n, cap, dev, row, val


def _rows(what, row_ptr, col, val, D, x, skipped, row0, n_rows, nactive):
    """The checks the launches over a window of rows with their bf16 inputs share; returns (G, n, d, cap, row0,
    n_rows, x_stride, col, val)."""
    G, n, d = _dictionary(D, what, 64, 1024)
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
