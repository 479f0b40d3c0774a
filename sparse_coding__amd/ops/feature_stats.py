"""Python front-end for the per-feature statistics kernels (``csrc/feature_stats.hip``)."""

from __future__ import annotations

import torch

from . import _lib

N_STATS = 6  # count, sum c, sum c^2, sum c^3, sum c^4, max
MAX_TOPK = 32


def _codes(c: torch.Tensor, what: str):
    if c.dim() != 3 or c.dtype != torch.bfloat16 or not c.is_contiguous():
        raise ValueError(f"{what} needs contiguous bf16 codes [G, B, n]")
    G, B, n = c.shape
    if G < 1 or B < 128 or B % 128 or n < 128 or n % 128:
        raise ValueError(f"{what} needs B % 128 == 0 and n % 128 == 0 (got B={B}, n={n})")
    return G, B, n


def moment_slabs(G: int, B: int, n: int) -> int:
    """Row slabs ``col_moments`` splits a batch into: 256-row slabs once those still give the device a
    thousand blocks (half the partials to sum afterwards), 128-row slabs otherwise."""
    if B % 256 == 0 and G * (n // 128) * (B // 256) >= 1024:
        return B // 256
    return B // 128


def col_moments(c: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """Per-column partials of the bf16 codes ``c`` [G, B, n] into ``out`` fp32 [G, S, 6, n]: for each of
    the S row slabs (S divides B, B / S a multiple of 16; ``moment_slabs`` picks one) the count of
    non-zeros, the sums of c, c^2, c^3, c^4 and the maximum.  Every element of ``out`` is written.  The
    caller sums the slabs (and takes the max of the last plane).  Bit-reproducible; nothing here
    synchronises; the launch is graph-capturable."""
    G, B, n = _codes(c, "col_moments")
    if out.dim() != 4 or out.dtype != torch.float32 or not out.is_contiguous() or out.device != c.device \
            or out.shape[0] != G or out.shape[2] != N_STATS or out.shape[3] != n:
        raise ValueError(f"out must be contiguous fp32 [{G}, S, {N_STATS}, {n}] on the codes' device")
    S = out.shape[1]
    if S < 1 or B % S or (B // S) % 16:
        raise ValueError(f"S = {S} slabs do not split {B} rows into multiples of 16")
    rc = _lib.lib().sc_col_moments(_lib.ptr(c), _lib.ptr(out), G, B, n, S, _lib.stream_handle())
    _lib.check(rc, "sc_col_moments")
    return out


def col_topk(c: torch.Tensor, top_vals: torch.Tensor, top_rows: torch.Tensor, row0: int):
    """Merge the batch ``c`` [G, B, n] (bf16; global row indices ``row0 .. row0 + B - 1``) into the
    running per-column top-K lists ``top_vals`` fp32 [G, n, K] / ``top_rows`` int64 [G, n, K]
    (1 <= K <= 32), in place: the K largest strictly positive codes, value descending then row
    ascending, empty slots (0.0, -1).  Batches must come in increasing ``row0`` (a new code never
    displaces a listed one of equal value).  Exact; nothing here synchronises; graph-capturable."""
    G, B, n = _codes(c, "col_topk")
    if top_vals.dim() != 3 or top_vals.shape[0] != G or top_vals.shape[1] != n:
        raise ValueError(f"top_vals must be fp32 [{G}, {n}, K]")
    K = top_vals.shape[2]
    if not 1 <= K <= MAX_TOPK:
        raise ValueError(f"col_topk needs 1 <= K <= {MAX_TOPK} (got {K})")
    for name, t, dt in (("top_vals", top_vals, torch.float32), ("top_rows", top_rows, torch.int64)):
        if t.dtype != dt or tuple(t.shape) != (G, n, K) or not t.is_contiguous() or t.device != c.device:
            raise ValueError(f"{name} must be contiguous {dt} [{G}, {n}, {K}] on the codes' device")
    row0 = int(row0)
    if row0 < 0:
        raise ValueError(f"row0 must be >= 0 (got {row0})")
    rc = _lib.lib().sc_col_topk(_lib.ptr(c), _lib.ptr(top_vals), _lib.ptr(top_rows), G, B, n, K, row0,
                                _lib.stream_handle())
    _lib.check(rc, "sc_col_topk")
    return top_vals, top_rows
