"""Python front-end for the feature-major sparse-code kernels (``csrc/feature_codes.hip``)."""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._args import INT32_MAX, _buffer, _csr, _lists

MAX_K = 32               # largest Kt / Kr of ``fragment_examples``
SEGMENT_ROWS = 1024      # default rows per segment of the transposition
LDS_BINS = 8192          # default widest LDS histogram: 32 KiB of the CU's 160 KiB, five blocks stay co-resident
MAX_LDS_BINS = 16384     # the kernels' own limit (64 KiB)
MAX_SEGMENT_ROWS = 8192


def by_feature(row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, n: int, *,
               nactive: Optional[torch.Tensor] = None, segment_rows: int = SEGMENT_ROWS, lds_bins: int = LDS_BINS,
               rows_per_block: int = 256, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
               skipped: Optional[torch.Tensor] = None):
    """Feature-major transposition of the CSR codes ``row_ptr`` int64 [G, N + 1], ``col`` int32 [G, cap], ``val``
    fp32 [G, cap] of G models with ``n`` features: returns ``(col_ptr, row, val, skipped)`` with ``col_ptr``
    int64 [G, n + 1], ``row`` int32 / ``val`` fp32 [G, cap_out] and ``skipped`` int64 [G].  The list of feature f
    of model g is ``row/val[g, col_ptr[g, f] : col_ptr[g, f + 1]]``, rows ascending: a stable transposition, the
    same bits every run and for every ``segment_rows`` / ``rows_per_block`` / histogram path.

    A row is left out whole and adds 1 to ``skipped[g]`` unless ``0 <= row_ptr[r] <= row_ptr[r + 1] <= cap``,
    it has at most n entries and every column lies in [0, lim), lim = n or ``min(n, nactive[g])`` (``nactive``
    int32 [G]).  ``col_ptr`` counts the entries of the rows that pass.

    ``out``: the ``(row, val)`` buffers to fill, [G, cap_out] each (default: zeros of ``cap`` entries, which
    always hold every entry of a monotone ``row_ptr``; the unused tail keeps (0, 0.0)).  Entries at positions
    ``>= cap_out`` are dropped, the stored prefix is exact and nothing is written outside.  ``segment_rows``: a
    power of two, 64 .. 8192, the rows one ordering bitmap covers; ``lds_bins``: the widest model that counts
    in an LDS histogram (at most 16384), wider ones add to global memory entry by entry; ``rows_per_block``: a
    power of two <= 256.  Three launches and device-side cumsums between them: nothing here synchronises and
    everything is graph-capturable.  (If ``row_ptr`` is not monotone, valid rows may overlap and hold more
    than ``cap`` entries between them; the surplus is dropped.)"""
    G, N, cap, dev = _csr(row_ptr, col, val, nactive)
    n = int(n)
    if n < 1:
        raise ValueError(f"n must be >= 1, got {n}")
    seg = int(segment_rows)
    if seg < 64 or seg > MAX_SEGMENT_ROWS or seg & (seg - 1):
        raise ValueError(f"segment_rows must be a power of two in 64..{MAX_SEGMENT_ROWS}, got {segment_rows!r}")
    rpb = int(rows_per_block)
    if rpb < 1 or rpb > 256 or rpb & (rpb - 1):
        raise ValueError(f"rows_per_block must be a power of two <= 256, got {rows_per_block!r}")
    rpb = min(rpb, seg)
    if not 0 <= int(lds_bins) <= MAX_LDS_BINS:
        raise ValueError(f"lds_bins must be in 0..{MAX_LDS_BINS}, got {lds_bins!r}")
    use_lds = int(n <= int(lds_bins))
    shift = seg.bit_length() - 1
    S = -(-N // seg)
    if out is None:
        orow = torch.zeros(G, cap, device=dev, dtype=torch.int32)
        oval = torch.zeros(G, cap, device=dev, dtype=torch.float32)
    else:
        orow, oval = out
        if orow.dim() != 2:
            raise ValueError(f"out must be (row int32 [{G}, cap_out], val fp32 [{G}, cap_out])")
        _buffer("out row", orow, torch.int32, (G, orow.shape[1]), dev)
        _buffer("out val", oval, torch.float32, (G, orow.shape[1]), dev)
    ocap = orow.shape[1]
    if ocap > INT32_MAX:
        raise ValueError("by_feature needs cap_out < 2^31")
    if skipped is None:
        skipped = torch.zeros(G, device=dev, dtype=torch.int64)
    _buffer("skipped", skipped, torch.int64, (G,), dev)
    if cap == 0:  # (no entry is stored: only rows 0 .. 0 pass the skip rule and no entry is read)
        col, val = row_ptr.new_zeros(G, 1, dtype=torch.int32), row_ptr.new_zeros(G, 1, dtype=torch.float32)
    lib, st = _lib.lib(), _lib.stream_handle()
    cnt = torch.zeros(G, S, n, device=dev, dtype=torch.int32)
    rc = lib.sc_feature_count(_lib.ptr(row_ptr), _lib.ptr(col), _lib.ptr(nactive), _lib.ptr(cnt), _lib.ptr(skipped),
                              G, N, n, N + 1, cap, shift, S, rpb, use_lds, st)
    _lib.check(rc, "sc_feature_count")
    col_ptr = torch.zeros(G, n + 1, device=dev, dtype=torch.int64)
    col_ptr[:, 1:] = torch.cumsum(cnt.sum(1, dtype=torch.int64), 1)
    seg_cum = torch.cumsum(cnt, 1, dtype=torch.int64)
    base = (seg_cum - cnt + col_ptr[:, None, :n]).contiguous()   # where sub-list (g, s, f) starts
    tcap = max(cap, 1)
    tmp = torch.empty(G, tcap, 2, device=dev, dtype=torch.int32)   # (row, float bits of val) pairs
    cur = torch.zeros(G, S, n, device=dev, dtype=torch.int32)
    rc = lib.sc_feature_scatter(_lib.ptr(row_ptr), _lib.ptr(col), _lib.ptr(val), _lib.ptr(nactive), _lib.ptr(base),
                                _lib.ptr(cur), _lib.ptr(tmp), G, N, n, N + 1, cap, tcap, shift, S,
                                rpb, use_lds, st)
    _lib.check(rc, "sc_feature_scatter")
    if ocap:
        rc = lib.sc_feature_order(_lib.ptr(cnt), _lib.ptr(base), _lib.ptr(tmp), _lib.ptr(orow),
                                  _lib.ptr(oval), G, n, S, shift, tcap, ocap, st)
        _lib.check(rc, "sc_feature_order")
    return col_ptr, orow, oval, skipped


def check_fragments(n_rows: int, fragment_len) -> int:
    """Number of fragments of ``fragment_len`` rows in ``n_rows`` rows; ``ValueError`` unless they tile."""
    if isinstance(fragment_len, bool) or int(fragment_len) != fragment_len or int(fragment_len) < 1:
        raise ValueError(f"fragment_len must be a positive integer, got {fragment_len!r}")
    L = int(fragment_len)
    if n_rows % L:
        raise ValueError(f"{n_rows} rows are no whole number of fragments of {L}")
    if n_rows // L > INT32_MAX:
        raise ValueError("fragment_examples needs fewer than 2^31 fragments")
    return n_rows // L


def check_k(name: str, k) -> int:
    if isinstance(k, bool) or int(k) != k or not 0 <= int(k) <= MAX_K:
        raise ValueError(f"{name} must be an integer in 0..{MAX_K}, got {k!r}")
    return int(k)


def fragment_examples(col_ptr: torch.Tensor, row: torch.Tensor, val: torch.Tensor, n_rows: int, fragment_len: int,
                      n_top: int, n_random: int, seed: int = 0):
    """Example fragments of every (model, feature) list of feature-major codes (``col_ptr`` int64 [G, n + 1],
    ``row`` int32 / ``val`` fp32 [G, cap], rows ascending in a list); fragment of a row = ``row //
    fragment_len``.  Returns ``(n_frags int64 [G, n], top_frag int32 [G, n, n_top], top_max fp32 [G, n, n_top],
    rand_frag int32 [G, n, n_random])``: the number of distinct fragments on which the feature fires; the
    fragments with the largest maximum code, maximum descending then fragment ascending, empty slots (-1, 0.0);
    and the active fragments with the smallest ``mix32(h0 ^ fragment)``, key ascending, empty slots -1 (the
    hash of ``engine.feature_codes.fragment_keys``).  ``n_top``, ``n_random`` in 0..32.  One launch, one wave
    per list; nothing synchronises."""
    G, n, cap, dev, row_, val_ = _lists(col_ptr, row, val)
    L = int(fragment_len)
    check_fragments(int(n_rows), fragment_len)
    Kt, Kr = check_k("n_top", n_top), check_k("n_random", n_random)
    n_frags = torch.empty(G, n, device=dev, dtype=torch.int64)
    top_frag = torch.empty(G, n, Kt, device=dev, dtype=torch.int32)
    top_max = torch.empty(G, n, Kt, device=dev, dtype=torch.float32)
    rand_frag = torch.empty(G, n, Kr, device=dev, dtype=torch.int32)
    rc = _lib.lib().sc_fragment_examples(_lib.ptr(col_ptr), _lib.ptr(row_), _lib.ptr(val_), _lib.ptr(n_frags),
                                         _lib.ptr(top_frag) if Kt else 0, _lib.ptr(top_max) if Kt else 0,
                                         _lib.ptr(rand_frag) if Kr else 0, G, n, cap, L, Kt, Kr,
                                         int(seed) & 0xFFFFFFFF, _lib.stream_handle())
    _lib.check(rc, "sc_fragment_examples")
    return n_frags, top_frag, top_max, rand_frag


def fragment_acts(col_ptr: torch.Tensor, row: torch.Tensor, val: torch.Tensor, n_rows: int, fragment_len: int,
                  frags: torch.Tensor, f0: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Activation records: ``out[g, f, k, t]`` (fp32 [G, nf, K, L]) is the code of feature ``f0 + f`` on row
    ``frags[g, f, k] * L + t`` of the feature-major codes, 0 where the feature does not fire and all zeros for a
    slot of -1 or a fragment outside [0, n_rows / L).  ``frags``: int32 [G, nf, K].  Every element is written;
    one launch, one wave per slot; nothing synchronises."""
    G, n, cap, dev, row_, val_ = _lists(col_ptr, row, val)
    L = int(fragment_len)
    n_frag = check_fragments(int(n_rows), fragment_len)
    if frags.dim() != 3 or frags.shape[0] != G:
        raise ValueError(f"frags must be int32 [{G}, features, K]")
    nf, K = frags.shape[1:]
    _buffer("frags", frags, torch.int32, (G, nf, K), dev)
    f0 = int(f0)
    if f0 < 0 or f0 + nf > n:
        raise ValueError(f"features [{f0}, {f0 + nf}) outside [0, {n}]")
    if out is None:
        out = torch.empty(G, nf, K, L, device=dev, dtype=torch.float32)
    _buffer("out", out, torch.float32, (G, nf, K, L), dev)
    if out.numel() == 0:
        return out
    rc = _lib.lib().sc_fragment_acts(_lib.ptr(col_ptr), _lib.ptr(row_), _lib.ptr(val_), _lib.ptr(frags), _lib.ptr(out),
                                     G, n, cap, f0, nf, K, L, n_frag, _lib.stream_handle())
    _lib.check(rc, "sc_fragment_acts")
    return out
