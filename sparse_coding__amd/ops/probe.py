"""Python front-end for the probe kernels (``csrc/probe.hip``): the two sparse-times-dense products of a linear
probe on sparse codes, with 32 right-hand sides, and the reductions and vector updates between them.

Dense operands are fp32 ``[G, M, 32]`` (``CONCEPTS`` columns; unused concepts are zero columns).  Every sum is
accumulated in fp64 in an order the kernels fix (``csrc/probe.hip``), and rounded once: the same bits every run and
for every ``waves``.  Nothing here synchronises and everything is graph-capturable."""

from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib
from ._args import INT32_MAX, WAVES, _buffer, _csr, _lists, check_waves, out_buffers  # noqa: F401 (WAVES is public)
from .value_order import stored_ptr

CONCEPTS = 32             # columns of every dense operand: one per bit of a flag word
PROBE_SEG = 512           # entries per list segment of ``lists_matmul``: one wave takes one segment (measured:
                          # profiles/r24/probes/README.md; part of the contract, it fixes the fp64 order)
PROBE_SLAB = 1024         # rows per slab of ``col_dots`` (``csrc/probe.hip``)
LINE_STEPS = 8            # line-search candidates ``2^-j`` of ``line_losses`` (``csrc/probe.hip``: PROBE_STEPS)


def _operand(name: str, t: torch.Tensor, G: int, M: int, dev):
    _buffer(name, t, torch.float32, (G, M, CONCEPTS), dev)


def rows_matmul(row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, P: torch.Tensor, *,
                shift: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                nactive: Optional[torch.Tensor] = None, skipped: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, waves: Optional[int] = None,
                scale: Optional[torch.Tensor] = None):
    """``Q = C P - 1 (x) shift`` on the rows of ``mask``, zeros on the others: the CSR codes ``row_ptr`` int64
    [G, N + 1], ``col`` int32 / ``val`` fp32 [G, cap] of G models, ``P`` fp32 [G, n, 32], ``shift`` fp64 [G, 32]
    (default: none), ``mask`` uint8 [N] (default: every row).  Returns ``(Q fp32 [G, N, 32], skipped int64 [G])``.
    ``scale``: fp32 [G, N, 32] (not ``out``); ``Q`` is multiplied by it element by element, in fp64 before the one
    rounding (``sc_probe_rows_scaled``: the Hessian product of a logistic probe in the same launch).

    Per row and concept the products are accumulated in fp64 -- entries 0, 2, 4 .. of the row in one sum, entries
    1, 3, 5 .. in another, each in order, one fma each -- and ``Q`` is the sum of the two, minus the shift, rounded
    once.  A row is left out (zeros, and 1 added to ``skipped[g]``) unless ``0 <= row_ptr[r] <= row_ptr[r + 1] <=
    cap``, it has at most n entries and every column lies in [0, lim), lim = n or ``min(n, nactive[g])``: the
    skip rule of ``ops.sparse_recon``.  ``out``: the ``Q`` buffer to fill, every element is written.  One launch,
    one wave per (model, row)."""
    G, N, cap, dev = _csr(row_ptr, col, val, nactive)
    waves = check_waves(waves, 4)
    if P.dim() != 3:
        raise ValueError(f"P must be fp32 [{G}, n, {CONCEPTS}]")
    n = P.shape[1]
    _operand("P", P, G, n, dev)
    if n < 1 or n > INT32_MAX:
        raise ValueError(f"rows_matmul needs 1 <= n < 2^31 (got {n})")
    if shift is not None:
        _buffer("shift", shift, torch.float64, (G, CONCEPTS), dev)
    if mask is not None:
        _buffer("mask", mask, torch.uint8, (N,), dev)
    if skipped is None:
        skipped = torch.zeros(G, device=dev, dtype=torch.int64)
    _buffer("skipped", skipped, torch.int64, (G,), dev)
    (Q,) = out_buffers((("Q", torch.float32, (G, N, CONCEPTS)),), None if out is None else (out,), dev)
    if cap == 0:  # (no entry is stored: only rows 0 .. 0 pass the skip rule and no entry is read)
        col, val = row_ptr.new_zeros(G, 1, dtype=torch.int32), row_ptr.new_zeros(G, 1, dtype=torch.float32)
    if scale is not None:
        _operand("scale", scale, G, N, dev)
        if scale.data_ptr() == Q.data_ptr():
            raise ValueError("rows_matmul needs scale and out to be different buffers")
        rc = _lib.lib().sc_probe_rows_scaled(_lib.ptr(row_ptr), _lib.ptr(col), _lib.ptr(val), _lib.ptr(nactive),
                                             _lib.ptr(P), _lib.ptr(shift), _lib.ptr(mask), _lib.ptr(scale),
                                             _lib.ptr(Q), _lib.ptr(skipped), G, N, n, cap, waves,
                                             _lib.stream_handle())
        _lib.check(rc, "sc_probe_rows_scaled")
        return Q, skipped
    rc = _lib.lib().sc_probe_rows(_lib.ptr(row_ptr), _lib.ptr(col), _lib.ptr(val), _lib.ptr(nactive), _lib.ptr(P),
                                  _lib.ptr(shift), _lib.ptr(mask), _lib.ptr(Q), _lib.ptr(skipped), G, N, n, cap,
                                  waves, _lib.stream_handle())
    _lib.check(rc, "sc_probe_rows")
    return Q, skipped


class ListsPlan(NamedTuple):
    """The segment table of ``lists_matmul`` for one ``col_ptr``: torch arithmetic on the device, built once for
    any number of products over the same lists."""

    ptr: torch.Tensor        # int64 [G, n + 1]  stored_ptr(col_ptr, cap)
    seg_ptr: torch.Tensor    # int64 [G, n + 1]  the first segment of every list (every list has at least one)
    seg_feat: torch.Tensor   # int32 [G, maxseg] the list of every segment, -1 past the last
    segment: int


def check_segment(segment) -> int:
    if isinstance(segment, bool) or int(segment) != segment or int(segment) < 64 or int(segment) % 2 \
            or int(segment) > 2 ** 30:
        raise ValueError(f"segment must be an even integer in 64..2^30, got {segment!r}")
    return int(segment)


def lists_plan(col_ptr: torch.Tensor, cap: int, segment: int = PROBE_SEG) -> ListsPlan:
    """``ListsPlan`` of the lists ``stored_ptr(col_ptr, cap)`` cut into segments of ``segment`` entries: a list of
    L entries has ``max(1, ceil(L / segment))`` segments, a model at most ``n + cap // segment``, which sizes the
    grid without a host read."""
    seg = check_segment(segment)
    ptr = stored_ptr(col_ptr, cap)
    G, n = ptr.shape[0], ptr.shape[1] - 1
    ln = ptr[:, 1:] - ptr[:, :-1]
    seg_ptr = torch.zeros_like(ptr)
    seg_ptr[:, 1:] = torch.cumsum(((ln + (seg - 1)) // seg).clamp(min=1), 1)
    maxseg = n + int(cap) // seg
    at = torch.arange(maxseg, device=ptr.device).expand(G, -1).contiguous()
    feat = torch.searchsorted(seg_ptr, at, right=True) - 1
    feat = torch.where(feat >= n, torch.full_like(feat, -1), feat).to(torch.int32)
    return ListsPlan(ptr, seg_ptr, feat.contiguous(), seg)


def lists_matmul(col_ptr: torch.Tensor, row: torch.Tensor, val: torch.Tensor, R: torch.Tensor, *,
                 plan: Optional[ListsPlan] = None, segment: int = PROBE_SEG, out: Optional[torch.Tensor] = None,
                 waves: Optional[int] = None) -> torch.Tensor:
    """``S = C^T R``, fp32 [G, n, 32]: the feature-major lists ``col_ptr`` int64 [G, n + 1], ``row`` int32 / ``val``
    fp32 [G, cap] (as ``by_feature`` writes them; the lists are those of ``stored_ptr(col_ptr, cap)``) and ``R`` fp32
    [G, N, 32].  An entry whose row lies outside [0, N) is skipped.

    A list is cut into segments of ``segment`` = ``PROBE_SEG`` entries and one wave takes one segment, so a feature
    that fires on half the pool does not set the time.  Per segment and concept the products are accumulated in
    fp64 -- entries 0, 2, 4 .. of the segment in one sum, entries 1, 3, 5 .. in another, each in order -- the
    segment's partial is the sum of the two, a list's partials are added in segment order and the result is rounded
    once.  ``plan``: ``lists_plan(col_ptr, cap, segment)`` of an earlier call on the same lists.  ``out``: the buffer
    to fill, every element is written.  Two launches and one fp64 [G, n + cap // segment, 32] scratch buffer."""
    G, n, cap, dev, row_, val_ = _lists(col_ptr, row, val)
    waves = check_waves(waves, 4)
    if R.dim() != 3:
        raise ValueError(f"R must be fp32 [{G}, N, {CONCEPTS}]")
    N = R.shape[1]
    _operand("R", R, G, N, dev)
    if N < 1 or N > INT32_MAX or cap > INT32_MAX:
        raise ValueError(f"lists_matmul needs 1 <= N < 2^31 and cap < 2^31 (got N={N}, cap={cap})")
    if plan is None:
        plan = lists_plan(col_ptr, cap, segment)
    maxseg = plan.seg_feat.shape[1]
    _buffer("plan.ptr", plan.ptr, torch.int64, (G, n + 1), dev)
    _buffer("plan.seg_ptr", plan.seg_ptr, torch.int64, (G, n + 1), dev)
    _buffer("plan.seg_feat", plan.seg_feat, torch.int32, (G, n + cap // check_segment(plan.segment)), dev)
    (S,) = out_buffers((("S", torch.float32, (G, n, CONCEPTS)),), None if out is None else (out,), dev)
    part = torch.empty(G, maxseg, CONCEPTS, device=dev, dtype=torch.float64)
    rc = _lib.lib().sc_probe_lists(_lib.ptr(plan.ptr), _lib.ptr(row_), _lib.ptr(val_), _lib.ptr(plan.seg_ptr),
                                   _lib.ptr(plan.seg_feat), _lib.ptr(R), _lib.ptr(part), _lib.ptr(S), G, n, cap, N,
                                   maxseg, plan.segment, waves, _lib.stream_handle())
    _lib.check(rc, "sc_probe_lists")
    return S


def col_dots(A: torch.Tensor, B: Optional[torch.Tensor] = None, *, out: Optional[torch.Tensor] = None,
             waves: Optional[int] = None) -> torch.Tensor:
    """fp64 [G, 32]: ``sum_m A[g, m, k] B[g, m, k]`` over ``A``, ``B`` fp32 [G, M, 32]; ``B = A`` gives squared
    norms, ``B = None`` the column sums of ``A``.  fp64 partials over slabs of ``PROBE_SLAB`` rows (even rows of
    the slab in one sum, odd rows in another, each in order), then the slabs in order: the order does not depend
    on the launch.  Two launches."""
    if A.dim() != 3:
        raise ValueError(f"A must be fp32 [G, M, {CONCEPTS}]")
    G, M, dev = A.shape[0], A.shape[1], A.device
    waves = check_waves(waves, 4)
    _operand("A", A, G, M, dev)
    if B is not None:
        _operand("B", B, G, M, dev)
    if G < 1 or M < 1 or M > INT32_MAX:
        raise ValueError(f"col_dots needs G >= 1 and 1 <= M < 2^31 (got G={G}, M={M})")
    (res,) = out_buffers((("out", torch.float64, (G, CONCEPTS)),), None if out is None else (out,), dev)
    part = torch.empty(G, -(-M // PROBE_SLAB), CONCEPTS, device=dev, dtype=torch.float64)
    rc = _lib.lib().sc_probe_dots(_lib.ptr(A), _lib.ptr(B), _lib.ptr(part), _lib.ptr(res), G, M, waves,
                                  _lib.stream_handle())
    _lib.check(rc, "sc_probe_dots")
    return res


def axpby_(y: torch.Tensor, x: torch.Tensor, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """``y <- a x + b y`` in place: ``x``, ``y`` fp32 [G, M, 32], ``a``, ``b`` fp64 [G, 32] per (model, concept).
    Computed in fp64 as ``fma(a, x, b y)`` and rounded once.  One launch."""
    if y.dim() != 3:
        raise ValueError(f"y must be fp32 [G, M, {CONCEPTS}]")
    G, M, dev = y.shape[0], y.shape[1], y.device
    _operand("y", y, G, M, dev)
    _operand("x", x, G, M, dev)
    _buffer("a", a, torch.float64, (G, CONCEPTS), dev)
    _buffer("b", b, torch.float64, (G, CONCEPTS), dev)
    if x.data_ptr() == y.data_ptr():
        raise ValueError("axpby_ needs x and y to be different buffers")
    if G < 1 or M < 1 or M > INT32_MAX or x.data_ptr() % 16 or y.data_ptr() % 16:
        raise ValueError(f"axpby_ needs G >= 1, 1 <= M < 2^31 and 16-byte aligned buffers (got G={G}, M={M})")
    rc = _lib.lib().sc_probe_axpby(_lib.ptr(x), _lib.ptr(a), _lib.ptr(b), _lib.ptr(y), G, M, _lib.stream_handle())
    _lib.check(rc, "sc_probe_axpby")
    return y


def _margins(name: str, Z: torch.Tensor, flags: torch.Tensor, mask: torch.Tensor):
    if Z.dim() != 3:
        raise ValueError(f"{name} must be fp32 [G, N, {CONCEPTS}]")
    G, N, dev = Z.shape[0], Z.shape[1], Z.device
    _operand(name, Z, G, N, dev)
    _buffer("flags", flags, torch.int32, (N,), dev)
    _buffer("mask", mask, torch.uint8, (N,), dev)
    if G < 1 or N < 1 or N > INT32_MAX:
        raise ValueError(f"the logistic ops need G >= 1 and 1 <= N < 2^31 (got G={G}, N={N})")
    return G, N, dev


def logit_terms(Z: torch.Tensor, flags: torch.Tensor, mask: torch.Tensor, *, out=None, waves: Optional[int] = None):
    """The terms of a logistic probe at the margins ``Z`` fp32 [G, N, 32]: ``(R fp32 [G, N, 32], D fp32 [G, N, 32],
    loss fp64 [G, 32])`` with ``R = sigma(Z) - t``, ``D = sigma(Z) (1 - sigma(Z))`` on the rows of ``mask`` (uint8
    [N]) and zeros on the others, ``t`` bit k of the flag words ``flags`` int32 [N], and ``loss`` the sum over the
    rows of ``mask`` of ``softplus(z) - t z``, ``softplus(z) = max(z, 0) + log1p(exp(-|z|))``.

    Sigma and the loss are evaluated in fp64 from the fp32 margin -- from ``e = exp(-|z|)`` alone, ``sigma(|z|) =
    1 / (1 + e)`` and ``sigma(-|z|) = e / (1 + e)`` -- and ``R``, ``D`` are rounded once.  The loss sums are fp64
    partials over slabs of ``PROBE_SLAB`` rows (even rows of the slab in one sum, odd rows in another, each in
    order), then the slabs in order, as ``col_dots``.  ``out``: the ``(R, D, loss)`` buffers to fill (not ``Z``).
    Two launches."""
    G, N, dev = _margins("Z", Z, flags, mask)
    waves = check_waves(waves, 4)
    R, D, loss = out_buffers((("R", torch.float32, (G, N, CONCEPTS)), ("D", torch.float32, (G, N, CONCEPTS)),
                              ("loss", torch.float64, (G, CONCEPTS))), out, dev)
    if len({Z.data_ptr(), R.data_ptr(), D.data_ptr()}) != 3:
        raise ValueError("logit_terms needs Z, R and D to be different buffers")
    part = torch.empty(G, -(-N // PROBE_SLAB), CONCEPTS, device=dev, dtype=torch.float64)
    rc = _lib.lib().sc_probe_logit(_lib.ptr(Z), _lib.ptr(flags), _lib.ptr(mask), _lib.ptr(R), _lib.ptr(D),
                                   _lib.ptr(part), _lib.ptr(loss), G, N, waves, _lib.stream_handle())
    _lib.check(rc, "sc_probe_logit")
    return R, D, loss


def line_losses(Z: torch.Tensor, U: torch.Tensor, flags: torch.Tensor, mask: torch.Tensor, *,
                out: Optional[torch.Tensor] = None, waves: Optional[int] = None) -> torch.Tensor:
    """fp64 [G, 8, 32]: the loss sums of ``logit_terms`` at the margins ``Z + 2^-j U``, j = 0 .. 7 (``Z``, ``U`` fp32
    [G, N, 32]): the eight candidates of a backtracking line search from one read of ``Z`` and ``U``.  The margin
    is formed in fp64 (the product with ``2^-j`` is exact, the sum is rounded once); the sums go as in
    ``logit_terms``.  Two launches."""
    G, N, dev = _margins("Z", Z, flags, mask)
    _operand("U", U, G, N, dev)
    waves = check_waves(waves, 4)
    if G > 2 ** 22 - 1:
        raise ValueError(f"line_losses needs G < 2^22 (got {G})")
    (res,) = out_buffers((("out", torch.float64, (G, LINE_STEPS, CONCEPTS)),), None if out is None else (out,), dev)
    part = torch.empty(G, LINE_STEPS, -(-N // PROBE_SLAB), CONCEPTS, device=dev, dtype=torch.float64)
    rc = _lib.lib().sc_probe_line(_lib.ptr(Z), _lib.ptr(U), _lib.ptr(flags), _lib.ptr(mask), _lib.ptr(part),
                                  _lib.ptr(res), G, N, waves, _lib.stream_handle())
    _lib.check(rc, "sc_probe_line")
    return res
