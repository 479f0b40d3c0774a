"""Python front-end for the dead-feature resampling kernels (``csrc/resample.hip``)."""

from __future__ import annotations

import torch

from . import _lib


def row_sqerr(r: torch.Tensor, err: torch.Tensor, off: int = 0) -> torch.Tensor:
    """err[g, off + b] = sum_j r[g, b, j]^2 for the bf16 residual ``r`` [G, B, d] (d % 256 == 0) into the
    fp32 matrix ``err`` [G, N] (N >= off + B): each pool batch writes its own column slice."""
    if r.dim() != 3 or r.dtype != torch.bfloat16 or not r.is_contiguous():
        raise ValueError("row_sqerr needs a contiguous bf16 residual [G, B, d]")
    G, B, d = r.shape
    if d % 256:
        raise ValueError(f"row_sqerr needs d % 256 == 0 (got {d})")
    if err.dim() != 2 or err.dtype != torch.float32 or not err.is_contiguous() or err.shape[0] != G \
            or err.device != r.device:
        raise ValueError("err must be contiguous fp32 [G, N] on the residual's device")
    N = err.shape[1]
    off = int(off)
    if off < 0 or off + B > N:
        raise ValueError(f"columns [{off}, {off + B}) are outside err [{G}, {N}]")
    rc = _lib.lib().sc_row_sqerr(_lib.ptr(r), _lib.ptr(err), G, B, d, N, off, _lib.stream_handle())
    _lib.check(rc, "sc_row_sqerr")
    return err


def resample_rows(dead_idx, src_idx, cnt, rows, enc_scale, enc, enc_m, enc_v, enc_shadow, bias, bias_m, bias_v,
                  norms, dec=None, dec_m=None, dec_v=None, dec_shadow=None, *, normalize_src: bool,
                  set_decoder: bool, zero_bias: bool):
    """Rewrite the rows ``dead_idx[g, j]`` (j < ``cnt[g]``, read on the device) of model g from the pool
    rows ``rows[src_idx[g, j]]``, consistently across masters, Adam moments, bf16 shadows and row norms
    (``csrc/resample.hip``).  ``dead_idx`` int32 [G, P], ``src_idx`` int64 [G, P], ``cnt`` int32 [G],
    ``rows`` bf16 [N, d], ``enc_scale`` fp32 [G]; the state tensors are the engine's ([G, n, d] fp32
    masters / moments, bf16 shadows, [G, n] bias and norms).  ``dec*`` None: a tied dictionary, whose
    encoder shadow is the normalised one.  Nothing here synchronises; the launch is graph-capturable."""
    if enc.dim() != 3:
        raise ValueError("enc must be [G, n, d]")
    G, n, d = enc.shape
    dev = enc.device
    if d % 256 or d > 4096:
        raise ValueError(f"resample_rows needs d % 256 == 0, d <= 4096 (got {d})")

    def need(t, name, dtype, shape):
        if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be contiguous {dtype} {tuple(shape)} on {dev}")

    if dead_idx.dim() != 2 or dead_idx.shape[0] != G or dead_idx.shape[1] < 1:
        raise ValueError("dead_idx must be int32 [G, P] with P >= 1")
    P = dead_idx.shape[1]
    need(dead_idx, "dead_idx", torch.int32, (G, P))
    need(src_idx, "src_idx", torch.int64, (G, P))
    need(cnt, "cnt", torch.int32, (G,))
    need(enc_scale, "enc_scale", torch.float32, (G,))
    if rows.dim() != 2 or rows.shape[0] < 1:
        raise ValueError("rows must be bf16 [N, d] with N >= 1")
    need(rows, "rows", torch.bfloat16, (rows.shape[0], d))
    for name, t in (("enc", enc), ("enc_m", enc_m), ("enc_v", enc_v)):
        need(t, name, torch.float32, (G, n, d))
    need(enc_shadow, "enc_shadow", torch.bfloat16, (G, n, d))
    for name, t in (("bias", bias), ("bias_m", bias_m), ("bias_v", bias_v), ("norms", norms)):
        need(t, name, torch.float32, (G, n))
    if dec is not None:
        for name, t in (("dec", dec), ("dec_m", dec_m), ("dec_v", dec_v)):
            if t is None:
                raise ValueError("an untied dictionary needs dec, dec_m, dec_v and dec_shadow")
            need(t, name, torch.float32, (G, n, d))
        if dec_shadow is None:
            raise ValueError("an untied dictionary needs dec, dec_m, dec_v and dec_shadow")
        need(dec_shadow, "dec_shadow", torch.bfloat16, (G, n, d))
    rc = _lib.lib().sc_resample_rows(
        _lib.ptr(dead_idx), _lib.ptr(src_idx), _lib.ptr(cnt), P, _lib.ptr(rows), rows.shape[0], _lib.ptr(enc_scale),
        int(bool(normalize_src)), int(bool(set_decoder)), int(bool(zero_bias)), _lib.ptr(enc), _lib.ptr(enc_m),
        _lib.ptr(enc_v), _lib.ptr(enc_shadow), _lib.ptr(dec), _lib.ptr(dec_m), _lib.ptr(dec_v), _lib.ptr(dec_shadow),
        _lib.ptr(bias), _lib.ptr(bias_m), _lib.ptr(bias_v), _lib.ptr(norms), G, n, d, _lib.stream_handle())
    _lib.check(rc, "sc_resample_rows")


def resample_dict_rows(dead_idx, src_idx, cnt, rows, scale, dict_, dict_m, dict_v, shadow, norms, *,
                       normalize_src: bool = True):
    """``resample_rows`` for a normalised dictionary with no bias and no separate decoder (the top-k
    ensembles): row ``dead_idx[g, j]`` (j < ``cnt[g]``, read on the device) of ``dict_`` fp32 [G, n, d] <-
    u scale[g] with u = x / max(|x|, 1e-8) of the pool row x = ``rows[src_idx[g, j]]`` (``normalize_src``;
    else x itself), its moments <- 0, and its normalised bf16 ``shadow`` row and ``norms`` entry rewritten
    with the bits of an ``adam.shadow_rows(normalize=True)`` pass.  Nothing here synchronises; the
    launch is graph-capturable."""
    if dict_.dim() != 3:
        raise ValueError("dict_ must be [G, n, d]")
    G, n, d = dict_.shape
    dev = dict_.device
    if d % 256 or d > 4096:
        raise ValueError(f"resample_dict_rows needs d % 256 == 0, d <= 4096 (got {d})")

    def need(t, name, dtype, shape):
        if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be contiguous {dtype} {tuple(shape)} on {dev}")

    if dead_idx.dim() != 2 or dead_idx.shape[0] != G or dead_idx.shape[1] < 1:
        raise ValueError("dead_idx must be int32 [G, P] with P >= 1")
    P = dead_idx.shape[1]
    need(dead_idx, "dead_idx", torch.int32, (G, P))
    need(src_idx, "src_idx", torch.int64, (G, P))
    need(cnt, "cnt", torch.int32, (G,))
    need(scale, "scale", torch.float32, (G,))
    if rows.dim() != 2 or rows.shape[0] < 1:
        raise ValueError("rows must be bf16 [N, d] with N >= 1")
    need(rows, "rows", torch.bfloat16, (rows.shape[0], d))
    for name, t in (("dict_", dict_), ("dict_m", dict_m), ("dict_v", dict_v)):
        need(t, name, torch.float32, (G, n, d))
    need(shadow, "shadow", torch.bfloat16, (G, n, d))
    need(norms, "norms", torch.float32, (G, n))
    rc = _lib.lib().sc_resample_dict_rows(
        _lib.ptr(dead_idx), _lib.ptr(src_idx), _lib.ptr(cnt), P, _lib.ptr(rows), rows.shape[0], _lib.ptr(scale),
        int(bool(normalize_src)), _lib.ptr(dict_), _lib.ptr(dict_m), _lib.ptr(dict_v), _lib.ptr(shadow),
        _lib.ptr(norms), G, n, d, _lib.stream_handle())
    _lib.check(rc, "sc_resample_dict_rows")
