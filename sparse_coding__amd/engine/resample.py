"""Dead-feature resampling for stacked SAE ensembles: the policy and the torch oracle.

At a resampling event a candidate pool of activation rows is scored forward-only; features that never
fire on it are *dead* and are re-seeded from badly reconstructed pool rows (Anthropic, "Towards
Monosemanticity", appendix on neuron resampling; reference ``experiments/huge_batch_size.py:224-250``
is the un-normalised, encoder-only special case).  This module holds what is the same for every
engine:

* ``plan_resample``: which pool row re-seeds which dead feature, built on the device with no host sync;
* ``resample_scales`` / ``RULES``: the two rewrite rules;
* ``resample_rows_reference``: the rewrite in fp32 torch over the stacked ``[G, n, d]`` dictionaries --
  the CPU implementation and the oracle of the gfx950 kernel (``ops/csrc/resample.hip``);
* ``resample_stacked``: the whole event in torch for the eager / analytic engines.
"""

from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

FLOOR = 1e-8

# rule -> kernel flags (normalize_src, set_decoder, zero_bias)
RULES = {
    # huge_batch_size.py:236-250: encoder rows only, from the raw example; decoder and bias values stay
    "reference": dict(normalize_src=False, set_decoder=False, zero_bias=False),
    # Anthropic: unit decoder row, encoder = that direction at a fraction of the alive encoder norm, bias 0
    "anthropic": dict(normalize_src=True, set_decoder=True, zero_bias=True),
}
PICKS = ("worst", "loss_sq")


def _check(rule: str, pick: str):
    if rule not in RULES:
        raise ValueError(f"rule must be one of {sorted(RULES)}, got {rule!r}")
    if pick not in PICKS:
        raise ValueError(f"pick must be one of {PICKS}, got {pick!r}")


@torch.no_grad()
def plan_resample(dead: torch.Tensor, err: torch.Tensor, *, pick: str = "worst",
                  generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Pair dead features with pool rows.  ``dead`` bool [G, n]; ``err`` [G, N] per-row reconstruction
    errors of the pool.  Returns ``(dead_idx int32 [G, P], src_idx int64 [G, P], cnt int32 [G])`` with
    P = min(n, N): for j < cnt[g] feature dead_idx[g, j] is re-seeded from pool row src_idx[g, j];
    entries past cnt[g] are padding (valid indices, never applied).  The dead indices ascend per model,
    cnt[g] = min(n_dead[g], N), the rows are distinct within a model.  ``pick="worst"``: the rows by
    descending error; ``pick="loss_sq"``: sampled without replacement with probability proportional to
    err^2 (Gumbel top-k on 2 log err, ``generator``).  Every op runs on ``err``'s device, unsynchronised."""
    if pick not in PICKS:
        raise ValueError(f"pick must be one of {PICKS}, got {pick!r}")
    if dead.dim() != 2 or err.dim() != 2 or dead.shape[0] != err.shape[0] or dead.dtype != torch.bool:
        raise ValueError("dead must be bool [G, n] and err [G, N]")
    n, N = dead.shape[1], err.shape[1]
    P = min(n, N)
    cnt = dead.sum(dim=1).clamp(max=N).to(torch.int32)
    # stable argsort of ~dead: the dead features first, each group in ascending index order
    dead_idx = torch.argsort((~dead).to(torch.uint8), dim=1, stable=True)[:, :P].to(torch.int32).contiguous()
    key = err.float()
    if pick == "loss_sq":
        gdev = generator.device if generator is not None else err.device
        u = torch.rand(err.shape, generator=generator, device=gdev).to(err.device)
        u = u.clamp(min=torch.finfo(torch.float32).tiny)
        key = 2.0 * torch.log(key) - torch.log(-torch.log(u))
    src_idx = torch.sort(key, dim=1, descending=True, stable=True).indices[:, :P].contiguous()
    return dead_idx, src_idx, cnt


@torch.no_grad()
def resample_scales(enc: torch.Tensor, dead: torch.Tensor, live: Optional[torch.Tensor], *, rule: str = "reference",
                    ratio: float = 0.2) -> torch.Tensor:
    """Per-model encoder scale [G] of a resampling event, from the encoder masters ``enc`` [G, n, d]
    BEFORE the rewrite.  ``live`` bool [G, n]: the rows that exist (masked ensembles), None = all.
    ``reference``: ratio / mean |enc_row| over the live rows (the reference divides by the mean norm,
    huge_batch_size.py:236-238; kept).  ``anthropic``: ratio x mean |enc_row| over the alive (live, not
    dead) rows, or over all live rows when none is alive."""
    if rule not in RULES:
        raise ValueError(f"rule must be one of {sorted(RULES)}, got {rule!r}")
    nrm = torch.linalg.vector_norm(enc.float(), dim=-1)
    lv = torch.ones_like(dead) if live is None else live
    lf = lv.to(nrm.dtype)
    mean_live = (nrm * lf).sum(1) / lf.sum(1).clamp(min=1.0)
    if rule == "reference":
        return (ratio / mean_live).float().contiguous()
    af = (lv & ~dead).to(nrm.dtype)
    n_alive = af.sum(1)
    mean_alive = (nrm * af).sum(1) / n_alive.clamp(min=1.0)
    return (ratio * torch.where(n_alive > 0, mean_alive, mean_live)).float().contiguous()


@torch.no_grad()
def resample_rows_reference(params: Dict[str, torch.Tensor], m: Dict[str, torch.Tensor], v: Dict[str, torch.Tensor],
                            dead_idx: torch.Tensor, src_idx: torch.Tensor, cnt: torch.Tensor, rows: torch.Tensor,
                            enc_scale: torch.Tensor, *, normalize_src: bool, set_decoder: bool, zero_bias: bool,
                            kind: str, bias_key: str = "encoder_bias"):
    """The arithmetic of ``sc_resample_rows`` in fp32 torch, in place on the stacked dictionaries
    (``params`` / ``m`` / ``v``: dicts with "encoder" [G, n, d], ``bias_key`` [G, n] and, for
    ``kind="untied"``, "decoder").  For f = dead_idx[g, j], j < cnt[g], and x = float(rows[src_idx[g, j]]):
    encoder row <- u enc_scale[g] with u = x / max(|x|, 1e-8) (``normalize_src``) or x; decoder row <-
    x / max(|x|, 1e-8) if ``set_decoder`` (untied only; ignored for tied); bias <- 0 if ``zero_bias``;
    the moments of all three <- 0.  Every other row is left as it is."""
    if kind not in ("untied", "tied"):
        raise ValueError(f"kind must be 'untied' or 'tied', got {kind!r}")
    G = params["encoder"].shape[0]
    counts = [int(c) for c in cnt.detach().cpu()]
    for g in range(G):
        k = counts[g]
        if k <= 0:
            continue
        f = dead_idx[g, :k].long()
        x = rows[src_idx[g, :k].long()].to(params["encoder"].device, torch.float32)
        unit = x / torch.linalg.vector_norm(x, dim=-1, keepdim=True).clamp(min=FLOOR)
        u = unit if normalize_src else x
        params["encoder"][g, f] = u * enc_scale[g].to(torch.float32)
        m["encoder"][g, f] = 0
        v["encoder"][g, f] = 0
        if kind == "untied":
            if set_decoder:
                params["decoder"][g, f] = unit
            m["decoder"][g, f] = 0
            v["decoder"][g, f] = 0
        if zero_bias:
            params[bias_key][g, f] = 0
        m[bias_key][g, f] = 0
        v[bias_key][g, f] = 0


@torch.no_grad()
def resample_stacked(params, m, v, rows: torch.Tensor, kind: str, *, live: Optional[torch.Tensor] = None,
                     rule: str = "reference", pick: str = "worst", ratio: float = 0.2,
                     generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """One resampling event in fp32 torch on stacked SAE dictionaries (the eager / analytic engines, the
    CPU): a feature is dead when it never fires on ``rows`` [N, d]; the per-row error is
    ((x_hat - x)^2).sum(-1).  ``live`` bool [G, n]: the rows that exist (masked ensembles).  Edits
    ``params`` / ``m`` / ``v`` in place and returns the per-model counts [G] (int32)."""
    _check(rule, pick)
    enc = params["encoder"]
    x = rows.to(enc.device, torch.float32)
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] != enc.shape[-1]:
        raise ValueError(f"rows must be [N >= 1, {enc.shape[-1]}], got {tuple(rows.shape)}")

    def unit(w):
        return w / torch.linalg.vector_norm(w, dim=-1, keepdim=True).clamp(min=FLOOR)

    w_e = unit(enc) if kind == "tied" else enc
    w_d = w_e if kind == "tied" else unit(params["decoder"])
    c = torch.baddbmm(params["encoder_bias"].unsqueeze(1), x.expand(enc.shape[0], *x.shape),
                      w_e.transpose(1, 2)).clamp_(min=0.0)
    if live is not None:
        c = c * live.unsqueeze(1).to(c.dtype)
    err = (torch.bmm(c, w_d) - x).pow(2).sum(-1)
    dead = ~(c > 0).any(dim=1)
    if live is not None:
        dead &= live
    dead_idx, src_idx, cnt = plan_resample(dead, err, pick=pick, generator=generator)
    scale = resample_scales(enc, dead, live, rule=rule, ratio=ratio)
    resample_rows_reference(params, m, v, dead_idx, src_idx, cnt, x, scale, kind=kind, **RULES[rule])
    return cnt
