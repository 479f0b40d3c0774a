"""Fire counts, dead-atom resampling and feature statistics of top-k ensembles: the torch oracles.

``FusedTopKEnsemble`` gets per-feature quantities from the select's picks (``idx`` int [G, B, kmax],
``val`` fp32 [G, B, kmax], per-model ``k``; slots at or past ``k[g]`` are the padding (0, 0.0)) without
densifying them (``ops/topk_stats.py``, ``ops/resample.py``).  This module is the same arithmetic in plain
torch, CPU included: what the tests compare the kernels against.  The pairing of dead atoms with pool
rows (``plan_resample``) and the result type (``FeatureStats``) are the SAE ensembles' own
(``engine/resample.py``, ``engine/feature_stats.py``).
"""

from __future__ import annotations

import torch

from .resample import FLOOR


def _slot_mask(idx: torch.Tensor, val: torch.Tensor, k, n: int) -> torch.Tensor:
    if idx.dim() != 3 or tuple(val.shape) != tuple(idx.shape):
        raise ValueError("idx and val must be [G, B, kmax]")
    G, _, kmax = idx.shape
    k = torch.as_tensor(k, device=idx.device).reshape(-1)
    if k.numel() != G:
        raise ValueError(f"k must have one entry per model ({G})")
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
        raise ValueError(f"picks outside [0, {n})")
    return torch.arange(kmax, device=idx.device).view(1, 1, kmax) < k.view(G, 1, 1)


@torch.no_grad()
def pick_counts_reference(idx: torch.Tensor, val: torch.Tensor, k, n: int) -> torch.Tensor:
    """int64 [G, n]: how many rows fire feature j -- the slots s < k[g] with val > 0 (a pick the ReLU
    clamped to 0 is not a firing; the padded slots never count)."""
    G = idx.shape[0]
    on = _slot_mask(idx, val, k, n) & (val > 0)
    out = torch.zeros(G, n, dtype=torch.int64, device=idx.device)
    for g in range(G):
        out[g] = torch.bincount(idx[g][on[g]].long().reshape(-1), minlength=n)
    return out


@torch.no_grad()
def dense_codes_from_picks(idx: torch.Tensor, val: torch.Tensor, k, n: int) -> torch.Tensor:
    """fp32 [G, B, n]: the dense codes of the picks, by ``scatter_add`` of ``val`` over the first k[g]
    slots (real indices are unique in a row; a masked slot adds 0 to feature 0)."""
    G, B, _ = idx.shape
    keep = _slot_mask(idx, val, k, n)
    v = torch.where(keep, val.float(), torch.zeros((), device=val.device))
    i = torch.where(keep, idx.long(), torch.zeros((), dtype=torch.int64, device=idx.device))
    return torch.zeros(G, B, n, dtype=torch.float32, device=idx.device).scatter_add_(-1, i, v)


@torch.no_grad()
def resample_dict_scales(dict_: torch.Tensor, dead: torch.Tensor, ratio: float = 1.0) -> torch.Tensor:
    """Per-model scale [G] of a resampling event on the dictionary masters ``dict_`` [G, n, d] BEFORE the
    rewrite: ``ratio`` x the mean row norm of the alive (not dead) atoms, or of all atoms when none is
    alive."""
    nrm = torch.linalg.vector_norm(dict_.float(), dim=-1)
    af = (~dead).to(nrm.dtype)
    n_alive = af.sum(1)
    mean_alive = (nrm * af).sum(1) / n_alive.clamp(min=1.0)
    return (ratio * torch.where(n_alive > 0, mean_alive, nrm.mean(1))).float().contiguous()


@torch.no_grad()
def resample_dict_reference(dict_: torch.Tensor, m: torch.Tensor, v: torch.Tensor, dead_idx: torch.Tensor,
                            src_idx: torch.Tensor, cnt: torch.Tensor, rows: torch.Tensor, scale: torch.Tensor):
    """The arithmetic of ``sc_resample_dict_rows`` in fp32 torch, in place on the stacked [G, n, d]
    tensors: for f = dead_idx[g, j], j < cnt[g], and x = float(rows[src_idx[g, j]]), dict row f <-
    x / max(|x|, 1e-8) * scale[g] and its moments <- 0.  Every other row is left as it is."""
    counts = [int(c) for c in cnt.detach().cpu()]
    for g, c in enumerate(counts):
        if c <= 0:
            continue
        f = dead_idx[g, :c].long()
        x = rows[src_idx[g, :c].long()].to(dict_.device, torch.float32)
        unit = x / torch.linalg.vector_norm(x, dim=-1, keepdim=True).clamp(min=FLOOR)
        dict_[g, f] = unit * scale[g].to(torch.float32)
        m[g, f] = 0
        v[g, f] = 0
