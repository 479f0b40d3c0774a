"""Per-feature activation statistics of an ensemble: the result type, the fp64 torch oracle and the
fp32 torch code path of the engines without kernels.

``FusedSAEEnsemble.feature_stats`` fills a ``FeatureStats`` from the bf16 codes of the grouped encoder
launch with two column-reduction kernels (``ops/feature_stats.py``); ``feature_stats_reference`` computes
the same object from any iterable of code tensors in fp64 torch (CPU included) and is what the tests
compare against.  The derived moments use the formulas and clamps of ``eval.metrics.calc_moments_streaming``
(reference standard_metrics.py:454-509), which does the same for one model at a time.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, Optional, Tuple

import torch

MAX_TOPK = 32


@dataclass
class FeatureStats:
    """Raw per-feature statistics of ``n_rows`` rows for G models with n features each."""

    n_rows: int
    count: torch.Tensor               # int64 [G, n]   rows on which the feature's code is non-zero
    sums: torch.Tensor                # fp64 [G, 4, n]  sum c, sum c^2, sum c^3, sum c^4
    max: torch.Tensor                 # fp32 [G, n]    largest code
    top_vals: Optional[torch.Tensor] = None   # fp32 [G, n, K]  K largest positive codes, descending; 0 = empty
    top_rows: Optional[torch.Tensor] = None   # int64 [G, n, K] their global row indices; -1 = empty

    # ------------------------------------------------------------------ derived moments
    def _raw(self):
        n = max(1, int(self.n_rows))
        return tuple(self.sums[:, p] / n for p in range(4))

    @property
    def frequency(self) -> torch.Tensor:
        return (self.count.double() / max(1, int(self.n_rows))).float()

    @property
    def mean(self) -> torch.Tensor:
        return self._raw()[0].float()

    @property
    def var(self) -> torch.Tensor:
        mean, m2, _, _ = self._raw()
        return (m2 - mean ** 2).float()

    @property
    def skew(self) -> torch.Tensor:
        mean, m2, m3, _ = self._raw()
        var = m2 - mean ** 2
        return (m3 / torch.clamp(var ** 1.5, min=1e-8)).float()

    @property
    def kurtosis(self) -> torch.Tensor:
        mean, m2, _, m4 = self._raw()
        var = m2 - mean ** 2
        return (m4 / torch.clamp(var ** 2, min=1e-8)).float()

    @property
    def m4(self) -> torch.Tensor:
        return self._raw()[3].float()

    @property
    def topk(self) -> int:
        return 0 if self.top_vals is None else int(self.top_vals.shape[-1])

    def per_model(self, g: int):
        """(times_active, mean, var, skew, kurtosis, m4) of model ``g``, as ``calc_moments_streaming``."""
        return (self.count[g].float(), self.mean[g], self.var[g], self.skew[g], self.kurtosis[g], self.m4[g])

    def top_rows_of(self, g: int, feat: int, k: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(rows, values) of the up to ``k`` largest activations of feature ``feat`` of model ``g``, largest
        first, on the CPU (empty slots dropped).  For a pool of fragments of L tokens each, the fragment is
        ``row // L`` and the token ``row % L``."""
        if self.top_rows is None:
            raise ValueError("these statistics were collected without a top-k list (topk=0)")
        k = self.topk if k is None else int(k)
        if not 1 <= k <= self.topk:
            raise ValueError(f"k must be in [1, {self.topk}], got {k}")
        rows = self.top_rows[g, feat, :k].cpu()
        vals = self.top_vals[g, feat, :k].cpu()
        keep = rows >= 0
        return rows[keep], vals[keep]

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        sd = {"n_rows": torch.tensor(int(self.n_rows), dtype=torch.int64), "count": self.count, "sums": self.sums,
              "max": self.max}
        if self.top_vals is not None:
            sd["top_vals"], sd["top_rows"] = self.top_vals, self.top_rows
        return sd

    def save(self, path):
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, map_location="cpu") -> "FeatureStats":
        sd = torch.load(path, map_location=map_location, weights_only=True)
        return cls(n_rows=int(sd["n_rows"]), count=sd["count"], sums=sd["sums"], max=sd["max"],
                   top_vals=sd.get("top_vals"), top_rows=sd.get("top_rows"))

    def to(self, device) -> "FeatureStats":
        mv = lambda t: None if t is None else t.to(device)
        return FeatureStats(self.n_rows, mv(self.count), mv(self.sums), mv(self.max), mv(self.top_vals),
                            mv(self.top_rows))


def check_request(topk: int, row_offset: int, state: Optional[FeatureStats], G: int, n: int):
    """Validate the ``topk`` / ``row_offset`` / ``state`` arguments of a ``feature_stats`` call."""
    topk, row_offset = int(topk), int(row_offset)
    if not 0 <= topk <= MAX_TOPK:
        raise ValueError(f"topk must be in [0, {MAX_TOPK}], got {topk}")
    if row_offset < 0:
        raise ValueError(f"row_offset must be >= 0, got {row_offset}")
    if state is not None:
        if not isinstance(state, FeatureStats):
            raise ValueError("state must be the FeatureStats of an earlier call")
        if tuple(state.count.shape) != (G, n) or tuple(state.sums.shape) != (G, 4, n) \
                or tuple(state.max.shape) != (G, n):
            raise ValueError(f"state is for another ensemble (count {tuple(state.count.shape)}, this one [{G}, {n}])")
        if state.topk != topk:
            raise ValueError(f"state carries top-{state.topk} lists, this call asks for topk={topk}")
    return topk, row_offset


def empty_topk(G: int, n: int, K: int, device=None):
    return (torch.zeros(G, n, K, dtype=torch.float32, device=device),
            torch.full((G, n, K), -1, dtype=torch.int64, device=device))


def open_accumulators(state: Optional[FeatureStats], G: int, n: int, topk: int, device, max0: float):
    """``(acc, mx, tv, tr, seen)`` of an engine's ``feature_stats`` loop, fresh or continuing ``state``: ``acc``
    fp64 [G, 5, n] (count, sum c .. sum c^4), ``mx`` fp32 [G, n] starting at ``max0`` (what a feature that
    never fires reads: -inf from a dense reduction, 0 from the picks), the top-K lists (``topk`` > 0) and the
    rows already seen.  Copies of the state's tensors: the state itself is left as it is."""
    tv = tr = None
    if state is None:
        acc = torch.zeros(G, 5, n, device=device, dtype=torch.float64)
        mx = torch.full((G, n), max0, device=device)
        if topk:
            tv, tr = empty_topk(G, n, topk, device)
        return acc, mx, tv, tr, 0
    acc = torch.cat([state.count.to(device, torch.float64).unsqueeze(1), state.sums.to(device)], dim=1).contiguous()
    mx = state.max.to(device, copy=True).contiguous()
    if topk:
        tv = state.top_vals.to(device, copy=True).contiguous()
        tr = state.top_rows.to(device, copy=True).contiguous()
    return acc, mx, tv, tr, int(state.n_rows)


def merge_topk_reference(top_vals: torch.Tensor, top_rows: torch.Tensor, c: torch.Tensor, row0: int):
    """The top-K merge on its own: the lists [G, n, K] after the batch of codes ``c`` [G, B, n] with global
    rows ``row0 .. row0 + B - 1``.  Previous entries first, then the candidates in row order, one stable
    descending sort over the values: equal values keep that order.  Only positive values are kept."""
    G, B, n = c.shape
    K = top_vals.shape[-1]
    cand = c.float().transpose(1, 2)
    rows = (int(row0) + torch.arange(B, dtype=torch.int64, device=c.device)).expand(G, n, B)
    vals = torch.cat([top_vals.float(), cand], dim=-1)
    rows = torch.cat([top_rows, rows], dim=-1)
    vals = torch.where(vals > 0, vals, torch.zeros_like(vals))  # (non-positive and NaN candidates never enter)
    vals, order = torch.sort(vals, dim=-1, descending=True, stable=True)
    vals, rows = vals[..., :K], torch.gather(rows, -1, order)[..., :K]
    keep = vals > 0
    return (torch.where(keep, vals, torch.zeros_like(vals)).contiguous(),
            torch.where(keep, rows, torch.full_like(rows, -1)).contiguous())


def feature_stats_reference(code_batches: Iterable[torch.Tensor], topk: int = 0, row_offset: int = 0,
                            state: Optional[FeatureStats] = None) -> FeatureStats:
    """fp64 torch oracle: the ``FeatureStats`` of the code tensors ``code_batches`` (each [G, B, n], any
    float dtype, B may vary), continuing ``state`` when given; the first row is row ``row_offset``."""
    first = True
    count = sums = mx = tv = tr = None
    n_rows = 0
    row = int(row_offset)
    for c in code_batches:
        if c.dim() != 3:
            raise ValueError(f"codes must be [G, B, n], got {tuple(c.shape)}")
        G, B, n = c.shape
        if first:
            topk, row = check_request(topk, row_offset, state, G, n)
            dev = c.device
            if state is None:
                count = torch.zeros(G, n, dtype=torch.int64, device=dev)
                sums = torch.zeros(G, 4, n, dtype=torch.float64, device=dev)
                mx = torch.full((G, n), float("-inf"), dtype=torch.float32, device=dev)
                if topk:
                    tv, tr = empty_topk(G, n, topk, dev)
            else:
                n_rows = int(state.n_rows)
                count, sums, mx = state.count.clone().to(dev), state.sums.clone().to(dev), state.max.clone().to(dev)
                if topk:
                    tv, tr = state.top_vals.clone().to(dev), state.top_rows.clone().to(dev)
            first = False
        cd = c.double()
        count += (cd != 0).sum(1)
        for p in range(4):
            sums[:, p] += (cd ** (p + 1)).sum(1)
        mx = torch.maximum(mx, c.float().amax(1))
        if topk:
            tv, tr = merge_topk_reference(tv, tr, c, row)
        row += B
        n_rows += B
    if first:
        raise ValueError("feature_stats_reference needs at least one batch of codes")
    return FeatureStats(n_rows, count, sums, mx, tv, tr)


def stacked_codes(params, buffers, kind: str, x: torch.Tensor) -> torch.Tensor:
    """fp32 torch codes [G, B, n] of the stacked untied / tied SAE parameters on the rows ``x`` [B, d]
    (the analytic and eager engines' forward pass: unit-norm tied rows, fixed affine centering, masked
    features zero)."""
    from ..models.signatures import unit_rows

    w = params["encoder"].detach().float()
    if kind == "tied":
        w = unit_rows(w)
    x = x.to(w.device, torch.float32)
    if kind == "tied" and "center_rot" in buffers:
        xc = (x.unsqueeze(0) - buffers["center_trans"].float().unsqueeze(1)) \
            @ buffers["center_rot"].float().transpose(-1, -2)
        xc = xc * buffers["center_scale"].float().unsqueeze(1)
    else:
        xc = x.unsqueeze(0).expand(w.shape[0], *x.shape)
    c = torch.baddbmm(params["encoder_bias"].detach().float().unsqueeze(1), xc, w.transpose(1, 2)).clamp(min=0.0)
    if "coef_mask" in buffers:
        c = c * (~buffers["coef_mask"].bool()).float().reshape(w.shape[0], 1, -1)
    return c
