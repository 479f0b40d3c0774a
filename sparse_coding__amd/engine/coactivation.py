"""Co-activation partners per feature from sparse codes, across models: the result type, the torch oracle and
the device route.

Two dictionaries are compared on their atoms by ``atom_matches`` / ``nearest_atoms``; this module compares them
on their ACTIVATIONS: which features fire on the same rows, and how correlated their codes are.  Inputs are two
sets of complete sparse codes over the same N rows, source ``A`` (G_a models, n_a features) and target ``B``
(G_b models, n_b features; ``B`` may be ``A`` itself).  For source model g, feature f, target model h, feature j:

- ``both[g, h, f, j]``: the rows on which both fire (int32).
- ``dot[g, h, f, j]``: the sum of ``a_r * b_r`` over those rows in fp32, in ascending row order, ``acc <-
  fmaf(a_r, b_r, acc)`` from 0.  The codes of both fused engines are bf16-valued, so every product is exact in
  fp32 and ``acc + a * b`` in torch fp32 has the same bits.
- per feature, from its list, in fp64 in a fixed order (``list_moments_reference``): ``cnt``, ``s1`` = the sum of
  its codes, ``s2`` = the sum of their squares.  From these, in fp64 torch ops rounded once to fp32
  (``shift_scale``): ``shift = s1 / sqrt(N)`` for ``pearson``, 0 for ``cosine``; ``scale = 1 / sqrt(s2 -
  shift^2)``, 0 where that radicand is <= 0 or the feature never fires.
- **score**, in fp32 with unfused operations: ``pearson`` / ``cosine``: ``((dot - shift_a shift_b) scale_a)
  scale_b``; ``jaccard``: ``float(both) / float(cnt_a + cnt_b - both)``.  A result of -0.0 is written +0.0.
- **candidates** of (g, h, f): the columns j with ``both >= min_both`` (>= 1); with ``exclude_self``, A is B
  and g == h, column f is not one.
- **partners**: the m best candidates (0 <= m <= 32), score descending, then column ascending; empty slots
  read ``(partner -1, score 0.0, both 0, dot 0.0)``.
- **skip rule** (that of ``by_feature``): a row of either side is left out whole unless its pointers are
  ordered and within the buffers, it has at most n entries and every column lies in ``[0, lim)``.  The rows
  left out are the ``skipped`` of each side's own ``by_feature()``; ``cnt`` / ``s1`` / ``s2`` are over the
  surviving rows.  Rows with a repeated column are outside the contract.

There is no ``state=``: the m best of a sum cannot be merged across chunks of rows, so a pool is given whole.
All outputs are integers or fp32 values computed in a fixed order: the oracle compares with ``torch.equal``.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from ..ops.coactivation import SCORES, check_m, check_min_both, check_score, check_width   # (plain Python: no
#                                                                                kernel library is loaded)
from .feature_codes import FeatureCodes, by_feature, feature_codes_reference
from .sparse_codes import SparseCodes


class CoActivationSkipped(RuntimeError):
    """Rows were left out of a ``CoActivation``: the sparse codes of one side were not all stored, or not valid."""


@dataclass
class CoActivation:
    """The ``m`` best co-activation partners in every target model h for every feature of every source model g."""

    partner: torch.Tensor     # int32 [Ga, Gb, n_a, m]  feature of model h; -1: empty slot
    score: torch.Tensor       # fp32 [Ga, Gb, n_a, m]   descending; 0.0: empty slot
    both: torch.Tensor        # int32 [Ga, Gb, n_a, m]  rows on which both fire
    dot: torch.Tensor         # fp32 [Ga, Gb, n_a, m]   sum of the products of their codes over those rows
    cnt_a: torch.Tensor       # int32 [Ga, n_a]         rows on which each source feature fires
    cnt_b: torch.Tensor       # int32 [Gb, n_b]
    skipped_a: torch.Tensor   # int64 [Ga]              source rows left out by the skip rule
    skipped_b: torch.Tensor   # int64 [Gb]
    score_kind: str
    min_both: int
    n_rows: int

    _TENSORS = ("partner", "score", "both", "dot", "cnt_a", "cnt_b", "skipped_a", "skipped_b")

    @property
    def m(self) -> int:
        return int(self.partner.shape[-1])

    def pair(self, g: int, h: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(partner, score, both, dot), [n_a, m] each, of model g's features against model h."""
        return self.partner[g, h], self.score[g, h], self.both[g, h], self.dot[g, h]

    def best(self, g: int, h: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(partner [n_a], score [n_a]): the first slot of every feature of model g against model h."""
        if self.m < 1:
            raise ValueError("best() needs m >= 1")
        return self.partner[g, h, :, 0], self.score[g, h, :, 0]

    def mean_best(self) -> torch.Tensor:
        """[Ga, Gb] fp32: entry (g, h) is the mean over model g's firing features of the score of their best
        partner in model h (0.0 where they have none): the activation-side analogue of ``AtomMatches.mmcs()``.
        A model without a firing feature reads 0."""
        if self.m < 1:
            raise ValueError("mean_best() needs m >= 1")
        fires = (self.cnt_a > 0).to(torch.float64)
        tot = (self.score[..., 0].double() * fires[:, None, :]).sum(-1)
        return (tot / fires.sum(-1).clamp(min=1)[:, None]).float()

    def agreement(self, atom_matches) -> torch.Tensor:
        """[Ga, Gb] fp32: the share of model g's features with a partner in model h whose best partner by
        activation is also their nearest atom (``atom_matches``: the ``AtomMatches`` of the same models, or an
        int tensor [Ga, Gb, n_a] / [Ga, Gb, n_a, m'] of nearest-atom indices).  0 where no feature has one."""
        if self.m < 1:
            raise ValueError("agreement() needs m >= 1")
        idx = getattr(atom_matches, "idx", atom_matches)
        idx = idx[..., 0] if idx.dim() == 4 else idx
        mine = self.partner[..., 0]
        if tuple(idx.shape) != tuple(mine.shape):
            raise ValueError(f"nearest-atom indices must be {list(mine.shape)}, got {list(idx.shape)}")
        has = mine >= 0
        same = (has & (mine == idx.to(mine.device))).sum(-1).double()
        return (same / has.sum(-1).clamp(min=1).double()).float()

    def check(self) -> "CoActivation":
        """Synchronises; raises ``CoActivationSkipped`` if either side left rows out."""
        sa, sb = self.skipped_a.cpu(), self.skipped_b.cpu()
        if bool((sa != 0).any()) or bool((sb != 0).any()):
            raise CoActivationSkipped(f"{sa.tolist()} source and {sb.tolist()} target rows per model were skipped "
                                      f"(of {self.n_rows}): their sparse codes were not all stored -- encode with a "
                                      "larger budget, or budget=None")
        return self

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        sd = {k: getattr(self, k) for k in self._TENSORS}
        sd["score_kind"] = torch.tensor(SCORES.index(self.score_kind), dtype=torch.int64)
        sd["min_both"] = torch.tensor(int(self.min_both), dtype=torch.int64)
        sd["n_rows"] = torch.tensor(int(self.n_rows), dtype=torch.int64)
        return sd

    def save(self, path):
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, map_location="cpu") -> "CoActivation":
        sd = torch.load(path, map_location=map_location, weights_only=True)
        return cls(*(sd[k] for k in cls._TENSORS), SCORES[int(sd["score_kind"])], int(sd["min_both"]),
                   int(sd["n_rows"]))

    def to(self, device) -> "CoActivation":
        return CoActivation(*(getattr(self, k).to(device) for k in self._TENSORS), self.score_kind, self.min_both,
                            self.n_rows)


# ---------------------------------------------------------------------- moments, shift and scale
def list_moments_reference(fc: FeatureCodes):
    """Torch oracle of ``ops.coactivation.list_moments`` (any device): ``(cnt int32, s1 fp64, s2 fp64)``, [G, n]
    each, in the kernel's order -- entry i of a list goes to lane ``i % 64``, a lane adds its entries in
    ascending order from 0.0, then the lanes are combined by the xor butterfly 1, 2, 4, 8, 16, 32."""
    G, n, dev = fc.n_models, fc.n, fc.row.device
    ptr = torch.cummax(fc.col_ptr.clamp(min=0, max=fc.cap), 1).values
    cnt = (ptr[:, 1:] - ptr[:, :-1])
    chunks = max(1, -(-int(cnt.max()) // 64)) if cnt.numel() else 1
    pos = torch.arange(chunks * 64, device=dev)
    s1 = torch.zeros(G, n, 64, dtype=torch.float64, device=dev)
    s2 = torch.zeros(G, n, 64, dtype=torch.float64, device=dev)
    lanes = torch.arange(64, device=dev)
    for g in range(G):
        at = ptr[g, :-1, None] + pos                                  # [n, chunks * 64]
        live = pos < cnt[g, :, None]
        c = torch.zeros(n, chunks * 64, dtype=torch.float64, device=dev)
        if fc.cap:
            c = torch.where(live, fc.val[g][at.clamp(max=fc.cap - 1)].double(), c)
        c = c.view(n, chunks, 64)
        for q in range(chunks):                                        # (adding 0.0 changes nothing)
            s1[g] = s1[g] + c[:, q]
            s2[g] = s2[g] + c[:, q] * c[:, q]
    for o in (1, 2, 4, 8, 16, 32):
        s1 = s1 + s1[..., lanes ^ o]
        s2 = s2 + s2[..., lanes ^ o]
    return cnt.to(torch.int32), s1[..., 0].contiguous(), s2[..., 0].contiguous()


def shift_scale(cnt: torch.Tensor, s1: torch.Tensor, s2: torch.Tensor, n_rows: int, score: str):
    """``(shift fp32, scale fp32)`` per feature from its moments (module docstring): separate fp64 torch
    operations (IEEE on every device), rounded once to fp32.  ``jaccard`` uses neither: zeros."""
    score = check_score(score)
    if score == "jaccard":
        z = torch.zeros_like(s1, dtype=torch.float32)
        return z, z.clone()
    # (tensor by tensor: a division by a Python scalar may run as a multiplication by its reciprocal)
    shift = s1 / torch.full_like(s1, math.sqrt(n_rows)) if score == "pearson" else torch.zeros_like(s1)
    rad = s2 - shift * shift
    ok = (rad > 0) & (cnt > 0)
    one = torch.ones_like(rad)
    scale = torch.where(ok, one / torch.sqrt(torch.where(ok, rad, one)), torch.zeros_like(rad))
    return shift.float().contiguous(), scale.float().contiguous()


# ---------------------------------------------------------------------- the oracle
def _dense(fc: FeatureCodes, g: int):
    """(codes fp32 [N, n], fires bool [N, n]) of model ``g`` from its lists (the rows that passed the skip rule)."""
    feats = fc.entry_features(g)
    k = feats.numel()
    rows = fc.row[g, :k].long()
    dense = torch.zeros(fc.n_rows, fc.n, dtype=torch.float32, device=fc.row.device)
    fires = torch.zeros(fc.n_rows, fc.n, dtype=torch.bool, device=fc.row.device)
    dense[rows, feats] = fc.val[g, :k]
    fires[rows, feats] = True
    return dense, fires


def topm_partners(score: torch.Tensor, cand: torch.Tensor, both: torch.Tensor, dot: torch.Tensor, m: int):
    """The m best candidates of every row of ``score`` [n_a, n_b]: score descending, then column ascending (a
    stable sort); empty slots (-1, 0.0, 0, 0.0).  Returns (partner int32, score, both int32, dot), [n_a, m]."""
    n_a, n_b = score.shape
    s = torch.where(cand, score, torch.full_like(score, float("-inf")))
    order = torch.sort(s, dim=-1, descending=True, stable=True).indices[:, :m]
    live = torch.gather(cand, 1, order)
    if order.shape[1] < m:
        pad = m - order.shape[1]
        order = torch.cat([order, order.new_zeros(n_a, pad)], 1)
        live = torch.cat([live, live.new_zeros(n_a, pad)], 1)
    pick = lambda t, fill: torch.where(live, torch.gather(t, 1, order), torch.full((), fill, dtype=t.dtype,
                                                                                    device=t.device))
    return (torch.where(live, order, torch.full_like(order, -1)).to(torch.int32), pick(score, 0.0),
            pick(both, 0), pick(dot, 0.0))


def _check_pair(sc_a: SparseCodes, sc_b: SparseCodes):
    if sc_a.n_rows != sc_b.n_rows:
        raise ValueError(f"co-activation needs the same rows on both sides, got {sc_a.n_rows} and {sc_b.n_rows}")
    if sc_a.col.device != sc_b.col.device:
        raise ValueError("co-activation needs both sides on one device")
    check_width(sc_b.n)


def dense_sums_reference(fa: FeatureCodes, fb: FeatureCodes):
    """``(both int32, dot fp32)``, [Ga, Gb, n_a, n_b] each, of two feature-major codes over the same rows: the
    dense accumulators of the oracle.  ``dot`` is added row by row in ascending order, ``acc + a * b`` in fp32,
    only where both fire."""
    N, dev = fa.n_rows, fa.row.device
    da = [_dense(fa, g) for g in range(fa.n_models)]
    db = da if fb is fa else [_dense(fb, h) for h in range(fb.n_models)]
    A, Af = torch.stack([d[0] for d in da]), torch.stack([d[1] for d in da])        # [Ga, N, n_a]
    B, Bf = torch.stack([d[0] for d in db]), torch.stack([d[1] for d in db])        # [Gb, N, n_b]
    both = torch.einsum("grf,hrj->ghfj", Af.double(), Bf.double()).to(torch.int32)
    dot = torch.zeros(both.shape, dtype=torch.float32, device=dev)
    for r in torch.nonzero(Af.any(2).any(0) & Bf.any(2).any(0)).flatten().tolist():
        # (a silent feature reads 0: its product is a zero and adding it changes no bit)
        dot += A[:, None, r, :, None] * B[None, :, r, None, :]
    return both, dot


def coactivation_reference(sc_a: SparseCodes, sc_b: Optional[SparseCodes] = None, *, m: int = 4,
                           score: str = "pearson", min_both: int = 1, exclude_self: bool = True,
                           nactive_a=None, nactive_b=None, sums=None) -> CoActivation:
    """Torch oracle of ``coactivation`` (any device; this is what runs off the GPU): the definitions of the
    module docstring on dense [n_a, n_b] accumulators per pair of models -- ``dot`` in fp32 row by row, ``both``
    in integers, the moments in fp64 in the kernel's order.  ``sums``: the ``dense_sums_reference`` of the same
    codes, to share between calls that differ in ``m``, ``score``, ``min_both`` or ``exclude_self`` only.  There
    is no ``state=``: a pool is given whole."""
    m, score, min_both = check_m(m), check_score(score), check_min_both(min_both)
    same = sc_b is None or sc_b is sc_a
    if same:
        sc_b, nactive_b = sc_a, nactive_a
    _check_pair(sc_a, sc_b)
    fa = feature_codes_reference(sc_a, nactive_a)
    fb = fa if same else feature_codes_reference(sc_b, nactive_b)
    N, dev = sc_a.n_rows, sc_a.col.device
    Ga, Gb, n_a, n_b = fa.n_models, fb.n_models, fa.n, fb.n
    cnt_a, s1a, s2a = list_moments_reference(fa)
    cnt_b, s1b, s2b = (cnt_a, s1a, s2a) if same else list_moments_reference(fb)
    sha, sca = shift_scale(cnt_a, s1a, s2a, N, score)
    shb, scb = shift_scale(cnt_b, s1b, s2b, N, score)
    both, dot = dense_sums_reference(fa, fb) if sums is None else sums
    if score == "jaccard":
        s = both.float() / (cnt_a[:, None, :, None] + cnt_b[None, :, None, :] - both).float()
    else:
        s = ((dot - sha[:, None, :, None] * shb[None, :, None, :]) * sca[:, None, :, None]) * scb[None, :, None, :]
    s = s + 0.0                                                       # (-0.0 reads +0.0)
    cand = both >= min_both
    if same and exclude_self:
        own = torch.eye(n_a, n_b, dtype=torch.bool, device=dev)
        for g in range(Ga):
            cand[g, g] &= ~own
    shape = (Ga, Gb, n_a, m)
    partner = torch.full(shape, -1, dtype=torch.int32, device=dev)
    out_s = torch.zeros(shape, dtype=torch.float32, device=dev)
    out_b = torch.zeros(shape, dtype=torch.int32, device=dev)
    out_d = torch.zeros(shape, dtype=torch.float32, device=dev)
    for g in range(Ga):
        for h in range(Gb):
            partner[g, h], out_s[g, h], out_b[g, h], out_d[g, h] = topm_partners(s[g, h], cand[g, h], both[g, h],
                                                                                 dot[g, h], m)
    return CoActivation(partner, out_s, out_b, out_d, cnt_a, cnt_b, fa.skipped, fb.skipped, score, min_both, N)


# ---------------------------------------------------------------------- the routes
def coactivation(sc_a: SparseCodes, sc_b: Optional[SparseCodes] = None, *, m: int = 4, score: str = "pearson",
                 min_both: int = 1, exclude_self: bool = True, nactive_a=None, nactive_b=None) -> CoActivation:
    """The ``m`` (0..32) best co-activation partners of every feature of every model of ``sc_a`` among the
    features of every model of ``sc_b`` (default: ``sc_a`` itself; then ``exclude_self`` keeps a feature from
    being its own partner), by ``score`` "pearson", "cosine" or "jaccard" among the features that fire together
    on at least ``min_both`` rows (module docstring).  ``nactive_*``: live features per model of a masked
    ensemble.

    On a GPU: ``by_feature`` on both sides, ``list_moments``, the shift / scale vectors in fp64 torch ops and one
    ``sc_coactivation_topm`` launch (``csrc/coactivation.hip``) -- one walk per (source feature, target model)
    over the source list, no [n_a, n_b] matrix; nothing synchronises.  Elsewhere ``coactivation_reference``.
    There is no ``state=``: the m best of a sum cannot be merged across chunks of rows, so a pool is given
    whole."""
    if not sc_a.col.is_cuda:
        return coactivation_reference(sc_a, sc_b, m=m, score=score, min_both=min_both, exclude_self=exclude_self,
                                      nactive_a=nactive_a, nactive_b=nactive_b)
    from ..ops import coactivation as co_ops
    from .interference import live_counts

    m, score, min_both = check_m(m), check_score(score), check_min_both(min_both)
    same = sc_b is None or sc_b is sc_a
    if same:
        sc_b, nactive_b = sc_a, nactive_a
    _check_pair(sc_a, sc_b)
    fa = by_feature(sc_a, nactive_a)
    fb = fa if same else by_feature(sc_b, nactive_b)
    N = sc_a.n_rows
    cnt_a, s1a, s2a = co_ops.list_moments(fa.col_ptr, fa.row, fa.val)
    cnt_b, s1b, s2b = (cnt_a, s1a, s2a) if same else co_ops.list_moments(fb.col_ptr, fb.row, fb.val)
    sha, sca = shift_scale(cnt_a, s1a, s2a, N, score)
    shb, scb = (sha, sca) if same else shift_scale(cnt_b, s1b, s2b, N, score)
    live_b = live_counts(nactive_b, sc_b.n_models, sc_b.n, sc_b.col.device)
    out = co_ops.coactivation_topm(fa.col_ptr, fa.row, fa.val, sc_b.row_ptr.contiguous(), sc_b.col, sc_b.val, sc_b.n,
                                   sha, sca, cnt_a, shb, scb, cnt_b, m, score, min_both, bool(exclude_self and same),
                                   live_b)
    return CoActivation(*out, cnt_a, cnt_b, fa.skipped, fb.skipped, score, min_both, N)
