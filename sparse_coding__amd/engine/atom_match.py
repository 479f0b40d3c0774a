"""Nearest-atom matching across the models of an ensemble: the result type, the fp64 torch oracle and the
kernel path the fused engines share.

``FusedSAEEnsemble.atom_matches`` / ``FusedTopKEnsemble.atom_matches`` fill an ``AtomMatches`` from the bf16
shadow that holds the unit-norm dictionaries of all G models, with the row-argmax epilogue of the grouped
GEMM (``ops.gemm.rowargmax_nt``): for every ordered pair (g, h) the m nearest atoms of model h for each
atom of model g, and for g == h the nearest *other* atoms.  ``atom_matches_reference`` computes the same
object in fp64 torch (CPU included) and is what the tests compare against.  Among equal cosines the lowest
atom index wins, everywhere.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

MAX_MATCHES = 8


@dataclass
class AtomMatches:
    """The ``m`` nearest atoms of model h for every atom of model g, for all ordered pairs (g, h)."""

    cos: torch.Tensor        # fp32 [G, G, n, m]  cosines, descending; 0.0 = empty slot
    idx: torch.Tensor        # int32 [G, G, n, m] atom indices in model h; -1 = empty slot
    dict_size: torch.Tensor  # int64 [G] live atoms of each model (rows at or past it are empty)

    @property
    def m(self) -> int:
        return int(self.cos.shape[-1])

    def mmcs(self) -> torch.Tensor:
        """[G, G] fp32: entry (g, h) is the mean over model g's live atoms of the cosine to their nearest
        atom of model h (``eval.metrics.mmcs(ld[h], ld[g])``); the diagonal is 1 (a model against itself;
        the nearest *other* atoms are in ``pair(g, g)``).  A model without live atoms reads 0."""
        G, _, n, _ = self.cos.shape
        size = self.dict_size.to(self.cos.device)
        live = (torch.arange(n, device=self.cos.device).unsqueeze(0) < size.unsqueeze(1)).to(torch.float64)
        tot = (self.cos[..., 0].double() * live[:, None, :]).sum(-1)
        out = (tot / size.clamp(min=1).double()[:, None]).float()
        out[torch.arange(G), torch.arange(G)] = 1.0
        return out

    def pair(self, g: int, h: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(cos [size_g, m], idx [size_g, m]) of model g's live atoms against model h."""
        s = int(self.dict_size[g])
        return self.cos[g, h, :s], self.idx[g, h, :s]

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        return {"cos": self.cos, "idx": self.idx, "dict_size": self.dict_size}

    def save(self, path):
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, map_location="cpu") -> "AtomMatches":
        sd = torch.load(path, map_location=map_location, weights_only=True)
        return cls(cos=sd["cos"], idx=sd["idx"], dict_size=sd["dict_size"])

    def to(self, device) -> "AtomMatches":
        return AtomMatches(self.cos.to(device), self.idx.to(device), self.dict_size.to(device))


def check_m(m: int) -> int:
    m = int(m)
    if not 1 <= m <= MAX_MATCHES:
        raise ValueError(f"m must be in [1, {MAX_MATCHES}], got {m}")
    return m


def topm_reference(sim: torch.Tensor, m: int, valid: Optional[torch.Tensor] = None):
    """The ``m`` largest entries of every row of ``sim`` [..., M, N] among the ``valid`` ones, ordered by
    value descending, then column ascending (a stable sort); missing entries read (0.0, -1).
    Returns (values in ``sim``'s dtype, int32 columns)."""
    s = sim if valid is None else torch.where(valid, sim, torch.full_like(sim, float("-inf")))
    vals, cols = torch.sort(s, dim=-1, descending=True, stable=True)
    vals, cols = vals[..., :m], cols[..., :m]
    if vals.shape[-1] < m:  # fewer columns than passes
        pad = m - vals.shape[-1]
        vals = torch.cat([vals, vals.new_full((*vals.shape[:-1], pad), float("-inf"))], -1)
        cols = torch.cat([cols, cols.new_zeros((*cols.shape[:-1], pad))], -1)
    none = torch.isinf(vals) & (vals < 0)
    return (torch.where(none, torch.zeros_like(vals), vals),
            torch.where(none, torch.full_like(cols, -1), cols).to(torch.int32))


def atom_matches_reference(dicts, dict_size: Optional[Sequence[int]] = None, m: int = 1,
                           exclude_self: bool = True) -> AtomMatches:
    """fp64 torch oracle: the ``AtomMatches`` of the stacked unit-norm dictionaries ``dicts`` [G, n, d]
    (any float dtype; the products are taken in fp64 of the values as given).  ``dict_size``: live atoms
    per model (default all n) -- rows past it read (0.0, -1) and columns past it are never named.
    ``exclude_self``: for g == h an atom is not its own match."""
    m = check_m(m)
    D = torch.stack(list(dicts)) if not torch.is_tensor(dicts) else dicts
    if D.dim() != 3:
        raise ValueError(f"dicts must be [G, n, d], got {tuple(D.shape)}")
    G, n, _ = D.shape
    dev = D.device
    size = torch.full((G,), n, dtype=torch.int64) if dict_size is None \
        else torch.as_tensor(dict_size).to(torch.int64).reshape(-1).cpu()
    if size.numel() != G or int(size.min()) < 0 or int(size.max()) > n:
        raise ValueError(f"dict_size must hold {G} values in [0, {n}]")
    Dd = D.double()
    ar = torch.arange(n, device=dev)
    cos = torch.zeros(G, G, n, m, dtype=torch.float32, device=dev)
    idx = torch.full((G, G, n, m), -1, dtype=torch.int32, device=dev)
    for g in range(G):
        row_live = (ar < int(size[g])).unsqueeze(1)
        for h in range(G):
            valid = row_live & (ar < int(size[h])).unsqueeze(0)
            if g == h and exclude_self:
                valid = valid & (ar.unsqueeze(0) != ar.unsqueeze(1))
            v, c = topm_reference(Dd[g] @ Dd[h].T, m, valid)
            cos[g, h], idx[g, h] = v.float(), c
    return AtomMatches(cos, idx, size)


def atom_matches_fused(shadow: torch.Tensor, dict_size: Optional[torch.Tensor], m: int = 1) -> AtomMatches:
    """The kernel path of the fused engines: ``shadow`` is the contiguous bf16 [G, n, d] tensor holding
    the unit-norm dictionaries (read in place, never copied), ``dict_size`` the engine's int32 [G] device
    tensor of live sizes or None.  G launches of G problems each per pass: A is every model (group stride
    n d), B model h (group stride 0); the problem g == h excludes each atom's own index.  No host
    synchronisation."""
    from ..ops import gemm

    m = check_m(m)
    G, n, d = shadow.shape
    dev = shadow.device
    cos = torch.empty(G, G, n, m, device=dev, dtype=torch.float32)
    idx = torch.empty(G, G, n, m, device=dev, dtype=torch.int32)
    own = torch.arange(n, device=dev, dtype=torch.int32)
    for h in range(G):
        excl = torch.full((G, n, 1), -1, device=dev, dtype=torch.int32)
        excl[h, :, 0] = own
        live_cols = None if dict_size is None else dict_size[h].expand(G)
        gemm.rowargmax_nt(shadow, shadow[h], m=m, exclude=excl, live_cols=live_cols, live_rows=dict_size,
                          out=(cos[:, h], idx[:, h]))
    size = torch.full((G,), n, dtype=torch.int64, device=dev) if dict_size is None else dict_size.to(torch.int64)
    return AtomMatches(cos, idx, size)
