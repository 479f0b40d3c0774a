"""Per-feature ablation effect and shrinkage of an ensemble from its sparse codes: the result type, the fp64
torch oracles and the device route.

Every other per-feature analysis on ``SparseCodes`` says what a feature fires on; this one says what it does
for the reconstruction.  Per model g and row: ``x`` is the row as the decoder sees it (bf16 on the device route),
the row's CSR entries are ``(col_e, c_e)`` with ``c_e > 0`` in ascending column order, ``D[g]`` is the unit-norm
dictionary (the bf16 shadow on the device route; ``d % 64 == 0``, ``64 <= d <= 1024``, anything else raises
``ValueError``).  With ``r = x - sum_e c_e D[g, col_e]``, ``p_e = <r, D[g, col_e]>`` and ``q_f = |D[g, f]|^2``:

- removing entry e from its row changes the row's squared error by ``delta_e = 2 c_e p_e + c_e^2 q_f``;
- scaling every code of feature f by ``1 + alpha`` changes the SSE by ``-2 alpha A_f + alpha^2 q_f C2_f`` with
  ``A_f = sum c_e p_e`` and ``C2_f = sum c_e^2``: the least-squares rescale is ``1 + A_f / (q_f C2_f)`` and
  removes ``A_f^2 / (q_f C2_f)`` of the SSE (L1-trained SAEs shrink their codes: rescale > 1).

**Residual.**  ``r`` starts at ``x``; every entry is subtracted in CSR order with one ``fma(-c_e, D[g, col_e, k],
r_k)`` per element in fp32 -- the order of ``recon_split``'s full residual.  ``sse_row`` is ``|r|^2`` in fp32, per
lane ``s = fma(r_i, r_i, s)`` over the lane's elements ascending, then the xor butterfly 1, 2, 4, 8, 16, 32 over
the 64 lanes: bit-equal to column 0 of ``recon_split``.  Lane l holds ``P = d / 64`` elements in pieces of
``V`` = 8, 4, 2 or 1 (the largest that divides P): element ``i = p V + j`` is ``k = 64 V p + V l + j``.

**Projection.**  ``p_e``: per lane ``s = fma(r_i, a_i, s)`` over i ascending from 0, then the same butterfly;
fp32, stored at the entry's position in ``proj`` [G, cap], aligned with ``col`` / ``val``.

**Per-feature raw sums** over the feature's list of the ``FeatureCodes`` of the same codes (rows ascending), in
``list_moments``' order -- entry i goes to lane ``i % 64``, a lane adds its entries ascending from 0.0, then the
xor butterfly: ``cnt`` int64; ``A = sum double(c) double(p)``, ``P1 = sum double(p)``, ``C2 = sum double(c)^2`` in
fp64 (the products are exact); ``n_harm`` int64, the entries with ``2 double(p) + double(c) double(q_f) < 0`` (the
product is exact, the sum rounded once: the sign of ``delta_e``); ``min_delta`` / ``max_delta`` fp32, that fp64
value rounded to fp32 (``delta_e / c_e``), 0.0 for an empty list.  ``q`` fp32 [G, n] is ``ops.interference.
row_norm2``.

**Views** are fp64 torch operations on the raw sums, 0 where undefined: ``delta_sse = 2 A + q C2``, ``delta_fvu``,
``rescale``, ``rescale_gain``, ``harmful_fraction``, ``mean_proj``, ``top_mask(k)``.

**Skip rule.**  That of ``recon_split``: a row with bad pointers, more than n entries or a column outside
``[0, lim)`` (lim = n or ``min(n, nactive[g])``) is left out whole, counted in ``skipped[g]``, and stores nothing
into ``proj``.  In the list walk an entry whose row lies outside the codes' rows, or whose CSR entry cannot be
found, is left out and counted in ``missing[g]``.  ``check()`` raises if either count is non-zero.

**Chunking.**  ``state=`` / ``merge(a, b)`` add the raw sums: ``a + b`` in fp64 for the sums, integer adds for
the counts, min / max for the extrema.  Integer outputs and extrema do not depend on how a pool is cut.  The fp64
sums of a chunked pool are bit-equal to ``merge`` of the separate calls; they are NOT required to equal one call
over the whole pool, because the lane an entry is added in depends on its position in the feature's list.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, NamedTuple, Optional

import torch

from . import sparse_recon as sr
from .feature_codes import FeatureCodes, by_feature, feature_codes_reference
from .interference import live_counts
from .sparse_codes import SparseCodes

U32 = 2.0 ** -24   # unit roundoff of fp32


class AttributionSkipped(RuntimeError):
    """Rows or entries were left out of an ``Attribution``."""


def _ratio(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    ok = den != 0
    return torch.where(ok, num / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(num))


@dataclass
class Attribution:
    """Raw attribution sums of every feature of G models over ``n_rows`` rows (module docstring)."""

    n_rows: int
    cnt: torch.Tensor          # int64 [G, n]  entries of the feature
    A: torch.Tensor            # fp64 [G, n]   sum c_e p_e
    P1: torch.Tensor           # fp64 [G, n]   sum p_e
    C2: torch.Tensor           # fp64 [G, n]   sum c_e^2
    n_harm: torch.Tensor       # int64 [G, n]  entries whose removal lowers their row's error
    min_delta: torch.Tensor    # fp32 [G, n]   min of 2 p_e + c_e q_f (0.0: empty)
    max_delta: torch.Tensor    # fp32 [G, n]   max of it
    q: torch.Tensor            # fp32 [G, n]   squared atom norms
    sse_full: torch.Tensor     # fp64 [G]      sum of sse_row
    s1: torch.Tensor           # fp64 [G, d]   sum of the rows
    s2: torch.Tensor           # fp64 [G]      sum of their squares
    skipped: torch.Tensor      # int64 [G]     rows left out by the skip rule
    missing: torch.Tensor      # int64 [G]     list entries left out
    live: Optional[torch.Tensor] = None   # int32 [G] features per model of a masked ensemble
    proj: Optional[torch.Tensor] = None   # fp32 [G, cap] per-entry projections of the LAST call, when asked for

    _TENSORS = ("cnt", "A", "P1", "C2", "n_harm", "min_delta", "max_delta", "q", "sse_full", "s1", "s2", "skipped",
                "missing")

    # ------------------------------------------------------------------ views
    @property
    def variance(self) -> torch.Tensor:
        """fp64 [G]: total sum of squares about the mean of the rows (``ReconProfile.variance``)."""
        return self.s2 - self.s1.pow(2).sum(-1) / max(self.n_rows, 1)

    @property
    def _qc2(self) -> torch.Tensor:
        return self.q.double() * self.C2

    @property
    def delta_sse(self) -> torch.Tensor:
        """fp64 [G, n]: rise of the summed squared error when the feature is removed."""
        return 2.0 * self.A + self._qc2

    @property
    def delta_fvu(self) -> torch.Tensor:
        return _ratio(self.delta_sse, self.variance.unsqueeze(-1).expand_as(self.A))

    @property
    def fvu_full(self) -> torch.Tensor:
        return _ratio(self.sse_full, self.variance)

    @property
    def rescale(self) -> torch.Tensor:
        """fp64 [G, n]: the least-squares factor on the feature's codes (0 for a feature without entries)."""
        den = self._qc2
        return torch.where(den != 0, 1.0 + _ratio(self.A, den), torch.zeros_like(den))

    @property
    def rescale_gain(self) -> torch.Tensor:
        """fp64 [G, n]: the SSE that factor removes."""
        return _ratio(self.A * self.A, self._qc2)

    @property
    def harmful_fraction(self) -> torch.Tensor:
        return _ratio(self.n_harm.double(), self.cnt.double())

    @property
    def mean_proj(self) -> torch.Tensor:
        return _ratio(self.P1, self.cnt.double())

    def top_mask(self, k: int) -> torch.Tensor:
        """bool [G, n]: the k features of every model with the largest ``delta_sse``, ties to the lower index, only
        below ``live[g]``; goes straight into ``recon_profile(keep=)``."""
        return sr.top_features(self.delta_sse, k, self.live)

    # ------------------------------------------------------------------ checks and merging
    def check(self) -> "Attribution":
        """Synchronises; raises ``AttributionSkipped`` if any row or list entry was left out."""
        sk, ms = self.skipped.cpu(), self.missing.cpu()
        if bool((sk != 0).any()) or bool((ms != 0).any()):
            raise AttributionSkipped(f"{sk.tolist()} rows per model were skipped (of {self.n_rows}) and "
                                     f"{ms.tolist()} list entries were not found: encode with a larger budget, or "
                                     "budget=None, and transpose the same codes")
        return self

    def merge(self, other: "Attribution") -> "Attribution":
        """The raw sums over the rows of both (same ensemble, same dictionaries): ``self + other`` in fp64, integer
        adds, min / max of the extrema over the non-empty sides."""
        check_state(other, self.A.shape[0], self.A.shape[1], self.s1.shape[1])
        dev = self.A.device
        o = other.to(dev)
        ea, eb = self.cnt == 0, o.cnt == 0
        ext = lambda a, b, f: torch.where(ea, b, torch.where(eb, a, f(a, b)))
        return Attribution(self.n_rows + o.n_rows, self.cnt + o.cnt, self.A + o.A, self.P1 + o.P1, self.C2 + o.C2,
                           self.n_harm + o.n_harm, ext(self.min_delta, o.min_delta, torch.minimum),
                           ext(self.max_delta, o.max_delta, torch.maximum), self.q, self.sse_full + o.sse_full,
                           self.s1 + o.s1, self.s2 + o.s2, self.skipped + o.skipped, self.missing + o.missing,
                           self.live, o.proj)

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        sd = {k: getattr(self, k) for k in self._TENSORS}
        sd["n_rows"] = torch.tensor(int(self.n_rows), dtype=torch.int64)
        for k in ("live", "proj"):
            if getattr(self, k) is not None:
                sd[k] = getattr(self, k)
        return sd

    def save(self, path):
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, map_location="cpu") -> "Attribution":
        sd = torch.load(path, map_location=map_location, weights_only=True)
        return cls(int(sd["n_rows"]), *(sd[k] for k in cls._TENSORS), sd.get("live"), sd.get("proj"))

    def to(self, device) -> "Attribution":
        mv = lambda t: None if t is None else t.to(device)
        return Attribution(self.n_rows, *(getattr(self, k).to(device) for k in self._TENSORS), mv(self.live),
                           mv(self.proj))


def check_state(state, G: int, n: int, d: Optional[int] = None):
    """Validate the ``state`` argument of an ``attribution`` call (the result of an earlier call)."""
    if not isinstance(state, Attribution):
        raise ValueError("state must be the Attribution of an earlier call")
    if tuple(state.A.shape) != (G, n) or (d is not None and tuple(state.s1.shape) != (G, d)):
        raise ValueError(f"state is for another ensemble (A {tuple(state.A.shape)}, this one [{G}, {n}])")


def _check_dims(sc: SparseCodes, D: torch.Tensor):
    G, n = sc.n_models, sc.n
    if D.dim() != 3 or D.shape[0] != G or D.shape[1] != n:
        raise ValueError(f"D must be [{G}, {n}, d], got {tuple(D.shape)}")
    d = D.shape[2]
    if d < 64 or d > 1024 or d % 64:
        raise ValueError(f"attribution needs d % 64 == 0 and 64 <= d <= 1024 (got d={d})")
    return G, n, d


# ---------------------------------------------------------------------- the fp64 oracles
def lane_elements(d: int) -> torch.Tensor:
    """int64 [64, P]: ``k`` of element i of lane l in the kernels' layout (module docstring)."""
    P = d // 64
    V = 8 if P % 8 == 0 else 4 if P % 4 == 0 else 2 if P % 2 == 0 else 1
    i = torch.arange(P)
    return 64 * V * (i // V).view(1, P) + V * torch.arange(64).view(64, 1) + (i % V).view(1, P)


def _fma32(a: torch.Tensor, b: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """``fma(a, b, s)`` of fp32 values held in fp64 tensors: the product is exact in fp64, the sum is rounded to
    fp64 and then to fp32 (equal to the fused fp32 result except for rare double roundings)."""
    return (a * b + s).float().double()


def _butterfly(s: torch.Tensor) -> torch.Tensor:
    """The xor butterfly 1, 2, 4, 8, 16, 32 over the last dimension (64 lanes), in the tensor's own precision."""
    lanes = torch.arange(64, device=s.device)
    for o in (1, 2, 4, 8, 16, 32):
        s = s + s[..., lanes ^ o]
    return s[..., 0]


def row_norm2_reference(D: torch.Tensor) -> torch.Tensor:
    """fp32 [G, n]: torch oracle of ``ops.interference.row_norm2`` in the kernel's order -- 16 lanes per atom,
    lane q adds the squares of the elements ``128 t + 8 q + j`` (t, then j = 0..7 ascending) with one fma each,
    then the xor butterfly 1, 2, 4, 8.  Squares of bf16 values are exact in fp32, so every step is a plain fp32
    add; for fp32 dictionaries the squares are rounded first (then this is the oracle's own definition)."""
    G, n, d = D.shape
    pad = -d % 128
    Df = torch.nn.functional.pad(D.float(), (0, pad)).view(G, n, -1, 16, 8)
    s = torch.zeros(G, n, 16, dtype=torch.float32, device=D.device)
    for t in range(Df.shape[2]):
        for j in range(8):
            s = _fma32(Df[:, :, t, :, j].double(), Df[:, :, t, :, j].double(), s.double()).float()
    lanes = torch.arange(16, device=D.device)
    for o in (1, 2, 4, 8):
        s = s + s[..., lanes ^ o]
    return s[..., 0].contiguous()


class ResidualProj(NamedTuple):
    """What ``residual_proj_reference`` returns.  ``proj`` / ``sse_row`` follow the fp32 order of the kernel;
    ``proj64`` is the exact value from fp64 arithmetic and ``bound`` the forward error bound of the fp32 order,
    ``gamma_L sum_k |a_k| m_k + gamma_{P + 6} sum_k |r_k| |a_k|`` with ``m_k = |x_k| + sum_e |c_e a_ek|``,
    ``gamma_j = j u / (1 - j u)``, ``u = 2^-24``, L the row's entries and P = d / 64."""

    proj: torch.Tensor      # fp32 [G, cap]
    sse_row: torch.Tensor   # fp32 [G, n_rows]
    skipped: torch.Tensor   # int64 [G]
    proj64: torch.Tensor    # fp64 [G, cap]
    bound: torch.Tensor     # fp64 [G, cap]
    sse64: torch.Tensor     # fp64 [G, n_rows]
    valid: torch.Tensor     # bool [G, n_rows]  rows that passed the skip rule


def _gamma(j):
    return j * U32 / (1.0 - j * U32)


def residual_proj_reference(sparse_codes: SparseCodes, D: torch.Tensor, x: torch.Tensor, nactive=None,
                            row0: int = 0, n_rows: Optional[int] = None) -> ResidualProj:
    """Torch oracle of ``ops.attribution.residual_proj`` (any device) on the rows ``row0 .. row0 + n_rows - 1``
    (default: all) of ``sparse_codes`` against ``D`` [G, n, d] and the window's rows ``x`` ([n_rows, d] shared or
    [G, n_rows, d]), values read as they are in fp32.  Positions of ``proj`` outside the window's valid rows stay
    0."""
    sc = sparse_codes
    G, n, d = _check_dims(sc, D)
    cap = sc.cap
    n_rows = sc.n_rows - row0 if n_rows is None else int(n_rows)
    if row0 < 0 or n_rows < 0 or row0 + n_rows > sc.n_rows:
        raise ValueError(f"rows [{row0}, {row0 + n_rows}) outside [0, {sc.n_rows}]")
    if x.dim() not in (2, 3) or x.shape[-1] != d or x.shape[-2] != n_rows or (x.dim() == 3 and x.shape[0] != G):
        raise ValueError(f"x must be [{n_rows}, {d}] or [{G}, {n_rows}, {d}], got {tuple(x.shape)}")
    dev = D.device
    P = d // 64
    kidx = lane_elements(d).to(dev)
    Dd, xd = D.float().double(), x.to(dev).float().double()
    live = live_counts(nactive, G, n, dev)
    lim = [n] * G if live is None else live.tolist()
    f64 = dict(dtype=torch.float64, device=dev)
    proj = torch.zeros(G, cap, dtype=torch.float32, device=dev)
    sse_row = torch.zeros(G, n_rows, dtype=torch.float32, device=dev)
    proj64, bound, sse64 = torch.zeros(G, cap, **f64), torch.zeros(G, cap, **f64), torch.zeros(G, n_rows, **f64)
    valid = torch.zeros(G, n_rows, dtype=torch.bool, device=dev)
    rp = sc.row_ptr.to(dev)
    for g in range(G):
        colg, valg = sc.col[g].to(dev).long(), sc.val[g].to(dev).double()
        lo, hi = rp[g, row0:row0 + n_rows], rp[g, row0 + 1:row0 + n_rows + 1]
        ok = (lo >= 0) & (hi >= lo) & (hi <= cap) & (hi - lo <= n)
        L = torch.where(ok, hi - lo, torch.zeros_like(lo))
        T = int(L.max()) if n_rows else 0
        t = torch.arange(T, device=dev)
        has = t < L.unsqueeze(1)                                   # [rows, T]: entry t of the row exists
        at_e = (torch.where(ok, lo, torch.zeros_like(lo)).unsqueeze(1) + t).clamp(max=max(cap - 1, 0))
        cols = colg[at_e] if cap else at_e
        ok &= ~(has & ((cols < 0) | (cols >= lim[g]))).any(1)     # one bad column condemns the whole row
        valid[g] = ok
        has &= ok.unsqueeze(1)
        cols = torch.where(has, cols, torch.zeros_like(cols))
        c = torch.where(has, valg[at_e] if cap else at_e.double(), torch.zeros((), **f64))
        xg = xd[g] if xd.dim() == 3 else xd
        res = xg                                                   # [rows, d]: the fp32 residual, held in fp64
        for e in range(T):
            res = torch.where(has[:, e, None], _fma32(-c[:, e, None], Dd[g, cols[:, e]], res), res)
        rl = res[:, kidx]                                          # [rows, 64, P]
        s = torch.zeros(n_rows, 64, **f64)
        for i in range(P):
            s = _fma32(rl[..., i], rl[..., i], s)
        sse_row[g] = torch.where(ok, _butterfly(s.float()), torch.zeros((), device=dev))
        pj = torch.zeros(n_rows, T, dtype=torch.float32, device=dev)
        for e in range(T):
            al = Dd[g, cols[:, e]][:, kidx]                        # [rows, 64, P]
            s = torch.zeros(n_rows, 64, **f64)
            for i in range(P):
                s = _fma32(rl[..., i], al[..., i], s)
            pj[:, e] = _butterfly(s.float())
        # the exact values and the bound, from dense fp64 products
        rows_of = torch.arange(n_rows, device=dev).unsqueeze(1).expand_as(cols)
        dense = torch.zeros(n_rows, n, **f64).index_put_((rows_of[has], cols[has]), c[has], accumulate=True)
        r64 = xg - dense @ Dd[g]
        m = xg.abs() + dense @ Dd[g].abs()
        sse64[g] = torch.where(ok, (r64 * r64).sum(1), torch.zeros((), **f64))
        p64 = (r64 @ Dd[g].T).gather(1, cols)
        bnd = _gamma(L.double()).unsqueeze(1) * (m @ Dd[g].abs().T).gather(1, cols) \
            + _gamma(P + 6) * (r64.abs() @ Dd[g].abs().T).gather(1, cols)
        proj[g, at_e[has]] = pj[has]
        proj64[g, at_e[has]] = p64[has]
        bound[g, at_e[has]] = bnd[has]
    return ResidualProj(proj, sse_row, (~valid).sum(1), proj64, bound, sse64, valid)


def attr_list_sums_reference(fc: FeatureCodes, sparse_codes: SparseCodes, proj: torch.Tensor, q: torch.Tensor):
    """Torch oracle of ``ops.attribution.attr_list_sums`` (any device): ``(cnt, A, P1, C2, n_harm, min_delta,
    max_delta, missing)`` in the kernel's order, the way ``list_moments_reference`` emulates it: list bounds
    clipped as the kernel clips them, the same binary search for the entry's CSR position, entry i in lane
    ``i % 64``, lanes added ascending from 0.0 and joined by the xor butterfly."""
    sc = sparse_codes
    G, n, N, cap, fcap, dev = fc.n_models, fc.n, sc.n_rows, sc.cap, fc.cap, fc.row.device
    if sc.n_models != G or sc.n != n or tuple(proj.shape) != (G, cap) or tuple(q.shape) != (G, n):
        raise ValueError("feature codes, sparse codes, proj [G, cap] and q [G, n] must belong together")
    lo_all = fc.col_ptr[:, :-1].clamp(min=0, max=fcap)
    hi_all = torch.maximum(fc.col_ptr[:, 1:], lo_all).clamp(max=fcap)
    cntl = hi_all - lo_all
    chunks = max(1, -(-int(cntl.max()) // 64)) if cntl.numel() else 1
    pos = torch.arange(chunks * 64, device=dev)
    feat = torch.arange(n, device=dev).unsqueeze(1)
    i64 = dict(dtype=torch.int64, device=dev)
    outs = [torch.zeros(G, n, **i64)] + [torch.zeros(G, n, 64, dtype=torch.float64, device=dev) for _ in range(3)] \
        + [torch.zeros(G, n, **i64), torch.zeros(G, n, device=dev), torch.zeros(G, n, device=dev)]
    cnt, A, P1, C2, n_harm, mn, mx = outs
    missing = torch.zeros(G, **i64)
    rp, colg_all, pj_all = sc.row_ptr.to(dev), sc.col.to(dev).long(), proj.to(dev)
    for g in range(G):
        live = pos < cntl[g, :, None]                                         # [n, chunks * 64]
        found = torch.zeros_like(live)
        c = torch.zeros(n, chunks * 64, dtype=torch.float64, device=dev)
        p = torch.zeros_like(c)
        if fcap and N and cap:
            at = (lo_all[g, :, None] + pos).clamp(max=fcap - 1)
            r = fc.row[g][at].long()
            c = torch.where(live, fc.val[g][at].double(), c)
            ok = live & (r >= 0) & (r < N)
            rs = r.clamp(0, N - 1)
            s, e = rp[g][rs], rp[g][rs + 1]
            ok &= (s >= 0) & (e >= s) & (e <= cap)
            zero = torch.zeros_like(s)
            lb, ub, e = torch.where(ok, s, zero), torch.where(ok, e, zero), torch.where(ok, e, zero)
            while bool((lb < ub).any()):                                      # the kernel's lower bound search
                act, mid = lb < ub, (lb + ub) >> 1
                less = colg_all[g][mid.clamp(0, cap - 1)] < feat
                lb, ub = torch.where(act & less, mid + 1, lb), torch.where(act & ~less, mid, ub)
            at_e = lb.clamp(0, cap - 1)
            found = ok & (lb < e) & (colg_all[g][at_e] == feat)
            p = torch.where(found, pj_all[g][at_e].double(), p)
        z = torch.zeros_like(c)
        qf = q[g].to(dev).double().unsqueeze(1)
        delta = 2.0 * p + c * qf                                              # (c qf is exact: one rounding)
        ta, tp, tc = (torch.where(found, t, z).view(n, chunks, 64) for t in (c * p, p, c * c))
        for k in range(chunks):                                               # (adding 0.0 changes nothing)
            A[g] = A[g] + ta[:, k]
            P1[g] = P1[g] + tp[:, k]
            C2[g] = C2[g] + tc[:, k]
        cnt[g] = found.sum(1)
        n_harm[g] = (found & (delta < 0)).sum(1)
        df = delta.float()
        inf = torch.full_like(df, float("inf"))
        some = cnt[g] > 0
        mn[g] = torch.where(some, torch.where(found, df, inf).amin(1), torch.zeros_like(mn[g]))
        mx[g] = torch.where(some, torch.where(found, df, -inf).amax(1), torch.zeros_like(mx[g]))
        missing[g] = (live & ~found).sum()
    return cnt, _butterfly(A).contiguous(), _butterfly(P1).contiguous(), _butterfly(C2).contiguous(), n_harm, mn, \
        mx, missing


def attribution_reference(sparse_codes: SparseCodes, D: torch.Tensor, x: torch.Tensor, nactive=None, *,
                          feature_codes: Optional[FeatureCodes] = None, proj: Optional[torch.Tensor] = None,
                          q: Optional[torch.Tensor] = None, residual: Optional[ResidualProj] = None,
                          state: Optional[Attribution] = None, return_proj: bool = False) -> Attribution:
    """The ``Attribution`` of ``sparse_codes`` against ``D`` [G, n, d] and all its rows ``x`` from the torch oracle
    (any device, any float dtype): the fp32 order of the kernels for ``proj`` / ``sse_row`` (emulated in fp64 and
    rounded after every operation) and their lane-strided fp64 order for the per-feature sums.  ``proj`` / ``q``:
    take these per-entry projections / squared norms instead of the oracle's own (to check the list walk on the
    kernel's values); ``residual``: the ``residual_proj_reference`` of the same inputs and ``feature_codes``: the
    transposition of the same codes, if they exist already."""
    sc = sparse_codes
    G, n, d = _check_dims(sc, D)
    dev = D.device
    if state is not None:
        check_state(state, G, n, d)
    rp = residual_proj_reference(sc, D, x, nactive) if residual is None else residual
    pj = rp.proj if proj is None else proj.to(dev)
    qq = row_norm2_reference(D) if q is None else q.to(dev)
    fc = feature_codes_reference(sc.to(dev), nactive) if feature_codes is None else feature_codes.to(dev)
    cnt, A, P1, C2, n_harm, mn, mx, missing = attr_list_sums_reference(fc, sc.to(dev), pj, qq)
    s1, s2 = sr._moments(x.to(dev), G)
    out = Attribution(sc.n_rows, cnt, A, P1, C2, n_harm, mn, mx, qq, rp.sse_row.sum(1, dtype=torch.float64),
                      s1.contiguous(), s2.contiguous(), rp.skipped, missing, live_counts(nactive, G, n, dev),
                      pj if return_proj else None)
    return out if state is None else state.merge(out)


def attribution_dense_reference(sparse_codes: SparseCodes, D: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """Brute force, fp64 [G, n]: the summed squared error with column f of the dense codes zeroed minus the full
    one, for every feature -- n dense reconstructions per model.  Needs complete codes."""
    sc = sparse_codes.check()
    G, n = sc.n_models, sc.n
    Dd, xd = D.double(), x.to(D.device).double()
    out = torch.zeros(G, n, dtype=torch.float64, device=D.device)
    for g in range(G):
        C = sc.to_dense(g).to(D.device).double()
        xg = xd[g] if xd.dim() == 3 else xd
        full = (xg - C @ Dd[g]).pow(2).sum()
        for f in range(n):
            Cf = C.clone()
            Cf[:, f] = 0
            out[g, f] = (xg - Cf @ Dd[g]).pow(2).sum() - full
    return out


# ---------------------------------------------------------------------- the routes
def attribution_fused(sparse_codes: SparseCodes, shadow: torch.Tensor, batches: Iterable[torch.Tensor],
                      nactive=None, feature_codes: Optional[FeatureCodes] = None,
                      state: Optional[Attribution] = None, *, waves: int = 4,
                      return_proj: bool = False) -> Attribution:
    """The ``Attribution`` of ``sparse_codes`` against the bf16 dictionaries ``shadow`` [G, n, d] on the device.
    ``batches`` yields the rows the decoder sees, batch by batch in the order of the CSR's rows (bf16 [B, d]
    shared or [G, B, d]; a batch may be overwritten once the next is asked for): per batch one ``residual_proj``
    launch on the batch's row window and the variance bookkeeping, then ``by_feature(nactive)`` (unless
    ``feature_codes`` is given), ``row_norm2`` and one ``attr_list_sums`` launch (``csrc/attribution.hip``).
    Never synchronises."""
    from ..ops import attribution as at_ops
    from ..ops import interference as ic_ops

    sc = sparse_codes
    G, n, d = _check_dims(sc, shadow)
    dev = shadow.device
    if state is not None:
        check_state(state, G, n, d)
    live = live_counts(nactive, G, n, dev)
    f64 = dict(dtype=torch.float64, device=dev)
    proj = torch.zeros(G, sc.cap, dtype=torch.float32, device=dev)
    skipped = torch.zeros(G, dtype=torch.int64, device=dev)
    missing = torch.zeros(G, dtype=torch.int64, device=dev)
    sse, s1, s2 = torch.zeros(G, **f64), torch.zeros(G, d, **f64), torch.zeros(G, **f64)
    row_ptr = sc.row_ptr.contiguous()
    at = 0
    for x in batches:
        _, sse_row = at_ops.residual_proj(row_ptr, sc.col, sc.val, shadow, x, skipped, row0=at, nactive=live,
                                          proj=proj)
        sse += sse_row.sum(1, dtype=torch.float64)
        b1, b2 = sr._moments(x, G)
        s1 += b1
        s2 += b2
        at += x.shape[-2]
    if at != sc.n_rows:
        raise ValueError(f"the batches hold {at} rows, the sparse codes {sc.n_rows}")
    fc = by_feature(sc, nactive) if feature_codes is None else feature_codes
    q = ic_ops.row_norm2(shadow)
    sums = at_ops.attr_list_sums(fc.col_ptr, fc.row, fc.val, row_ptr, sc.col, proj, q, missing, waves=waves)
    out = Attribution(sc.n_rows, *sums, q, sse, s1, s2, skipped, missing, live, proj if return_proj else None)
    return out if state is None else state.merge(out)


def attribution(sparse_codes: SparseCodes, D: torch.Tensor, x: torch.Tensor, nactive=None,
                feature_codes: Optional[FeatureCodes] = None, *, state: Optional[Attribution] = None,
                return_proj: bool = False, **kw) -> Attribution:
    """The ``Attribution`` of ``sparse_codes`` against the unit-norm dictionaries ``D`` [G, n, d] and all its rows
    ``x`` ([n_rows, d] shared or [G, n_rows, d]) as the decoder sees them.  On a GPU: the kernels (``D`` and ``x``
    bf16; ``kw``: ``waves``); elsewhere ``attribution_reference``.  Works from saved ``SparseCodes`` without an
    engine."""
    if not sparse_codes.col.is_cuda:
        if kw:
            raise TypeError(f"attribution: {sorted(kw)} are keywords of the device route")
        return attribution_reference(sparse_codes, D, x, nactive, feature_codes=feature_codes, state=state,
                                     return_proj=return_proj)
    return attribution_fused(sparse_codes, D, [x], nactive, feature_codes, state, return_proj=return_proj, **kw)
