"""Whole-dictionary ridge probes from sparse codes: is a concept linearly readable from the code as a whole, and
which features carry it?  The result type, the solver, the torch oracles and the device route.

``ridge_probes`` fits, for every model of an ensemble and up to 32 concepts at once, exactly
``sklearn.linear_model.RidgeClassifier(alpha)`` on the model's codes: targets ``y = +-1`` from bit k of the flag
words, an unpenalised intercept through centring, ``min |Xc w - yc|^2 + alpha |w|^2``.  It is the ensemble form of
the reference's ``ridge_regression_auroc`` and the whole-dictionary counterpart of ``feature_auroc``.

- **Centring never densifies anything**: with mu the feature means over the fit rows, ``Xc v = C v - (mu . v) 1``
  (the shift of ``ops.probe.rows_matmul``) and ``Xc^T u = C^T u - mu (sum u)``.
- **Solver**: CGLS on the regularised normal equations, all G models and K concepts in lockstep.  Per (g, k)::

      w = 0; r = yc; s = Xc^T r - alpha w; p = s; gamma = gamma0 = |s|^2; live = gamma0 > 0
      repeat max_iter times:
          live &= gamma > tol^2 gamma0
          q = Xc p;  delta = |q|^2 + alpha |p|^2;  a = (live and delta > 0) ? gamma / delta : 0
          w += a p;  r -= a q;  s = Xc^T r - alpha w;  gamma' = |s|^2
          b = live ? gamma' / gamma : 0;  p = live ? s + b p : p;  gamma = live ? gamma' : gamma;  iters += live
      converged = gamma <= tol^2 gamma0

  A finished concept is frozen: fp32 CGLS run past its convergence diverges, and with the freeze the result is the
  same for every ``max_iter`` past the stop.  On the device the iterates are fp32 and every sum and scalar is fp64
  (``ops.probe``); nothing in the loop reads a value to the host.
- **Rows**: ``fit_rows`` (bool [N], default all) selects the rows the fit sees -- means, targets and residuals use
  those rows only; the others are held out and only scored.  Every row must pass the skip rule of
  ``ops.probe.rows_matmul`` (``FeatureCodesSkipped`` otherwise: a fit that silently lost rows answers another
  question); ``LinearProbes.scores`` on other codes gives a row that fails it the score 0.
- **AUROC**: the scores ``C w + b`` of every row, ranked exactly with integer arithmetic (``score_auroc``: ties are
  equal fp32 values and count half), separately over the fit rows and the held-out rows.

``logistic_probes`` fits, on the same codes, rows and concepts, exactly ``sklearn.linear_model.LogisticRegression(C)``:
``min sum_fit l(z_i, t_i) + |w|^2 / 2C`` with ``z = Xc w + b'``, targets ``t`` in {0, 1}, ``l(z, t) = softplus(z) -
t z`` and the stable ``softplus(z) = max(z, 0) + log1p(exp(-|z|))``; the intercept is unpenalised and reported as
``b' - mu . w`` in fp64.  It is the ensemble form of the reference's ``logistic_regression_auroc``.

- **Solver**: truncated Newton-CG in the centred parametrisation, all G models and K concepts in lockstep, written
  once (``_newton_cg``) for the kernel operator and a dense one.  Vectors are pairs (weights, intercept); per (g, k)::

      w = 0; b' = log(pos / neg); p = sigma(z); r = p - t, D = p (1 - p) on the fit rows, 0 elsewhere
      g = (Xc^T r + w / C, sum r); g0 = g; f = sum_fit l + |w|^2 / 2C; live = |g0| > 0
      repeat max_iter times:
          live &= |g| > tol |g0|;  iters += live                 (early_stop: leave when no (g, k) is live)
          d = 0; res = p = live ? -g : 0; rho = |res|^2; eta = min(0.5, sqrt(|g| / |g0|)); cgl = live
          repeat cg_iter times:                                  CG on H d = -g
              cgl &= rho > eta^2 |g|^2
              q = D o (Xc p_w + p_b);  h = (Xc^T q + p_w / C, sum q);  a = (cgl and p.h > 0) ? rho / p.h : 0
              d += a p;  res -= a h;  rho' = |res|^2;  beta = cgl ? rho' / rho : 0
              p = cgl ? res + beta p : p;  rho = cgl ? rho' : rho;  cg_iters += cgl
          u = Xc d_w + d_b;  f_j = sum_fit l(z + 2^-j u) + |w + 2^-j d_w|^2 / 2C,  j = 0 .. 7, from one pass
          s = the largest 2^-j with f_j <= f + 1e-4 2^-j g.d;  none: s = 0, stalled, live = false
          w += s d_w;  b' += s d_b;  z, r, D, f, g afresh
      converged = |g| <= tol |g0|

  A finished (or stalled) concept is frozen -- its step is 0 -- so the result is the same for every ``max_iter``
  past its stop, and the same with and without ``early_stop``, which reads one bool per outer step to the host.
- **Constant concepts** (no positive or no negative among the fit rows): the maximiser is at infinity; the probes
  report weight 0 and the intercept ``+-log(2 n_fit)``, the logit at which the absent class has probability
  ``1 / (2 n_fit + 1)`` -- less than half a row's worth over the fit rows -- ``converged``, and NaN AUROC.
- **AUROC**: of the logits; sigma is monotone, so it is the reference's ``roc_auc_score(y, predict_proba[:, 1])``
  without the ties that fp32 probabilities saturate into.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from ..ops.probe import CONCEPTS   # (plain Python: no kernel library is loaded)
from .feature_codes import FeatureCodesSkipped
from .interference import live_counts
from .sparse_codes import SparseCodes
from .value_order import check_flags, float_keys

MIN_TOL = 1e-6     # fp32 iterates cannot promise less


def concept_bits(flags: torch.Tensor, n_concepts: int) -> torch.Tensor:
    """bool [N, K]: bit k of every flag word."""
    return ((flags.to(torch.int64).unsqueeze(1) >> torch.arange(n_concepts, device=flags.device)) & 1).bool()


def check_fit_rows(fit_rows, n_rows: int, device) -> torch.Tensor:
    if fit_rows is None:
        return torch.ones(n_rows, dtype=torch.bool, device=device)
    if not isinstance(fit_rows, torch.Tensor) or fit_rows.dtype != torch.bool or tuple(fit_rows.shape) != (n_rows,):
        raise ValueError(f"fit_rows must be a bool tensor [{n_rows}]")
    return fit_rows.to(device)


def check_solver(alpha, max_iter, tol, min_tol: float = MIN_TOL):
    alpha = float(alpha)
    if not alpha >= 0.0 or alpha == float("inf"):
        raise ValueError(f"alpha must be a finite number >= 0, got {alpha!r}")
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or int(max_iter) < 0:
        raise ValueError(f"max_iter must be a non-negative integer, got {max_iter!r}")
    tol = float(tol)
    if not tol >= min_tol or not tol < 1.0:
        raise ValueError(f"tol must lie in [{min_tol:g}, 1): fp32 iterates cannot promise less (got {tol!r})")
    return alpha, int(max_iter), tol


# ---------------------------------------------------------------------- exact AUROC of score columns
def score_auroc(scores: torch.Tensor, bits: torch.Tensor, rows: torch.Tensor):
    """The exact rank sums of the score columns ``scores`` fp32 [G, N, K] against ``bits`` bool [N, K] over the rows
    ``rows`` bool [N]: ``(u2 int64 [G, K], pos int64 [K], cnt int64 [], tp int64 [G, K], tn int64 [G, K])`` --
    ``u2`` sums over the positive rows ``2 #{negative rows with a smaller score} + #{negative rows with an equal
    score}``, ``pos`` counts the positives and ``cnt`` the rows, ``tp`` / ``tn`` count the positives with ``score >
    0`` and the negatives without.  One sort of the ``float_keys`` per model, integer sums: torch on any device,
    nothing synchronises."""
    G, N, K = scores.shape
    dev = scores.device
    pos_rows = bits & rows.unsqueeze(1)                              # [N, K]
    neg_rows = ~bits & rows.unsqueeze(1)
    u2 = torch.zeros(G, K, dtype=torch.int64, device=dev)
    tp, tn = torch.zeros_like(u2), torch.zeros_like(u2)
    for g in range(G):
        sc = scores[g].float() + 0.0                                 # (-0.0 becomes +0.0: equal values, equal keys)
        keys, order = torch.sort(float_keys(sc.t().contiguous()), dim=1)
        start = torch.searchsorted(keys, keys, right=False)
        end = torch.searchsorted(keys, keys, right=True)
        cn = torch.zeros(K, N + 1, dtype=torch.int64, device=dev)    # negatives before every sorted position
        cn[:, 1:] = torch.cumsum(neg_rows.t().gather(1, order).to(torch.int64), 1)
        gain = cn.gather(1, start) + cn.gather(1, end)
        u2[g] = (gain * pos_rows.t().gather(1, order)).sum(1)
        hit = sc > 0
        tp[g] = (hit & pos_rows).sum(0)
        tn[g] = (~hit & neg_rows).sum(0)
    return u2, pos_rows.sum(0), rows.sum(), tp, tn


def score_auroc_reference(scores: torch.Tensor, bits: torch.Tensor, rows: torch.Tensor):
    """``score_auroc`` by the definition, a brute-force pair count, O(N^2) per column: for small cases."""
    G, N, K = scores.shape
    u2 = torch.zeros(G, K, dtype=torch.int64)
    tp, tn = torch.zeros_like(u2), torch.zeros_like(u2)
    scores, bits, rows = scores.float().cpu(), bits.cpu(), rows.cpu()
    for g in range(G):
        for k in range(K):
            s = scores[g, :, k]
            p, q = s[bits[:, k] & rows], s[~bits[:, k] & rows]
            u2[g, k] = (2 * (q[None, :] < p[:, None]).long() + (q[None, :] == p[:, None]).long()).sum()
            tp[g, k], tn[g, k] = (p > 0).sum(), (~(q > 0)).sum()
    return u2, (bits & rows.unsqueeze(1)).sum(0), rows.sum(), tp, tn


# ---------------------------------------------------------------------- the result type
@dataclass
class LinearProbes:
    """Ridge probes of G models for K concepts, fitted on the fit rows of a pool of ``n_rows`` rows."""

    weight: torch.Tensor       # fp32 [G, n, K]
    intercept: torch.Tensor    # fp64 [G, K]
    iters: torch.Tensor        # int32 [G, K]  iterations the concept was live
    converged: torch.Tensor    # bool [G, K]
    resid: torch.Tensor        # fp64 [G, K]   sqrt(gamma / gamma0) at the stop (0 for a constant concept)
    u2_fit: torch.Tensor       # int64 [G, K]  rank sums of the scores over the fit rows (``score_auroc``)
    pos_fit: torch.Tensor      # int64 [K]     positives among the fit rows
    cnt_fit: torch.Tensor      # int64 []      fit rows
    tp_fit: torch.Tensor       # int64 [G, K]  positives of the fit rows with score > 0
    tn_fit: torch.Tensor       # int64 [G, K]  negatives of the fit rows without
    u2_held: torch.Tensor      # the same over the held-out rows
    pos_held: torch.Tensor
    cnt_held: torch.Tensor
    tp_held: torch.Tensor
    tn_held: torch.Tensor
    skipped: torch.Tensor      # int64 [G]     rows the scoring pass left out by the skip rule (a fit refuses them)
    alpha: float
    n_rows: int

    _TENSORS = ("weight", "intercept", "iters", "converged", "resid", "u2_fit", "pos_fit", "cnt_fit", "tp_fit",
                "tn_fit", "u2_held", "pos_held", "cnt_held", "tp_held", "tn_held", "skipped")

    @property
    def n_concepts(self) -> int:
        return int(self.weight.shape[2])

    @staticmethod
    def _ratio(num, pos, cnt):
        den = 2 * pos * (cnt - pos)
        return num.to(torch.float64) / den.to(torch.float64).masked_fill(den == 0, float("nan"))

    def auroc(self) -> torch.Tensor:
        """fp64 [G, K]: the exact AUROC of the scores over the fit rows, ties counting half: one division of
        integers; NaN for a concept with no positive or no negative among them."""
        return self._ratio(self.u2_fit, self.pos_fit, self.cnt_fit)

    def auroc_heldout(self) -> torch.Tensor:
        """fp64 [G, K]: the same over the held-out rows (NaN everywhere when no row was held out)."""
        return self._ratio(self.u2_held, self.pos_held, self.cnt_held)

    def auroc_predicted(self, heldout: bool = False) -> torch.Tensor:
        """fp64 [G, K]: the AUROC of the hard predictions ``score > 0``, which is their balanced accuracy -- the
        number the reference's ``ridge_regression_auroc`` reports (``roc_auc_score(y, clf.predict(X))``).  From
        integer counts; NaN for a concept with no positive or no negative."""
        tp, tn, pos, cnt = ((self.tp_held, self.tn_held, self.pos_held, self.cnt_held) if heldout else
                            (self.tp_fit, self.tn_fit, self.pos_fit, self.cnt_fit))
        return self._ratio(tp * (cnt - pos) + tn * pos, pos, cnt)

    def scores(self, sparse_codes: SparseCodes, nactive=None, *, kernels: Optional[bool] = None) -> torch.Tensor:
        """fp32 [G, N', K]: ``C w + b`` on any codes of the same models (``ops.probe.rows_matmul`` when they are on
        a GPU, dense torch elsewhere or with ``kernels=False``).  A row the skip rule leaves out scores 0."""
        if sparse_codes.n_models != self.weight.shape[0] or sparse_codes.n != self.weight.shape[1]:
            raise ValueError("scores: codes of another ensemble")
        dev = sparse_codes.col.device
        w, b = self.weight.to(dev), self.intercept.to(dev)
        if sparse_codes.col.is_cuda if kernels is None else kernels:
            return _scores_fused(sparse_codes, w.float(), b, _nactive(nactive, sparse_codes))[0]
        dense, bad = _dense_codes(sparse_codes, nactive, torch.float64)
        return _scores_dense(dense, bad, w.double(), b).float()

    def top_features(self, m: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(feature int64 [G, K, m], weight [G, K, m]): per model and concept the ``m`` features with the largest
        ``|weight|``, descending, then feature ascending."""
        w = self.weight.transpose(1, 2)
        if isinstance(m, bool) or int(m) != m or not 1 <= int(m) <= w.shape[-1]:
            raise ValueError(f"m must be an integer in 1..{w.shape[-1]}, got {m!r}")
        feat = torch.sort(w.abs(), dim=-1, descending=True, stable=True).indices[..., :int(m)]
        return feat, torch.gather(w, -1, feat)

    def state_dict(self):
        sd = {k: getattr(self, k) for k in self._TENSORS}
        sd["alpha"] = torch.tensor(float(self.alpha), dtype=torch.float64)
        sd["n_rows"] = torch.tensor(int(self.n_rows), dtype=torch.int64)
        return sd

    def save(self, path):
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, map_location="cpu") -> "LinearProbes":
        sd = torch.load(path, map_location=map_location, weights_only=True)
        return cls(*(sd[k] for k in cls._TENSORS), float(sd["alpha"]), int(sd["n_rows"]))

    def to(self, device) -> "LinearProbes":
        return LinearProbes(*(getattr(self, k).to(device) for k in self._TENSORS), self.alpha, self.n_rows)


# ---------------------------------------------------------------------- dense views (the oracles' side)
def _nactive(nactive, sc: SparseCodes):
    return None if nactive is None else live_counts(nactive, sc.n_models, sc.n, sc.col.device)


def _dense_codes(sc: SparseCodes, nactive, dtype):
    """(dense [G, N, n] in ``dtype``, skipped-row mask bool [G, N]) under the skip rule of ``rows_matmul``: a row
    with a column outside [0, lim) or entries past the buffers is left out whole.  (``row_ptr`` must be monotone.)"""
    G, N, n, dev = sc.n_models, sc.n_rows, sc.n, sc.col.device
    live = _nactive(nactive, sc)
    lim = torch.full((G,), n, dtype=torch.int64, device=dev) if live is None else live.to(torch.int64)
    dense = torch.zeros(G, N, n, dtype=dtype, device=dev)
    bad = torch.zeros(G, N, dtype=torch.bool, device=dev)
    for g in range(G):
        ptr = sc.row_ptr[g]
        ln = ptr[1:] - ptr[:-1]
        bad[g] = (ptr[:-1] < 0) | (ptr[1:] > sc.cap) | (ln > n)
        rows = sc.entry_rows(g)
        cols = sc.col[g, :rows.numel()].long()
        off = (cols < 0) | (cols >= lim[g])
        bad[g] |= torch.zeros(N, dtype=torch.int64, device=dev).index_add_(0, rows, off.to(torch.int64)) > 0
        keep = ~bad[g][rows]
        dense[g, rows[keep], cols[keep]] = sc.val[g, :rows.numel()][keep].to(dtype)
    return dense, bad


def _scores_dense(dense, bad, w, b):
    return (dense @ w + b.unsqueeze(1)).masked_fill(bad.unsqueeze(-1), 0.0)


# ---------------------------------------------------------------------- oracles of the three ops
def rows_matmul_reference(sc: SparseCodes, P: torch.Tensor, shift=None, mask=None, nactive=None):
    """fp64 oracle of ``ops.probe.rows_matmul`` on the codes ``sc``: ``(Q fp64 [G, N, 32], skipped int64 [G])``
    before the one rounding to fp32 (dense torch; the summation order is torch's)."""
    dense, bad = _dense_codes(sc, nactive, torch.float64)
    Q = dense @ P.double()
    if shift is not None:
        Q = Q - shift.unsqueeze(1)
    Q = Q.masked_fill(bad.unsqueeze(-1), 0.0)
    if mask is not None:
        Q = Q.masked_fill((mask == 0).view(1, -1, 1), 0.0)
    return Q, bad.sum(1)


def lists_matmul_reference(col_ptr, row, val, R: torch.Tensor):
    """fp64 oracle of ``ops.probe.lists_matmul``: ``S fp64 [G, n, 32]`` before the rounding (an entry whose row lies
    outside [0, N) is skipped)."""
    from ..ops.value_order import stored_ptr

    G, cap = row.shape
    n, N = col_ptr.shape[1] - 1, R.shape[1]
    b = stored_ptr(col_ptr, cap)
    S = torch.zeros(G, n, R.shape[2], dtype=torch.float64, device=R.device)
    for g in range(G):
        ln = b[g, 1:] - b[g, :-1]
        feat = torch.repeat_interleave(torch.arange(n, device=b.device), ln)
        at = int(b[g, 0]) + torch.arange(feat.numel(), device=b.device)
        r = row[g][at].long()
        ok = (r >= 0) & (r < N)
        S[g].index_add_(0, feat[ok], val[g][at][ok].double().unsqueeze(1) * R[g][r[ok]].double())
    return S


def col_dots_reference(A: torch.Tensor, B: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp64 oracle of ``ops.probe.col_dots``."""
    return (A.double() * (1.0 if B is None else B.double())).sum(1)


# ---------------------------------------------------------------------- closed form
def ridge_closed_form_reference(dense: torch.Tensor, bits: torch.Tensor, alpha: float = 1.0, fit_rows=None):
    """Dense normal equations, for small n: ``(weight fp64 [G, n, K], intercept fp64 [G, K])`` of
    ``RidgeClassifier(alpha)`` on the rows ``fit_rows`` of the dense codes ``dense`` [G, N, n] with targets +-1
    from ``bits`` bool [N, K]."""
    X = dense.double()
    if fit_rows is not None:
        X, bits = X[:, fit_rows], bits[fit_rows]
    y = bits.double() * 2 - 1
    mu, ybar = X.mean(1), y.mean(0)
    Xc, yc = X - mu.unsqueeze(1), y - ybar
    A = Xc.transpose(1, 2) @ Xc + alpha * torch.eye(X.shape[2], dtype=torch.float64, device=X.device)
    w = torch.linalg.solve(A, Xc.transpose(1, 2) @ yc)
    return w, ybar - (mu.unsqueeze(-1) * w).sum(1)


# ---------------------------------------------------------------------- the solver, written once
class _DenseOps:
    """The operator of the recurrence on dense codes in one number format (the oracle's side): every product, sum
    and scalar in ``dtype``, one torch operation per step."""

    def __init__(self, dense, mask, dtype):
        self.X, self.m, self.dtype = dense.to(dtype), mask.to(dtype).view(1, -1, 1), dtype
        self.nfit = mask.sum().to(dtype)
        self.mu = (self.X * self.m).sum(1) / self.nfit                # [G, n]

    def scalar(self, x):
        return x.to(self.dtype)

    def forward(self, v):          # Xc v on the fit rows
        return (self.X @ v - (self.mu.unsqueeze(-1) * v).sum(1, keepdim=True)) * self.m

    def adjoint(self, u, w, alpha):  # Xc^T u - alpha w
        return self.X.transpose(1, 2) @ u - self.mu.unsqueeze(-1) * u.sum(1, keepdim=True) - alpha * w

    def dots(self, a, b):
        return (a * b).sum(1)

    def axpby_(self, y, x, a, b):
        return y.copy_(a.unsqueeze(1) * x + b.unsqueeze(1) * y)

    def mu_dot(self, w):
        return (self.mu.unsqueeze(-1) * w).sum(1)


def _cgls(ops, yc, n: int, alpha: float, max_iter: int, tol: float):
    """The recurrence of the module docstring on ``ops``; ``yc`` [G, N, C] the centred targets, zero off the fit
    rows.  Returns (w, iters int32, converged, resid, gamma0); every scalar is [G, C] in ``ops``' format."""
    G, _, C = yc.shape
    w = torch.zeros(G, n, C, dtype=yc.dtype, device=yc.device)
    r = yc.clone()
    s = ops.adjoint(r, w, alpha)
    p = s.clone()
    gamma = ops.dots(s, s)
    gamma0 = gamma.clone()
    live = gamma0 > 0
    iters = torch.zeros(G, C, dtype=torch.int32, device=yc.device)
    one, zero = torch.ones_like(gamma), torch.zeros_like(gamma)
    tol2 = ops.scalar(torch.tensor(tol, dtype=torch.float64)) ** 2
    for _ in range(max_iter):
        live = live & (gamma > tol2 * gamma0)
        q = ops.forward(p)
        delta = ops.dots(q, q) + alpha * ops.dots(p, p)
        ok = live & (delta > 0)
        a = torch.where(ok, gamma / torch.where(ok, delta, one), zero)
        ops.axpby_(w, p, a, one)
        ops.axpby_(r, q, -a, one)
        s = ops.adjoint(r, w, alpha)
        gamma_new = ops.dots(s, s)
        b = torch.where(live, gamma_new / torch.where(live, gamma, one), zero)
        ops.axpby_(p, s, torch.where(live, one, zero), torch.where(live, b, one))
        gamma = torch.where(live, gamma_new, gamma)
        iters += live.to(torch.int32)
    converged = gamma <= tol2 * gamma0
    resid = torch.sqrt(gamma / torch.where(gamma0 > 0, gamma0, one))
    return w, iters, converged, resid.double(), gamma0


def _finish(w, b, it, conv, resid, scores, skipped, bits, fit, alpha, n_rows) -> LinearProbes:
    fit_sums = score_auroc(scores, bits, fit)
    held_sums = score_auroc(scores, bits, ~fit)
    return LinearProbes(w, b, it, conv, resid, *fit_sums, *held_sums, skipped, float(alpha), int(n_rows))


def _targets(bits, fit, dtype):
    """(ybar [K], yc [N, K]) in ``dtype``: the mean of the +-1 targets over the fit rows and the centred targets,
    zero off the fit rows."""
    y = bits.to(dtype) * 2 - 1
    m = fit.to(dtype).unsqueeze(1)
    ybar = (y * m).sum(0) / fit.sum().to(dtype)
    return ybar, (y - ybar) * m


def ridge_probes_reference(sparse_codes: SparseCodes, flags: torch.Tensor, n_concepts=None, *, alpha: float = 1.0,
                           fit_rows=None, max_iter: int = 64, tol: float = 1e-5, nactive=None,
                           dtype=torch.float64) -> LinearProbes:
    """Torch oracle of ``ridge_probes`` (any device; this is what runs off the GPU): the same recurrence on
    ``to_dense`` codes with every product, sum and scalar in ``dtype`` -- fp64 is the reference (its ``weight`` is
    fp64, and ``tol`` may go below the device route's floor), fp32 the plain evaluation of the recurrence that the
    device route's error is measured against."""
    alpha, max_iter, tol = check_solver(alpha, max_iter, tol, 1e-15 if dtype == torch.float64 else MIN_TOL)
    sparse_codes.check()
    dev = sparse_codes.col.device
    flags, K = check_flags(flags, sparse_codes.n_rows, n_concepts, dev)
    fit = check_fit_rows(fit_rows, sparse_codes.n_rows, dev)
    bits = concept_bits(flags, K)
    dense, bad = _dense_codes(sparse_codes, nactive, dtype)
    if bool(bad.any()):
        raise FeatureCodesSkipped(f"{bad.sum(1).tolist()} rows per model fail the skip rule (of "
                                  f"{sparse_codes.n_rows}): ridge_probes needs valid codes for every row")
    ops = _DenseOps(dense, fit, dtype)
    ybar, yc = _targets(bits, fit, dtype)
    w, it, conv, resid, _ = _cgls(ops, yc.unsqueeze(0).expand(dense.shape[0], -1, -1).contiguous(), sparse_codes.n,
                                  alpha, max_iter, tol)
    b = (ybar - ops.mu_dot(w)).double()
    scores = _scores_dense(dense.double(), bad, w.double(), b).float()
    return _finish(w, b, it, conv, resid, scores, bad.sum(1), bits, fit, alpha, sparse_codes.n_rows)


# ---------------------------------------------------------------------- the device route
def _pad(t: torch.Tensor) -> torch.Tensor:
    """``t`` [..., K] as a contiguous [..., 32] with zero columns behind."""
    out = t.new_zeros(*t.shape[:-1], CONCEPTS)
    out[..., :t.shape[-1]] = t
    return out


def _scores_fused(sc: SparseCodes, w: torch.Tensor, b: torch.Tensor, nactive, waves=None):
    """(scores fp32 [G, N, K], skipped) = C w + b: one ``rows_matmul`` with shift -b."""
    from ..ops import probe as pr

    K = w.shape[2]
    Q, skipped = pr.rows_matmul(sc.row_ptr.contiguous(), sc.col, sc.val, _pad(w.contiguous()), shift=_pad(-b.double()),
                                nactive=nactive, waves=waves)
    return Q[..., :K], skipped


class _KernelOps:
    """The operator of the recurrence on the kernels of ``ops.probe``: fp32 iterates [G, M, 32], fp64 sums and
    scalars [G, 32]."""

    def __init__(self, sc: SparseCodes, fc, fit, nactive, waves):
        from ..ops import probe as pr

        self.pr, self.sc, self.fc, self.nactive, self.waves = pr, sc, fc, nactive, waves
        G, N, dev = sc.n_models, sc.n_rows, sc.col.device
        self.row_ptr = sc.row_ptr.contiguous()
        self.col_ptr = fc.col_ptr.contiguous()
        self.plan = pr.lists_plan(self.col_ptr, fc.cap)
        self.mask = fit.to(torch.uint8).contiguous()
        self.nfit = fit.sum().to(torch.float64)
        ones = fit.to(torch.float32).view(1, N, 1).expand(G, N, CONCEPTS).contiguous()
        mu = self.lists(ones)[:, :, 0].double() / self.nfit            # the feature means over the fit rows
        self.mu32 = mu.float().unsqueeze(-1).expand(-1, -1, CONCEPTS).contiguous()
        self.mu64 = self.mu32[:, :, :1].double()
        self.q = torch.empty(G, N, CONCEPTS, device=dev, dtype=torch.float32)
        self.scratch = torch.zeros(G, device=dev, dtype=torch.int64)

    def scalar(self, x):
        return x.to(torch.float64)

    def lists(self, R):
        return self.pr.lists_matmul(self.col_ptr, self.fc.row, self.fc.val, R, plan=self.plan, waves=self.waves)

    def forward(self, v):
        shift = self.pr.col_dots(v, self.mu32, waves=self.waves)
        self.pr.rows_matmul(self.row_ptr, self.sc.col, self.sc.val, v, shift=shift, mask=self.mask,
                            nactive=self.nactive, skipped=self.scratch, out=self.q, waves=self.waves)
        return self.q

    def adjoint(self, u, w, alpha):
        S, su = self.lists(u), self.pr.col_dots(u, waves=self.waves)
        return (S.double() - self.mu64 * su.unsqueeze(1) - alpha * w.double()).float()

    def dots(self, a, b):
        return self.pr.col_dots(a, b, waves=self.waves)

    def axpby_(self, y, x, a, b):
        return self.pr.axpby_(y, x, a.contiguous(), b.contiguous())

    def mu_dot(self, w):
        return self.pr.col_dots(w, self.mu32, waves=self.waves)


def ridge_probes_fused(sparse_codes: SparseCodes, flags: torch.Tensor, n_concepts=None, *, alpha: float = 1.0,
                       fit_rows=None, max_iter: int = 64, tol: float = 1e-5, nactive=None, feature_codes=None,
                       waves: Optional[int] = None) -> LinearProbes:
    """``ridge_probes`` on the kernels of ``csrc/probe.hip``: ``by_feature`` (or ``feature_codes``, the lists of
    these codes from an earlier call), then per iteration one ``rows_matmul`` over the CSR rows, one
    ``lists_matmul`` over the feature lists, five ``col_dots`` and three ``axpby_``; the scores are one more
    ``rows_matmul``.  Synchronises before the loop (``SparseCodes.check()`` and ``FeatureCodes.check()``: every row
    must be stored and valid); the loop reads nothing to the host."""
    from .feature_codes import by_feature

    alpha, max_iter, tol = check_solver(alpha, max_iter, tol)
    sparse_codes.check()
    dev = sparse_codes.col.device
    flags, K = check_flags(flags, sparse_codes.n_rows, n_concepts, dev)
    fit = check_fit_rows(fit_rows, sparse_codes.n_rows, dev)
    bits = concept_bits(flags, K)
    nactive = _nactive(nactive, sparse_codes)
    fc = (by_feature(sparse_codes, nactive) if feature_codes is None else feature_codes).check()
    ops = _KernelOps(sparse_codes, fc, fit, nactive, waves)
    ybar, yc = _targets(bits, fit, torch.float64)
    G = sparse_codes.n_models
    w, it, conv, resid, _ = _cgls(ops, _pad(yc.float()).unsqueeze(0).expand(G, -1, -1).contiguous(), sparse_codes.n,
                                  alpha, max_iter, tol)
    b = ybar - ops.mu_dot(w)[:, :K]
    w = w[..., :K].contiguous()
    scores, skipped = _scores_fused(sparse_codes, w, b, nactive, waves)
    return _finish(w, b, it[:, :K].contiguous(), conv[:, :K].contiguous(), resid[:, :K].contiguous(), scores, skipped,
                   bits, fit, alpha, sparse_codes.n_rows)


def ridge_probes(sparse_codes: SparseCodes, flags: torch.Tensor, n_concepts=None, *, kernels: Optional[bool] = None,
                 **kw) -> LinearProbes:
    """The ``LinearProbes`` of the complete sparse codes ``sparse_codes`` against the concepts of ``flags`` (int32
    words [n_rows], ``n_concepts`` of them, default 32, or a bool [n_rows, K] matrix): keywords ``alpha`` (1.0,
    sklearn's default), ``fit_rows``, ``max_iter`` (64), ``tol`` (1e-5; below 1e-6 is refused), ``nactive``.  The
    kernels when the codes are on a GPU (further keywords ``feature_codes``, ``waves``), the oracle elsewhere or
    with ``kernels=False`` (its fp64 weights rounded to fp32).  Synchronises before the fit
    (``SparseCodesOverflow`` if entries were dropped, ``FeatureCodesSkipped`` if a row fails the skip rule)."""
    if sparse_codes.col.is_cuda if kernels is None else kernels:
        return ridge_probes_fused(sparse_codes, flags, n_concepts, **kw)
    for k in ("feature_codes", "waves"):
        if kw.pop(k, None) is not None:
            raise TypeError(f"ridge_probes: {k} is a keyword of the device route")
    res = ridge_probes_reference(sparse_codes, flags, n_concepts, **kw)
    res.weight = res.weight.float()
    return res


# ====================================================================== logistic probes
MIN_TOL_LOGISTIC = 1e-5   # fp32 iterates cannot promise a smaller relative gradient
ARMIJO = 1e-4             # sufficient-decrease constant of the line search


def check_logistic(C, max_iter, cg_iter, tol, min_tol: float = MIN_TOL_LOGISTIC):
    C = float(C)
    if not C > 0.0 or not math.isfinite(C):
        raise ValueError(f"C must be a finite number > 0 (the inverse of the penalty's strength), got {C!r}")
    for name, v in (("max_iter", max_iter), ("cg_iter", cg_iter)):
        if isinstance(v, bool) or int(v) != v or int(v) < 0:
            raise ValueError(f"{name} must be a non-negative integer, got {v!r}")
    tol = float(tol)
    if not tol >= min_tol or not tol < 1.0:
        raise ValueError(f"tol must lie in [{min_tol:g}, 1): fp32 iterates cannot promise less (got {tol!r})")
    return C, int(max_iter), int(cg_iter), tol


def _softplus_loss(z, t):
    """``softplus(z) - t z`` with the stable ``softplus(z) = max(z, 0) + log1p(exp(-|z|))``; ``t`` bool."""
    return z.clamp(min=0) + torch.log1p(torch.exp(-z.abs())) - torch.where(t, z, torch.zeros_like(z))


def _logit_terms(z, t, m):
    """(r, D, loss [G, K]) of the margins ``z`` [G, N, K] in their own format: ``t`` bool [N, K] the targets, ``m``
    bool [N] the fit rows.  From ``e = exp(-|z|)`` alone, as ``csrc/probe.hip``: ``sigma(|z|) = 1 / (1 + e)`` and
    ``sigma(-|z|) = e / (1 + e)``, so neither sigma nor 1 - sigma is a difference of nearly equal numbers."""
    e = torch.exp(-z.abs())
    big = 1.0 / (1.0 + e)
    small = e * big
    up = z >= 0
    r = torch.where(t, -torch.where(up, small, big), torch.where(up, big, small))
    loss = z.clamp(min=0) + torch.log1p(e) - torch.where(t, z, torch.zeros_like(z))
    m, zero = m.view(1, -1, 1), torch.zeros_like(z)
    return torch.where(m, r, zero), torch.where(m, big * small, zero), torch.where(m, loss, zero).sum(1)


def logit_terms_reference(Z: torch.Tensor, flags: torch.Tensor, mask: torch.Tensor):
    """fp64 oracle of ``ops.probe.logit_terms``: ``(R fp64 [G, N, 32], D fp64 [G, N, 32], loss fp64 [G, 32])`` before
    the one rounding of ``R`` and ``D`` (the summation order of ``loss`` is torch's)."""
    return _logit_terms(Z.double(), concept_bits(flags, Z.shape[2]), mask != 0)


def line_losses_reference(Z: torch.Tensor, U: torch.Tensor, flags: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """fp64 oracle of ``ops.probe.line_losses``: fp64 [G, 8, 32], the loss sums at ``Z + 2^-j U``."""
    from ..ops.probe import LINE_STEPS

    t, m = concept_bits(flags, Z.shape[2]), (mask != 0).view(1, -1, 1)
    z, u = Z.double(), U.double()
    return torch.stack([torch.where(m, _softplus_loss(z + 2.0 ** -j * u, t), torch.zeros_like(z)).sum(1)
                        for j in range(LINE_STEPS)], 1)


@dataclass
class LogisticProbes:
    """Logistic-regression probes of G models for K concepts, fitted on the fit rows of a pool of ``n_rows`` rows:
    exactly ``sklearn.linear_model.LogisticRegression(C=C)`` per (model, concept)."""

    weight: torch.Tensor       # fp32 [G, n, K]
    intercept: torch.Tensor    # fp64 [G, K]
    iters: torch.Tensor        # int32 [G, K]  outer (Newton) steps the concept was live
    cg_iters: torch.Tensor     # int32 [G, K]  inner (CG) iterations the concept was live, in total
    converged: torch.Tensor    # bool [G, K]
    stalled: torch.Tensor      # bool [G, K]   no candidate of the line search passed: frozen where it stood
    resid: torch.Tensor        # fp64 [G, K]   |g| / |g0| at the stop (0 for a constant concept)
    loss: torch.Tensor         # fp64 [G, K]   the objective at the stop
    u2_fit: torch.Tensor       # int64 [G, K]  rank sums of the logits over the fit rows (``score_auroc``)
    pos_fit: torch.Tensor      # int64 [K]
    cnt_fit: torch.Tensor      # int64 []
    tp_fit: torch.Tensor       # int64 [G, K]  positives of the fit rows with logit > 0
    tn_fit: torch.Tensor       # int64 [G, K]  negatives of the fit rows without
    u2_held: torch.Tensor      # the same over the held-out rows
    pos_held: torch.Tensor
    cnt_held: torch.Tensor
    tp_held: torch.Tensor
    tn_held: torch.Tensor
    skipped: torch.Tensor      # int64 [G]     rows the scoring pass left out by the skip rule (a fit refuses them)
    C: float
    n_rows: int

    _TENSORS = ("weight", "intercept", "iters", "cg_iters", "converged", "stalled", "resid", "loss", "u2_fit",
                "pos_fit", "cnt_fit", "tp_fit", "tn_fit", "u2_held", "pos_held", "cnt_held", "tp_held", "tn_held",
                "skipped")

    n_concepts = LinearProbes.n_concepts
    _ratio = staticmethod(LinearProbes._ratio)
    top_features = LinearProbes.top_features

    def auroc(self) -> torch.Tensor:
        """fp64 [G, K]: the exact AUROC of the **logits** over the fit rows, ties counting half; NaN for a concept
        with no positive or no negative among them.  Sigma is monotone, so this is the reference's
        ``roc_auc_score(y, clf.predict_proba(X)[:, 1])`` -- without the ties that fp32 probabilities saturate
        into at 0 and 1."""
        return self._ratio(self.u2_fit, self.pos_fit, self.cnt_fit)

    def auroc_heldout(self) -> torch.Tensor:
        """fp64 [G, K]: the same over the held-out rows (NaN everywhere when no row was held out)."""
        return self._ratio(self.u2_held, self.pos_held, self.cnt_held)

    def auroc_predicted(self, heldout: bool = False) -> torch.Tensor:
        """fp64 [G, K]: the AUROC of the hard predictions ``logit > 0`` (probability above one half), which is
        their balanced accuracy.  From integer counts; NaN for a concept with no positive or no negative."""
        return LinearProbes.auroc_predicted(self, heldout)

    def scores(self, sparse_codes: SparseCodes, nactive=None, *, kernels: Optional[bool] = None) -> torch.Tensor:
        """fp32 [G, N', K]: the logits ``C w + b`` on any codes of the same models (``ops.probe.rows_matmul`` when
        they are on a GPU, dense torch elsewhere or with ``kernels=False``).  A row the skip rule leaves out
        scores 0."""
        return LinearProbes.scores(self, sparse_codes, nactive, kernels=kernels)

    def predict_proba(self, sparse_codes: SparseCodes, nactive=None, *, kernels: Optional[bool] = None):
        """fp32 [G, N', K]: ``sigma(scores)``, the probability of the positive class (torch)."""
        return torch.sigmoid(self.scores(sparse_codes, nactive, kernels=kernels))

    def state_dict(self):
        sd = {k: getattr(self, k) for k in self._TENSORS}
        sd["C"] = torch.tensor(float(self.C), dtype=torch.float64)
        sd["n_rows"] = torch.tensor(int(self.n_rows), dtype=torch.int64)
        return sd

    def save(self, path):
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, map_location="cpu") -> "LogisticProbes":
        sd = torch.load(path, map_location=map_location, weights_only=True)
        return cls(*(sd[k] for k in cls._TENSORS), float(sd["C"]), int(sd["n_rows"]))

    def to(self, device) -> "LogisticProbes":
        return LogisticProbes(*(getattr(self, k).to(device) for k in self._TENSORS), self.C, self.n_rows)


# ---------------------------------------------------------------------- the operators of the Newton loop
class _DenseLogitOps(_DenseOps):
    """``_DenseOps`` with the logistic terms: every product, sum and scalar in ``dtype``."""

    def __init__(self, dense, mask, dtype, bits):
        super().__init__(dense, mask, dtype)
        self.t, self.fit, self.n_models = bits, mask, dense.shape[0]
        self.vdtype = self.sdtype = dtype

    def margins(self, v, vb, slot="z"):     # Xc v + vb on the fit rows
        return self.forward(v) + vb.unsqueeze(1) * self.m

    def terms(self, z):
        return _logit_terms(z, self.t, self.fit)

    def grad(self, r, w, lam):              # (Xc^T r + lam w, sum r)
        return self.adjoint(r, w, -lam), r.sum(1)

    def hess(self, D, v, vb, lam):          # the same of q = D o (Xc v + vb)
        return self.grad(D * self.margins(v, vb), v, lam)

    def line(self, z, u):
        from ..ops.probe import LINE_STEPS

        m, zero = self.fit.view(1, -1, 1), torch.zeros_like(z)
        return torch.stack([torch.where(m, _softplus_loss(z + 2.0 ** -j * u, self.t), zero).sum(1)
                            for j in range(LINE_STEPS)], 1)


class _KernelLogitOps(_KernelOps):
    """``_KernelOps`` with the logistic kernels: fp32 iterates [G, M, 32], fp64 sums and scalars [G, 32]."""

    vdtype, sdtype = torch.float32, torch.float64

    def __init__(self, sc, fc, fit, nactive, waves, flags):
        super().__init__(sc, fc, fit, nactive, waves)
        G, N, dev = sc.n_models, sc.n_rows, sc.col.device
        self.flags, self.n_models = flags.contiguous(), G
        self.slots = {k: torch.empty(G, N, CONCEPTS, device=dev, dtype=torch.float32) for k in ("z", "u", "r", "D")}
        self.loss = torch.empty(G, CONCEPTS, device=dev, dtype=torch.float64)

    def _rows(self, v, vb, out, scale=None):
        shift = self.pr.col_dots(v, self.mu32, waves=self.waves) - vb
        self.pr.rows_matmul(self.row_ptr, self.sc.col, self.sc.val, v, shift=shift, mask=self.mask,
                            nactive=self.nactive, skipped=self.scratch, out=out, waves=self.waves, scale=scale)
        return out

    def margins(self, v, vb, slot="z"):
        return self._rows(v, vb, self.slots[slot])

    def terms(self, z):
        return self.pr.logit_terms(z, self.flags, self.mask, out=(self.slots["r"], self.slots["D"], self.loss),
                                   waves=self.waves)

    def grad(self, r, w, lam):
        S, su = self.lists(r), self.pr.col_dots(r, waves=self.waves)
        return (S.double() - self.mu64 * su.unsqueeze(1) + lam * w.double()).float(), su

    def hess(self, D, v, vb, lam):
        return self.grad(self._rows(v, vb, self.q, scale=D), v, lam)

    def line(self, z, u):
        return self.pr.line_losses(z, u, self.flags, self.mask, waves=self.waves)


def _armijo(fj, f, gd, steps):
    """(step [G, C], found bool [G, C]): the largest candidate ``steps[j]`` with ``fj[:, j] <= f + ARMIJO steps[j]
    gd`` (``fj`` [G, J, C] the objective at the candidates, ``f`` at 0, ``gd`` the slope)."""
    step = torch.zeros_like(f)
    for j in reversed(range(steps.numel())):
        step = torch.where(fj[:, j] <= f + ARMIJO * steps[j] * gd, steps[j], step)
    return step, step > 0


def _newton_cg(ops, n: int, pos, C: float, max_iter: int, cg_iter: int, tol: float, early_stop: bool = True,
               step_rule=_armijo):
    """The recurrence of the module docstring on ``ops``; ``pos`` [C] the positives among the fit rows.  Returns
    (w, b', iters, cg_iters, converged, stalled, resid, objective); every scalar is [G, C] in ``ops``' format."""
    from ..ops.probe import LINE_STEPS

    sd, dev, G, cols = ops.sdtype, pos.device, ops.n_models, pos.numel()
    lam = 1.0 / C
    nfit = ops.nfit.to(sd)
    pos = pos.to(sd)
    neg = nfit - pos
    const = (pos == 0) | (neg == 0)
    clip = torch.log(2 * nfit)
    one, zero = torch.ones(G, cols, dtype=sd, device=dev), torch.zeros(G, cols, dtype=sd, device=dev)
    b0 = torch.where(const, torch.where(pos > 0, clip, -clip),
                     torch.log(torch.where(const, one[0], pos) / torch.where(const, one[0], neg)))
    b = b0.expand(G, cols).clone()
    w = torch.zeros(G, n, cols, dtype=ops.vdtype, device=dev)
    d, res, p = torch.zeros_like(w), torch.zeros_like(w), torch.zeros_like(w)

    def evaluate():
        z = ops.margins(w, b)
        r, D, L = ops.terms(z)
        ww = ops.dots(w, w)
        gw, gb = ops.grad(r, w, lam)
        return z, D, ww, L + 0.5 * lam * ww, gw, gb, ops.dots(gw, gw) + gb * gb

    z, D, ww, f, gw, gb, gn2 = evaluate()
    g0 = gn2.clone()
    live = ~const & (g0 > 0)
    stalled = torch.zeros_like(live)
    iters = torch.zeros(G, cols, dtype=torch.int32, device=dev)
    cg_iters = torch.zeros_like(iters)
    tol2 = ops.scalar(torch.tensor(tol, dtype=torch.float64)) ** 2
    steps = (2.0 ** -torch.arange(LINE_STEPS, dtype=torch.float64, device=dev)).to(sd)
    for _ in range(max_iter):
        live = live & (gn2 > tol2 * g0)
        if early_stop and not bool(live.any()):
            break
        iters += live.to(torch.int32)
        # conjugate gradients on H d = -g, truncated at |res| <= eta |g|
        lv = torch.where(live, one, zero)
        d.zero_()
        db = zero.clone()
        ops.axpby_(res, gw, -lv, zero)
        rb = -gb * lv
        ops.axpby_(p, res, one, zero)
        pb = rb.clone()
        rho = gn2 * lv
        stop2 = torch.minimum(0.25 * one, torch.sqrt(gn2 / torch.where(g0 > 0, g0, one))) * gn2
        cgl = live
        for _ in range(cg_iter):
            cgl = cgl & (rho > stop2)
            hw, hb = ops.hess(D, p, pb, lam)
            php = ops.dots(p, hw) + pb * hb
            ok = cgl & (php > 0)
            a = torch.where(ok, rho / torch.where(ok, php, one), zero)
            ops.axpby_(d, p, a, one)
            db = db + a * pb
            ops.axpby_(res, hw, -a, one)
            rb = rb - a * hb
            rho_new = ops.dots(res, res) + rb * rb
            beta = torch.where(cgl, rho_new / torch.where(cgl, rho, one), zero)
            ops.axpby_(p, res, torch.where(cgl, one, zero), torch.where(cgl, beta, one))
            pb = torch.where(cgl, rb + beta * pb, pb)
            rho = torch.where(cgl, rho_new, rho)
            cg_iters += cgl.to(torch.int32)
        # Armijo backtracking over the candidates 2^-j, all from one pass: z is linear in the step
        u = ops.margins(d, db, "u")
        gd = ops.dots(gw, d) + gb * db
        wd, dd = ops.dots(w, d), ops.dots(d, d)
        t = steps.view(1, -1, 1)
        fj = ops.line(z, u) + 0.5 * lam * (ww.unsqueeze(1) + 2 * t * wd.unsqueeze(1) + t * t * dd.unsqueeze(1))
        step, found = step_rule(fj, f, gd, steps)
        stalled = stalled | (live & ~found)
        live = live & found
        step = torch.where(live, step, zero)
        ops.axpby_(w, d, step, one)
        b = b + step * db
        z, D, ww, f, gw, gb, gn2 = evaluate()
    converged = const | (gn2 <= tol2 * g0)
    resid = torch.where(const, zero, torch.sqrt(gn2 / torch.where(g0 > 0, g0, one)))
    return w, b, iters, cg_iters, converged, stalled, resid.double(), f.double()


def _finish_logistic(w, b, out, scores, skipped, bits, fit, C, n_rows) -> LogisticProbes:
    it, cg, conv, stalled, resid, loss = out
    fit_sums = score_auroc(scores, bits, fit)
    held_sums = score_auroc(scores, bits, ~fit)
    return LogisticProbes(w, b, it, cg, conv, stalled, resid, loss, *fit_sums, *held_sums, skipped, float(C),
                          int(n_rows))


def logistic_probes_reference(sparse_codes: SparseCodes, flags: torch.Tensor, n_concepts=None, *, C: float = 1.0,
                              fit_rows=None, max_iter: int = 12, cg_iter: int = 16, tol: float = 1e-4,
                              early_stop: bool = True, nactive=None, dtype=torch.float64) -> LogisticProbes:
    """Torch oracle of ``logistic_probes`` (any device; this is what runs off the GPU): the same recurrence on
    ``to_dense`` codes with every product, sum and scalar in ``dtype`` -- fp64 is the reference (its ``weight`` is
    fp64, and ``tol`` may go below the device route's floor), fp32 the plain evaluation of the recurrence that the
    device route's error is measured against."""
    C, max_iter, cg_iter, tol = check_logistic(C, max_iter, cg_iter, tol,
                                               1e-15 if dtype == torch.float64 else MIN_TOL_LOGISTIC)
    sparse_codes.check()
    dev = sparse_codes.col.device
    flags, K = check_flags(flags, sparse_codes.n_rows, n_concepts, dev)
    fit = check_fit_rows(fit_rows, sparse_codes.n_rows, dev)
    bits = concept_bits(flags, K)
    dense, bad = _dense_codes(sparse_codes, nactive, dtype)
    if bool(bad.any()):
        raise FeatureCodesSkipped(f"{bad.sum(1).tolist()} rows per model fail the skip rule (of "
                                  f"{sparse_codes.n_rows}): logistic_probes needs valid codes for every row")
    ops = _DenseLogitOps(dense, fit, dtype, bits)
    w, bc, *out = _newton_cg(ops, sparse_codes.n, (bits & fit.unsqueeze(1)).sum(0), C, max_iter, cg_iter, tol,
                             early_stop)
    b = (bc - ops.mu_dot(w)).double()
    scores = _scores_dense(dense.double(), bad, w.double(), b).float()
    return _finish_logistic(w, b, out, scores, bad.sum(1), bits, fit, C, sparse_codes.n_rows)


def logistic_probes_fused(sparse_codes: SparseCodes, flags: torch.Tensor, n_concepts=None, *, C: float = 1.0,
                          fit_rows=None, max_iter: int = 12, cg_iter: int = 16, tol: float = 1e-4,
                          early_stop: bool = True, nactive=None, feature_codes=None,
                          waves: Optional[int] = None) -> LogisticProbes:
    """``logistic_probes`` on the kernels of ``csrc/probe.hip``: ``by_feature`` (or ``feature_codes``), then per
    outer step one ``logit_terms``, per inner iteration one ``rows_matmul(scale=D)`` over the CSR rows and one
    ``lists_matmul`` over the feature lists, and one ``line_losses`` for the eight step candidates; the logits are
    one more ``rows_matmul``.  Synchronises before the loop (``SparseCodes.check()`` and ``FeatureCodes.check()``);
    with ``early_stop`` the loop reads one bool per outer step, without it nothing."""
    from .feature_codes import by_feature
    from .value_order import concept_words

    C, max_iter, cg_iter, tol = check_logistic(C, max_iter, cg_iter, tol)
    sparse_codes.check()
    dev = sparse_codes.col.device
    flags, K = check_flags(flags, sparse_codes.n_rows, n_concepts, dev)
    fit = check_fit_rows(fit_rows, sparse_codes.n_rows, dev)
    bits = concept_bits(flags, K)
    nactive = _nactive(nactive, sparse_codes)
    fc = (by_feature(sparse_codes, nactive) if feature_codes is None else feature_codes).check()
    ops = _KernelLogitOps(sparse_codes, fc, fit, nactive, waves, concept_words(bits))
    w, bc, *out = _newton_cg(ops, sparse_codes.n, _pad((bits & fit.unsqueeze(1)).sum(0)), C, max_iter, cg_iter, tol,
                             early_stop)
    b = (bc - ops.mu_dot(w))[:, :K].contiguous()
    w = w[..., :K].contiguous()
    scores, skipped = _scores_fused(sparse_codes, w, b, nactive, waves)
    return _finish_logistic(w, b, [t[:, :K].contiguous() for t in out], scores, skipped, bits, fit, C,
                            sparse_codes.n_rows)


def logistic_probes(sparse_codes: SparseCodes, flags: torch.Tensor, n_concepts=None, *,
                    kernels: Optional[bool] = None, **kw) -> LogisticProbes:
    """The ``LogisticProbes`` of the complete sparse codes ``sparse_codes`` against the concepts of ``flags`` (int32
    words [n_rows], ``n_concepts`` of them, default 32, or a bool [n_rows, K] matrix): keywords ``C`` (1.0,
    sklearn's default), ``fit_rows``, ``max_iter`` (12), ``cg_iter`` (16), ``tol`` (1e-4), ``early_stop``,
    ``nactive``.  The kernels when the codes are on a GPU (further keywords ``feature_codes``, ``waves``), the oracle
    elsewhere or with ``kernels=False`` (its fp64 weights rounded to fp32).  The floor of ``tol`` belongs to fp32
    iterates: the kernels (and the oracle with ``dtype=torch.float32``) refuse a ``tol`` below 1e-5, the fp64 oracle
    that runs off the GPU takes any ``tol`` down to 1e-15, as in ``ridge_probes``.  Synchronises
    before the fit (``SparseCodesOverflow`` if entries were dropped, ``FeatureCodesSkipped`` if a row fails the
    skip rule)."""
    if sparse_codes.col.is_cuda if kernels is None else kernels:
        return logistic_probes_fused(sparse_codes, flags, n_concepts, **kw)
    for k in ("feature_codes", "waves"):
        if kw.pop(k, None) is not None:
            raise TypeError(f"logistic_probes: {k} is a keyword of the device route")
    res = logistic_probes_reference(sparse_codes, flags, n_concepts, **kw)
    res.weight = res.weight.float()
    return res


def logistic_newton_reference(dense: torch.Tensor, bits: torch.Tensor, C: float = 1.0, fit_rows=None,
                              max_steps: int = 100):
    """Plain dense Newton with exact solves, for small n: ``(weight fp64 [G, n, K], intercept fp64 [G, K])`` of
    ``LogisticRegression(C=C)`` on the rows ``fit_rows`` of the dense codes ``dense`` [G, N, n] with targets from
    ``bits`` bool [N, K], run until ``|g| <= 1e-12 |g0|`` (g0 the gradient at w = 0, b = log(pos / neg)) or until
    the objective stops falling in fp64.  A concept that is constant on the rows gets weight 0 and intercept
    ``+-log(2 n_fit)``, as the probes do."""
    X = dense.double()
    if fit_rows is not None:
        X, bits = X[:, fit_rows], bits[fit_rows]
    G, N, n = X.shape
    K = bits.shape[1]
    t = bits.unsqueeze(0)
    A = torch.cat([X, torch.ones(G, N, 1, dtype=torch.float64, device=X.device)], 2)            # [G, N, n + 1]
    pen = torch.full((n + 1,), 1.0 / C, dtype=torch.float64, device=X.device)
    pen[n] = 0.0
    pos = bits.sum(0).double()
    const = (pos == 0) | (pos == N)
    safe = torch.where(const, torch.ones_like(pos), pos)
    theta = torch.zeros(G, K, n + 1, dtype=torch.float64, device=X.device)
    clip = torch.log(torch.tensor(2.0 * N, dtype=torch.float64, device=X.device))
    theta[..., n] = torch.where(const, torch.where(pos > 0, clip, -clip),
                                torch.log(safe / torch.where(const, torch.ones_like(pos), N - pos)))
    every = torch.ones(N, dtype=torch.bool, device=X.device)

    def at(th):
        r, D, L = _logit_terms(A @ th.transpose(1, 2), bits, every)
        return r, D, L + 0.5 * (pen * th * th).sum(-1), (A.transpose(1, 2) @ r).transpose(1, 2) + pen * th

    r, D, f, g = at(theta)
    g0 = g.norm(dim=-1)
    for _ in range(max_steps):
        live = ~const & (g.norm(dim=-1) > 1e-12 * g0)
        if not bool(live.any()):
            break
        H = (A.unsqueeze(1) * D.transpose(1, 2).unsqueeze(-1)).transpose(2, 3) @ A.unsqueeze(1) + torch.diag(pen)
        H = torch.where(live[..., None, None], H, torch.eye(n + 1, dtype=torch.float64, device=X.device))
        step = torch.linalg.solve(H, -(g * live.unsqueeze(-1)).unsqueeze(-1)).squeeze(-1)
        slope = (g * step).sum(-1)
        moved = torch.zeros_like(live)
        for j in range(40):                                              # backtracking: the first 2^-j that descends
            cand = theta + 2.0 ** -j * step
            ok = live & ~moved & (at(cand)[2] <= f + ARMIJO * 2.0 ** -j * slope)
            theta = torch.where(ok.unsqueeze(-1), cand, theta)
            moved |= ok
        if not bool(moved.any()):
            break
        r, D, f, g = at(theta)
    return theta[..., :n].transpose(1, 2).contiguous(), theta[..., n].contiguous()
