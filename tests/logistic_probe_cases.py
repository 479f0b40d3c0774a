"""Case builders shared by ``test_logistic_probes_cpu.py`` and ``test_logistic_probes_gpu.py``: the margins, flag
words, masks and comparators of the logistic probes (``engine/probe.py``, ``ops/probe.py``, ``csrc/probe.hip``).  The
codes, concepts and the solver case are those of ``probe_cases``.

Saturated exact tier (``saturated``): every margin z is an odd multiple of 1024 and every direction u a multiple of
2^18, so ``z + 2^-j u`` (j <= 7) is an odd multiple of 1024 too.  ``exp(-|z|)`` is then 0 in fp64 (it underflows
below -745), sigma is 0 or 1, D is 0, every loss is 0 or ``|z|``, and every sum is a sum of integers below 2^53: exact
in any order.  Chosen rows of one column hold z = 0, where ``r = +-0.5`` and ``D = 0.25`` exactly (their loss,
log 2, is not an integer: that column's sums are compared within ``sum_bound``).

Realistic tier: margins and directions random fp32 in +-12.  An element is within one fp32 rounding of the fp64
oracle plus ``EVAL_ULPS`` fp64 ulps for the evaluation.  Source of ``EVAL_ULPS``: the device library's fp64 ``exp``
and ``log1p`` are OpenCL-conformant, for which the OpenCL C specification (section "Relative error as ULPs", double
precision) allows 3 ulp and 2 ulp; division is correctly rounded and every other operation adds half an ulp.  ``r``
and ``D`` pass through ``exp`` (3), an addition, a division and at most two multiplications (4 x 0.5): 5 ulp; the
host oracle's own evaluation adds at most 3 (libm ``exp`` within 1 ulp and the same operations): 8.  A loss
``max(z, 0) + log1p(e) - t z`` carries the 3 ulp of ``e`` and 2 of ``log1p`` on a term of at most log 2, and two
additions on terms of at most ``|z|``: within 8 ulp of ``|z| + 1`` with the oracle's share.  The sums add the fp64
accumulation of ``realistic_bound``: ``(length + EVAL_ULPS) 2^-52 sum |terms|`` (an fp64 output has no fp32
rounding)."""

import torch

import probe_cases as C

EVAL_ULPS = 8
ULP64 = 2.0 ** -52
ODD = torch.tensor([-5.0, -3.0, -1.0, 1.0, 3.0, 5.0]) * 1024
ZERO_COL = 1                      # the column of ``saturated`` that holds the z = 0 rows
_CACHE = {}


def _seeded(seed):
    return torch.Generator().manual_seed(int(seed))


def flag_words(N: int, K: int, seed: int) -> torch.Tensor:
    """int32 [N]: random bits 0 .. K - 1 (bit 31 is the sign bit), rows 0 .. 3 all-zero, all-one, alternating."""
    gen = _seeded(seed)
    bits = torch.rand(N, K, generator=gen) < 0.5
    for r, pat in enumerate((0, 1, 2, 3)):
        if r < N:
            bits[r] = torch.tensor([(False, True, k % 2 == 0, k % 2 == 1)[pat] for k in range(K)])
    return C.flags_of(bits)


def fit_mask(N: int, seed: int, slab: int = 0) -> torch.Tensor:
    """uint8 [N]: about three rows in four, with runs of both kinds at the start; ``slab``: rows [slab, 2 slab) are
    masked out whole (a slab that contributes nothing)."""
    m = torch.rand(N, generator=_seeded(seed)) < 0.75
    m[:2], m[2:5] = True, False
    if slab and N >= 2 * slab:
        m[slab:2 * slab] = False
    return m.to(torch.uint8)


def saturated(G: int, N: int, K: int, seed: int, slab: int = 0):
    """(Z fp32 [G, N, 32], U fp32 [G, N, 32], flags int32 [N], mask uint8 [N]); columns at and past K are zero."""
    key = ("sat", G, N, K, seed, slab)
    if key not in _CACHE:
        gen = _seeded(seed)
        Z = torch.zeros(G, N, 32)
        U = torch.zeros(G, N, 32)
        Z[..., :K] = ODD[torch.randint(0, 6, (G, N, K), generator=gen)]
        U[..., :K] = torch.randint(-3, 4, (G, N, K), generator=gen).float() * 2.0 ** 18
        Z[:, ::7, ZERO_COL] = 0.0                                   # z = 0 on fit rows and on masked rows alike
        U[:, ::7, ZERO_COL] = 0.0
        _CACHE[key] = (Z, U, flag_words(N, K, seed + 1), fit_mask(N, seed + 2, slab))
    return _CACHE[key]


def realistic(G: int, N: int, seed: int):
    """The same with random fp32 margins and directions in +-12 in all 32 columns."""
    gen = _seeded(seed)
    Z = (torch.rand(G, N, 32, generator=gen) * 24 - 12)
    U = (torch.rand(G, N, 32, generator=gen) * 24 - 12)
    return Z, U, flag_words(N, 32, seed + 1), fit_mask(N, seed + 2)


def elem_bound(ref64: torch.Tensor) -> torch.Tensor:
    """One fp32 rounding of the fp64 value plus its evaluation allowance."""
    return (2.0 ** -24 + EVAL_ULPS * ULP64) * ref64.abs()


def sum_bound(abs_terms: torch.Tensor, length) -> torch.Tensor:
    """The fp64 accumulation of ``length`` terms whose absolute values sum to ``abs_terms`` (the second term of
    ``probe_cases.realistic_bound``) plus the evaluation allowance of every term."""
    return (length + EVAL_ULPS) * ULP64 * abs_terms


def loss_abs_terms(Z64: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """[G, 32]: sum over the fit rows of ``|z| + 1``, which bounds every loss term and its evaluation error."""
    return ((Z64.abs() + 1) * (mask != 0).view(1, -1, 1)).sum(1)


# ---------------------------------------------------------------------- the definition, in plain dense algebra
def objective(dense, bits, fit, Cinv, w, b):
    """(f, g_w, g_b) fp64 of ``sum_fit softplus(z) - t z + |w|^2 / 2C`` at (w [G, n, K], b [G, K]) by its definition,
    uncentred: ``z = X w + b``, ``g_w = X^T (sigma(z) - t) + w / C``, ``g_b = sum (sigma(z) - t)``."""
    X, t = dense.double(), bits.double()
    if fit is not None:
        X, t = X[:, fit], t[fit]
    w, b = w.double(), b.double()
    z = X @ w + b.unsqueeze(1)
    f = (torch.logaddexp(z, torch.zeros_like(z)) - t * z).sum(1) + 0.5 * Cinv * (w * w).sum(1)
    r = torch.sigmoid(z) - t
    return f, X.transpose(1, 2) @ r + Cinv * w, r.sum(1)


def _row_radius(dense, fit):
    X = dense.double() if fit is None else dense.double()[:, fit]
    return X.pow(2).sum(-1).sqrt().amax(1)                            # [G]: the longest row of every model


def distance_bound(dense, bits, fit, Cc, w, b) -> torch.Tensor:
    """fp64 [G, K]: how far the weights ``w`` can be from the minimiser w*, in the 2-norm, from the gradient at
    (w, b) alone.  With H the Hessian averaged over the segment to the minimiser, blocks ``[[A, c], [c^T, s]]`` for
    (w, b): ``g_w = A dw + c db`` and ``g_b = c^T dw + s db``, so ``dw = S^-1 (g_w - c g_b / s)`` with the Schur
    complement ``S = A - c c^T / s >= I / C`` (the data part is a weighted covariance, the penalty is on w alone: the
    objective is 1/C-strongly convex in w once b is minimised out).  ``c / s`` is a weighted mean of the rows, no
    longer than the longest row R: ``|w - w*| <= C (|g_w| + R |g_b|)``.  With ``g_b = 0`` this is the familiar
    ``C |g|``."""
    _, gw, gb = objective(dense, bits, fit, 1.0 / Cc, w, b)
    return Cc * (gw.pow(2).sum(1).sqrt() + _row_radius(dense, fit).unsqueeze(1) * gb.abs())


def stop_radius(dense, bits, fit, Cc, tol) -> torch.Tensor:
    """fp64 [G, K]: how far from w* an iterate can be that met the stop ``|g| <= tol |g0|`` of the centred
    recurrence (``g0`` the gradient at ``w = 0, b' = log(pos / neg)``, where its intercept part vanishes).  As
    ``distance_bound``, in the centred coordinates, where the rows are ``x_i - mu``: ``|w - w*| <= C (|g_w| + Rc
    |g_b|) <= C sqrt(1 + Rc^2) tol |g0|`` with Rc the longest centred row.  Two converged routes differ by at most
    twice that."""
    X, t = dense.double(), bits.double()
    if fit is not None:
        X, t = X[:, fit], t[fit]
    Xc = X - X.mean(1, keepdim=True)
    g0 = Xc.transpose(1, 2) @ (t.mean(0) - t)                         # sigma(log(pos / neg)) = pos / n
    Rc = Xc.pow(2).sum(-1).sqrt().amax(1).unsqueeze(1)
    return Cc * torch.sqrt(1 + Rc * Rc) * tol * g0.pow(2).sum(1).sqrt()


def weight_gap(w, w_ref) -> torch.Tensor:
    """fp64 [G, K]: the 2-norm of the difference of two weight tensors [G, n, K]."""
    return (w.double().cpu() - w_ref.double().cpu()).pow(2).sum(1).sqrt()


def newton(K: int, Cc: float = 1.0, held: bool = True):
    """``logistic_newton_reference`` on ``solver_case(K)``, computed once: (weight, intercept)."""
    from sparse_coding__amd.engine import probe as pb

    key = ("newton", K, Cc, held)
    if key not in _CACHE:
        dense, bits, fit = C.solver_case(K)
        _CACHE[key] = pb.logistic_newton_reference(dense, bits, Cc, fit if held else None)
    return _CACHE[key]


def overshoot_case():
    """(dense fp32 [1, 48, 4], bits bool [48, 1], C = 1e4): a nearly separable concept under a weak penalty -- signed
    features whose rows have log-normal lengths, labels from a random hyperplane with two rows flipped.  The first
    steps from w = 0 are short (the curvature is largest there), then most rows saturate, the curvature at the
    iterate understates the curvature ahead of it, where the flipped rows wake up, and the full Newton step
    overshoots: the line search takes t = 1/4 on the way, and a solver that always takes t = 1 leaves the basin
    (its objective passes 1e8; found by a search over seeds, this is seed 105)."""
    gen = _seeded(105)
    N, n = 48, 4
    x = torch.randn(N, n, generator=gen) * torch.exp(1.0 * torch.randn(N, 1, generator=gen))
    y = (x @ torch.randn(n, 1, generator=gen)) > 0
    flip = torch.randperm(N, generator=gen)[:2]
    y[flip] = ~y[flip]
    return x.unsqueeze(0), y, 1e4


def same_probes(a, b):
    """Two ``LogisticProbes``: the same bits in every field."""
    a, b = a.to("cpu"), b.to("cpu")
    assert a.n_rows == b.n_rows and a.C == b.C
    for k in a._TENSORS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape, k
        if x.is_floating_point():
            assert torch.equal(x.isnan(), y.isnan()) and torch.equal(x.nan_to_num(), y.nan_to_num()), k
        else:
            assert torch.equal(x, y), k
