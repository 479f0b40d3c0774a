"""Dictionary quality metrics (reference ``standard_metrics.py``).

Every function takes a ``LearnedDict`` and activations ``[B, d]`` (or another
dictionary / ground-truth matrix) and returns tensors, so they run on CPU or
GPU unchanged.  Formulas follow SURVEY.md Appendix A:
``L0 = sum_j mean_b 1[c_bj != 0]`` on ``encode(center(x))`` and
``FVU = mean((x - predict(x))^2) / mean((x - mean_b x)^2)``.
Deliberate fixes of reference defects are tagged "fix B#k".
"""

from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

from ..models.learned_dict import LearnedDict


# ------------------------------------------------------------------ sparsity / reconstruction
def mean_nonzero_activations(model: LearnedDict, batch: torch.Tensor) -> torch.Tensor:
    """Per-feature activation frequency (reference standard_metrics.py:303-306)."""
    c = model.encode(model.center(batch))
    return (c != 0).float().mean(dim=0)


def mean_l0(model: LearnedDict, batch: torch.Tensor) -> torch.Tensor:
    """Average number of active features per row (= sum of ``mean_nonzero_activations``)."""
    return mean_nonzero_activations(model, batch).sum()


def fraction_variance_unexplained(model: LearnedDict, batch: torch.Tensor) -> torch.Tensor:
    """Reference standard_metrics.py:308-312."""
    x_hat = model.predict(batch)
    resid = (batch - x_hat).pow(2).mean()
    total = (batch - batch.mean(dim=0)).pow(2).mean()
    return resid / total


def r_squared(model: LearnedDict, batch: torch.Tensor) -> torch.Tensor:
    return 1.0 - fraction_variance_unexplained(model, batch)


def fraction_variance_unexplained_top_activating(model: LearnedDict, batch: torch.Tensor, n_top: int = 2
                                                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """FVU using only the ``n_top`` most active features vs. the rest (reference :314-340).

    fix B#24: reconstructions are mapped back with ``uncenter`` (the reference applies ``center``).
    """
    c = model.encode(model.center(batch))
    order = torch.argsort(c.mean(dim=0), descending=True)
    top, rest = order[:n_top], order[n_top:]
    c_top = torch.zeros_like(c)
    c_top[:, top] = c[:, top]
    c_rest = torch.zeros_like(c)
    c_rest[:, rest] = c[:, rest]
    var = (batch - batch.mean(dim=0)).pow(2).mean()
    r_top = (batch - model.uncenter(model.decode(c_top))).pow(2).mean()
    r_rest = (batch - model.uncenter(model.decode(c_rest))).pow(2).mean()
    return r_top / var, r_rest / var


def batched_fvu_l0(model: LearnedDict, activations: torch.Tensor, batch_size: int = 8192
                   ) -> Tuple[float, float]:
    """Streaming FVU and L0 over a large activation set without materialising all codes."""
    n = activations.shape[0]
    mean = activations.float().mean(0)
    se = tot = 0.0
    l0 = 0.0
    for i in range(0, n, batch_size):
        x = activations[i:i + batch_size].float()
        c = model.encode(model.center(x))
        x_hat = model.uncenter(model.decode(c))
        se += float((x - x_hat).pow(2).sum())
        tot += float((x - mean).pow(2).sum())
        l0 += float((c != 0).sum())
    return se / tot, l0 / n


# ------------------------------------------------------------------ dictionary similarity
# Above this many similarity entries, GPU max-cosine reductions run on the fused
# EPI_ROWMAX kernel (bf16 MFMA, the [n1, n2] matrix never materialised; 16k x 16k fp32
# would be 1 GiB); below it the exact fp32 torch product is cheap enough.
ROWMAX_MIN_ENTRIES = 1 << 24


def max_cosine(rows: torch.Tensor, against: torch.Tensor, fused: bool | None = None) -> torch.Tensor:
    """max_j <rows_i, against_j> for every row (inputs already unit-norm)."""
    if fused is None:
        fused = rows.is_cuda and rows.shape[0] * against.shape[0] >= ROWMAX_MIN_ENTRIES
    if fused:
        from ..ops import gemm

        return gemm.rowmax_nt(rows.to(torch.bfloat16).contiguous(), against.to(torch.bfloat16).contiguous())
    return (rows @ against.T).max(dim=-1).values


def nearest_atoms(rows: torch.Tensor, against: torch.Tensor, m: int = 1, exclude_self: bool = False,
                  fused: bool | None = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The ``m`` (1..8) nearest atoms of ``against`` [n2, d] for every atom of ``rows`` [n1, d] (inputs
    already unit-norm): (cos fp32 [n1, m], idx int64 [n1, m]), cosine descending; among equal cosines the
    lowest index wins; slots without a candidate read (0.0, -1).  ``exclude_self`` (``rows`` and
    ``against`` the same dictionary): atom i is not its own match.

    ``fused=None`` follows ``max_cosine``: on the GPU from ``ROWMAX_MIN_ENTRIES`` similarity entries on, the
    row-argmax kernel (``ops.gemm.rowargmax_nt``: bf16 MFMA, the matches of the bf16-rounded dictionaries,
    the [n1, n2] matrix never materialised); otherwise the exact fp32 torch product, same tie rule."""
    m = int(m)
    if not 1 <= m <= 8:
        raise ValueError(f"m must be in [1, 8], got {m}")
    n1, n2 = rows.shape[0], against.shape[0]
    if exclude_self and n1 != n2:
        raise ValueError(f"exclude_self needs the same dictionary on both sides, got {n1} and {n2} atoms")
    if fused is None:
        fused = rows.is_cuda and n1 * n2 >= ROWMAX_MIN_ENTRIES
    if fused:
        from ..ops import gemm

        cos, idx = gemm.rowargmax_nt(rows.to(torch.bfloat16).contiguous(), against.to(torch.bfloat16).contiguous(),
                                     m=m, exclude_self=exclude_self)
        return cos, idx.long()
    sim = rows.float() @ against.float().T
    ar = torch.arange(n2, device=sim.device)
    if exclude_self:
        sim.fill_diagonal_(float("-inf"))
    cos = torch.zeros(n1, m, device=sim.device)
    idx = torch.full((n1, m), -1, dtype=torch.int64, device=sim.device)
    for k in range(min(m, n2)):
        mx = sim.max(dim=-1).values
        col = torch.where(sim == mx.unsqueeze(1), ar, n2).amin(dim=-1)  # the lowest index among equal values
        found = mx > float("-inf")
        cos[:, k] = torch.where(found, mx, torch.zeros_like(mx))
        idx[:, k] = torch.where(found, col, torch.full_like(col, -1))
        sim.scatter_(1, col.clamp(max=n2 - 1).unsqueeze(1), float("-inf"))
    return cos, idx


def activation_matches(sc_small, sc_large, m: int = 4, score: str = "pearson", min_both: int = 1):
    """Nearest features by ACTIVATION between two ensembles whose sparse codes ``sc_small`` / ``sc_large``
    (``engine.sparse_codes.SparseCodes`` of the smaller and the larger dictionaries) cover the same rows: an
    ``engine.coactivation.CoActivation`` [G_small, G_large, n_small, m] -- per feature of a smaller dictionary
    the ``m`` features of each larger one that fire on the same rows and score best (``score``: "pearson",
    "cosine" or "jaccard" of their codes).  ``nearest_atoms`` compares the atoms; two close atoms may fire on
    different rows, and a feature that splits keeps modest cosines with partners that fire exactly where it
    does.  The kernels of ``csrc/coactivation.hip`` on a GPU, the torch oracle elsewhere."""
    from ..engine.coactivation import coactivation

    return coactivation(sc_small, sc_large, m=m, score=score, min_both=min_both, exclude_self=False)


def label_selectivity(sparse_codes, labels: torch.Tensor, n_classes: int, m: int = 1, nactive=None):
    """Every feature as a detector of its best label: ``(label int32, precision, recall, f1)``, [G, n] each (fp64
    scores), from the sparse codes of a pool (``engine.sparse_codes.SparseCodes``) and one label per row
    (``labels`` int32 / int64 [n_rows] in [0, ``n_classes``); negative: the row is left out).  Precision is the
    part of the feature's rows that carry the label, recall the part of the label's rows on which the feature
    fires.  The best label is, among the feature's ``m`` most frequent labels, the one with the largest F1 (the
    more frequent one among equals); with ``m`` = 1 it is the most frequent label.  A feature that never fires
    reads ``(-1, 0, 0, 0)``.  From ``engine.label_profile.label_profile``: the kernels of
    ``csrc/label_profile.hip`` on a GPU, the torch oracle elsewhere."""
    from ..engine.label_profile import label_profile

    prof = label_profile(sparse_codes, labels, m=m, rank_by="count", n_classes=n_classes, nactive=nactive)
    p, r, f = prof.precision(), prof.recall(), prof.f1()
    best = f.argmax(-1, keepdim=True)
    pick = lambda t: t.gather(-1, best).squeeze(-1)
    return pick(prof.top_label), pick(p), pick(r), pick(f)


def activation_quantiles(sparse_codes, Q: int, nactive=None) -> torch.Tensor:
    """fp32 [G, n, Q + 1]: quantiles of every feature's activations over the rows on which it fires, from the
    sparse codes of a pool (``engine.sparse_codes.SparseCodes``): entry k is the value at sorted position
    ``(k (L - 1)) // Q`` of the feature's L codes (k = 0 the smallest, k = Q the largest); NaN for a feature
    that never fires.  From ``SparseCodes.by_value``: the segmented sort of ``csrc/value_order.hip`` on a GPU,
    the torch oracle elsewhere."""
    return sparse_codes.by_value(nactive).quantiles(Q)


def feature_auroc(sparse_codes, flags: torch.Tensor, nactive=None, n_concepts=None) -> torch.Tensor:
    """fp64 [G, n, K]: the exact AUROC of every feature's activation as a score for each of K <= 32 concepts over
    all rows of a pool, ties counting half, from its complete sparse codes (``engine.sparse_codes.SparseCodes``).
    ``flags``: int32 words [n_rows] whose bit k marks the positives of concept k (``n_concepts`` of them, default
    32), or a bool [n_rows, K] matrix.  A row on which the feature does not fire scores 0; a feature that never
    fires reads 0.5; a concept with no positive or no negative reads NaN.  The per-feature counterpart of probing
    a whole dictionary with a logistic regression.  From ``engine.value_order.feature_auroc``: the kernels of
    ``csrc/value_order.hip`` on a GPU, the torch oracle elsewhere."""
    from ..engine.value_order import feature_auroc as route

    return route(sparse_codes, flags, n_concepts, nactive).auroc()


def ablation_effects(sparse_codes, D: torch.Tensor, x: torch.Tensor, nactive=None):
    """``(delta_sse, delta_fvu)``, fp64 [G, n] each: the exact rise of the summed squared error, and of the FVU,
    when feature f of model g alone is removed from the reconstruction of the rows ``x`` ([n_rows, d] shared or
    [G, n_rows, d], as the decoder sees them) from the sparse codes of a pool (``engine.sparse_codes.
    SparseCodes``) and the unit-norm dictionaries ``D`` [G, n, d] -- leave-one-out for all G n features from one
    pass.  A feature that never fires reads 0; a negative value marks a feature the reconstruction is better
    without.  From ``engine.attribution.attribution``: the kernels of ``csrc/attribution.hip`` on a GPU, the
    torch oracle elsewhere."""
    from ..engine.attribution import attribution

    attr = attribution(sparse_codes, D, x, nactive)
    return attr.delta_sse, attr.delta_fvu


def feature_shrinkage(sparse_codes, D: torch.Tensor, x: torch.Tensor, nactive=None) -> torch.Tensor:
    """fp64 [G, n]: the least-squares rescale of every feature's codes -- the factor that, applied to all codes of
    feature f alone, lowers the squared error most.  L1-trained SAEs shrink their codes: values above 1 measure
    by how much.  0 for a feature that never fires.  Arguments and routes as ``ablation_effects``."""
    from ..engine.attribution import attribution

    return attribution(sparse_codes, D, x, nactive).rescale


def mutual_nearest(a: torch.Tensor, b: torch.Tensor, fused: bool | None = None
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The pairs (i, j) with b_j the nearest atom of a_i and a_i the nearest atom of b_j: (ia, ib, cos),
    one-to-one by construction and ordered by ``ia``; ``cos`` is <a_i, b_j> as seen from ``a``."""
    ca, ab = nearest_atoms(a, b, fused=fused)
    _, ba = nearest_atoms(b, a, fused=fused)
    ab, ba = ab[:, 0], ba[:, 0]
    ia = torch.arange(a.shape[0], device=ab.device)
    keep = (ab >= 0) & (ba[ab.clamp(min=0)] == ia)
    return ia[keep], ab[keep], ca[keep, 0]


def duplicate_atoms(rows: torch.Tensor, threshold: float = 0.9, fused: bool | None = None
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Atoms whose nearest *other* atom of the same dictionary is at or above ``threshold``: (i, j, cos)
    with j the nearest other atom of atom i, ordered by i."""
    cos, idx = nearest_atoms(rows, rows, exclude_self=True, fused=fused)
    cos, idx = cos[:, 0], idx[:, 0]
    keep = (idx >= 0) & (cos >= threshold)
    return torch.arange(rows.shape[0], device=idx.device)[keep], idx[keep], cos[keep]


def mcs_duplicates(ground: LearnedDict, model: LearnedDict) -> torch.Tensor:
    """Max cosine similarity of each ``model`` atom to the ``ground`` atoms (reference :268-272)."""
    return max_cosine(model.get_learned_dict(), ground.get_learned_dict())


def mmcs(model: LearnedDict, model2: LearnedDict) -> torch.Tensor:
    return mcs_duplicates(model, model2).mean()


def mcs_to_fixed(model: LearnedDict, truth: torch.Tensor) -> torch.Tensor:
    return max_cosine(model.get_learned_dict(), truth)


def mmcs_to_fixed(model: LearnedDict, truth: torch.Tensor) -> torch.Tensor:
    return mcs_to_fixed(model, truth).mean()


def mmcs_from_list(ld_list: Sequence[LearnedDict]) -> torch.Tensor:
    """Symmetric matrix of pairwise MMCS (reference :285-296)."""
    k = len(ld_list)
    out = torch.eye(k)
    for i in range(k):
        for j in range(i):
            out[i, j] = out[j, i] = float(mmcs(ld_list[i], ld_list[j]))
    return out


def representedness(features: torch.Tensor, model: LearnedDict) -> torch.Tensor:
    """For each ground-truth feature, max cosine similarity to any learned atom (reference :298-301)."""
    return (features @ model.get_learned_dict().T).max(dim=-1).values


def hungarian_mmcs(a: LearnedDict, b: LearnedDict) -> float:
    """Mean cosine similarity under the optimal one-to-one atom matching (reference :809-840)."""
    from scipy.optimize import linear_sum_assignment

    sim = (a.get_learned_dict() @ b.get_learned_dict().T).detach().float().cpu().numpy()
    r, c = linear_sum_assignment(-sim)
    return float(sim[r, c].mean())


# ------------------------------------------------------------------ dictionary geometry
def neurons_per_feature(model: LearnedDict) -> torch.Tensor:
    """Simpson-diversity count of neurons each atom uses (reference :345-350)."""
    D = model.get_learned_dict()
    p = D / D.abs().sum(dim=-1, keepdim=True)
    return (1.0 / p.pow(2).sum(dim=-1)).mean()


def capacity_per_feature(model: LearnedDict) -> torch.Tensor:
    """Capacity of Scherlis et al. 2022 (reference :354-360)."""
    D = model.get_learned_dict()
    sq = (D @ D.T).pow(2)
    return torch.diagonal(sq) / sq.sum(dim=-1)


def capacity_per_feature_lowrank(D: torch.Tensor, live=None) -> torch.Tensor:
    """``capacity_per_feature`` without the [n, n] matrix, in fp64: for the dictionary ``D`` [n, d] or a
    stack [G, n, d], ``sum_j (d_i . d_j)^2 = d_i^T (D^T D) d_i``, so with ``M = D^T D`` [d, d] and
    ``q = ((D M) * D).sum(-1)`` the capacity is ``(d_i . d_i)^2 / q`` -- n d^2 operations instead of n^2 d.
    ``live``: the number of atoms that exist (an int, or one count per model of a stack): atoms at or
    past it take no part and read 0, as does an all-zero atom.  Never synchronises."""
    Dd = D.detach().double()
    if live is not None:
        n = Dd.shape[-2]
        lv = torch.as_tensor(live, device=Dd.device).reshape(-1, 1) if Dd.dim() == 3 \
            else torch.as_tensor(live, device=Dd.device).reshape(())
        keep = torch.arange(n, device=Dd.device) < lv
        Dd = Dd * keep.unsqueeze(-1)
    M = Dd.transpose(-1, -2) @ Dd
    q = ((Dd @ M) * Dd).sum(-1)
    self2 = (Dd * Dd).sum(-1) ** 2
    return torch.where(q > 0, self2 / q.clamp(min=torch.finfo(torch.float64).tiny), torch.zeros_like(q))


def calc_expected_interference(dictionary: torch.Tensor, batch: torch.Tensor) -> torch.Tensor:
    """Activity-weighted capacity of Scherlis et al. 2022 on dense tensors (reference big_sweep.py:44-58):
    ``dictionary`` [n, d], ``batch`` [B, n] codes.  With the atoms normalised (norms clamped at 1e-8),
    ``totals[b, i] = sum_j cos^2(i, j) batch[b, j]`` and ``capacities = batch / clamp(totals, 1e-8)``; the
    result [n] is the per-feature sum of the capacities over the rows, divided by the number of rows on
    which the feature is non-zero (clamped at 1)."""
    normed = dictionary / torch.clamp(torch.linalg.vector_norm(dictionary, dim=-1), min=1e-8).unsqueeze(-1)
    cos2 = (normed @ normed.T) ** 2
    totals = batch @ cos2.T
    capacities = batch / torch.clamp(totals, min=1e-8)
    fired = torch.count_nonzero(batch, dim=0).to(capacities.dtype)
    return capacities.sum(dim=0) / torch.clamp(fired, min=1.0)


def expected_interference(sparse_codes, D: torch.Tensor, nactive=None):
    """``calc_expected_interference`` for every model of an ensemble from its sparse codes: an
    ``engine.interference.Interference`` of ``sparse_codes`` (``engine.sparse_codes.SparseCodes``) against
    the dictionaries ``D`` [G, n, d]; ``.expected`` [G, n] is the metric, ``.capacity`` the static
    capacity.  ``nactive``: live atoms per model of a masked ensemble.  bf16 dictionaries on the GPU run
    the ``active_capacity`` kernel (a missing kernel library is an error); anything else runs the fp64
    torch oracle."""
    from ..engine import interference as ic

    if D.is_cuda and D.dtype == torch.bfloat16:
        return ic.interference_fused(sparse_codes, D.contiguous(), nactive)
    ref = ic.active_capacity_reference(sparse_codes, D, nactive)
    live = ic.live_counts(nactive, D.shape[0], D.shape[1], D.device)
    return ic.Interference(sparse_codes.n_rows, ref.qsum, ref.count, ref.skipped,
                           capacity_per_feature_lowrank(D, live))


def truncated_fvu(sparse_codes, D: torch.Tensor, x: torch.Tensor, max_kept: int = 32, keep=None, nactive=None):
    """FVU of every model of an ensemble when only the j largest codes of every row are kept, j = 0 ..
    ``max_kept``, from its sparse codes: an ``engine.sparse_recon.ReconProfile`` of ``sparse_codes``
    (``engine.sparse_codes.SparseCodes``) against the unit-norm dictionaries ``D`` [G, n, d] and the rows
    ``x`` the decoder sees ([N, d] shared or [G, N, d]); ``.fvu_prefix`` [G, J + 1] is the curve,
    ``.fvu_full`` the FVU from all codes and, with ``keep`` (bool [G, n] or ``keep_words``), ``.fvu_keep`` /
    ``.fvu_rest`` the FVU from the kept features and from the others.  ``nactive``: live atoms per model of a
    masked ensemble.  bf16 dictionaries and rows on the GPU run the ``recon_curve`` / ``recon_split``
    kernels (a missing kernel library is an error); anything else runs the fp64 torch oracle."""
    from ..engine import sparse_recon as sr

    if D.is_cuda and D.dtype == torch.bfloat16 and x.dtype == torch.bfloat16:
        return sr.recon_profile_fused(sparse_codes, D.contiguous(), [x.to(D.device).contiguous()], max_kept, keep,
                                      nactive)
    return sr.recon_profile_reference(sparse_codes, D, x, max_kept, keep, nactive)


def ensemble_fvu_top_activating(engine_or_trainer, activations: torch.Tensor, n_top: int = 2):
    """``fraction_variance_unexplained_top_activating`` for every model of an ensemble: ``engine_or_trainer``
    is a fused engine or an ``EnsembleTrainer`` (anything with ``fvu_top_activating`` and ``batch_size``).
    The activations are trimmed to a multiple of the batch size.  Returns (rows used, fvu_top [G],
    fvu_rest [G])."""
    B = int(getattr(getattr(engine_or_trainer, "impl", None), "batch_size", engine_or_trainer.batch_size))
    N = activations.shape[0] - activations.shape[0] % B
    if N == 0:
        raise ValueError(f"need at least {B} rows")
    top, rest = engine_or_trainer.fvu_top_activating(activations[:N], n_top)
    return N, top, rest


# ------------------------------------------------------------------ activity statistics
def calc_feature_n_active(codes: torch.Tensor) -> torch.Tensor:
    return (codes != 0).sum(dim=0)


def batched_calc_feature_n_ever_active(learned_dict: LearnedDict, activations: torch.Tensor,
                                       batch_size: int = 1000, threshold: int = 10) -> int:
    """Number of features active more than ``threshold`` times (reference :444-452)."""
    counts = torch.zeros(learned_dict.n_feats, device=activations.device)
    for i in range(0, len(activations), batch_size):
        counts += calc_feature_n_active(learned_dict.encode(activations[i:i + batch_size]))
    return int((counts > threshold).sum())


def calc_feature_mean(codes):
    return codes.mean(dim=0)


def calc_feature_variance(codes):
    return codes.var(dim=0)


def calc_feature_skew(codes):
    var = codes.var(dim=0)
    return (codes ** 3).mean(dim=0) / torch.clamp(var ** 1.5, min=1e-8)


def calc_feature_kurtosis(codes):
    var = codes.var(dim=0)
    return (codes ** 4).mean(dim=0) / torch.clamp(var ** 2, min=1e-8)


def calc_moments_streaming(learned_dict: LearnedDict, activations: torch.Tensor, batch_size: int = 1000):
    """Streaming raw moments of every feature's activation (reference :454-509).

    fix B#25: a partial last batch is weighted by its true size and ``times_active`` counts
    samples (rows where the feature fired), not batches.
    Returns (times_active, mean, var, skew, kurtosis, m4).
    """
    nf = learned_dict.n_feats
    dev = activations.device
    times_active = torch.zeros(nf, device=dev)
    s1 = torch.zeros(nf, device=dev, dtype=torch.float64)
    s2 = torch.zeros_like(s1)
    s3 = torch.zeros_like(s1)
    s4 = torch.zeros_like(s1)
    n = 0
    for i in range(0, len(activations), batch_size):
        c = learned_dict.encode(activations[i:i + batch_size]).double()
        times_active += (c != 0).sum(0).float()
        s1 += c.sum(0)
        s2 += (c ** 2).sum(0)
        s3 += (c ** 3).sum(0)
        s4 += (c ** 4).sum(0)
        n += c.shape[0]
    mean, m2, m3, m4 = s1 / n, s2 / n, s3 / n, s4 / n
    var = m2 - mean ** 2
    skew = m3 / torch.clamp(var ** 1.5, min=1e-8)
    kurt = m4 / torch.clamp(var ** 2, min=1e-8)
    f = lambda t: t.float()
    return times_active, f(mean), f(var), f(skew), f(kurt), f(m4)


def ensemble_moments_streaming(engine_or_trainer, activations: torch.Tensor):
    """``calc_moments_streaming`` for every model of an ensemble in one pass: ``engine_or_trainer`` is a
    ``FusedSAEEnsemble`` or an ``EnsembleTrainer`` (anything with ``feature_stats`` and ``batch_size``).
    The activations are trimmed to a multiple of the batch size.  Returns (rows used, one
    (times_active, mean, var, skew, kurtosis, m4) tuple per model)."""
    # (a sharded trainer's engine works on the gathered global batch)
    B = int(getattr(getattr(engine_or_trainer, "impl", None), "batch_size", engine_or_trainer.batch_size))
    N =activations.shape[0] - activations.shape[0] % B
    if N == 0:
        raise ValueError(f"need at least {B} rows")
    stats = engine_or_trainer.feature_stats(activations[:N])
    return N, [stats.per_model(g) for g in range(stats.count.shape[0])]


def ridge_regression_auroc(activations: torch.Tensor, labels: torch.Tensor, **kwargs) -> float:
    """Linear-probe AUROC (reference :252-258)."""
    from sklearn import metrics as skm
    from sklearn.linear_model import RidgeClassifier

    X, y = activations.detach().cpu().numpy(), labels.detach().cpu().numpy()
    clf = RidgeClassifier(**kwargs).fit(X, y)
    return float(skm.roc_auc_score(y, clf.predict(X)))


def ridge_probe_auroc(sparse_codes, flags: torch.Tensor, nactive=None, n_concepts=None, **kw) -> torch.Tensor:
    """fp64 [G, K]: the exact AUROC, ties counting half, of a ridge probe on the whole code of every model for each
    of K <= 32 concepts, over the rows the probe was fitted on, from the complete sparse codes of a pool
    (``engine.sparse_codes.SparseCodes``).  ``flags``: int32 words [n_rows] whose bit k marks the positives of
    concept k (``n_concepts`` of them, default 32), or a bool [n_rows, K] matrix; ``kw``: ``alpha``, ``fit_rows``,
    ``max_iter``, ``tol``.  A concept with no positive or no negative reads NaN.  The whole-dictionary counterpart
    of ``feature_auroc``.  From ``engine.probe.ridge_probes``: the kernels of ``csrc/probe.hip`` on a GPU, the torch
    oracle elsewhere; its ``LinearProbes`` also holds the weights and the held-out AUROC."""
    from ..engine.probe import ridge_probes

    return ridge_probes(sparse_codes, flags, n_concepts, nactive=nactive, **kw).auroc()


def ensemble_ridge_regression_auroc(engine, activations: torch.Tensor, labels: torch.Tensor, **kw) -> torch.Tensor:
    """``ridge_regression_auroc`` for a whole ensemble, on the device: fp64 [G] (``labels`` [N], one concept) or
    [G, K] (``labels`` [N, K]) -- the AUROC of the hard predictions of ``RidgeClassifier(alpha)`` fitted on the
    codes of every model of ``engine`` (a fused engine or an ``EnsembleTrainer``) on ``activations`` [N, d], which
    is their balanced accuracy (reference :252-258 scores ``clf.predict``).  ``labels``: bool, or numbers with
    positives > 0.  ``kw``: ``alpha``, ``max_iter``, ``tol``, ``budget``."""
    labels = labels if labels.dtype == torch.bool else labels > 0
    one = labels.dim() == 1
    out = engine.ridge_probes(activations, labels.unsqueeze(1) if one else labels, **kw).auroc_predicted()
    return out[:, 0] if one else out


def logistic_probe_auroc(sparse_codes, flags: torch.Tensor, nactive=None, n_concepts=None, **kw) -> torch.Tensor:
    """fp64 [G, K]: the exact AUROC, ties counting half, of the logits of a logistic-regression probe on the whole
    code of every model for each of K <= 32 concepts, over the rows the probe was fitted on, from the complete
    sparse codes of a pool (``engine.sparse_codes.SparseCodes``) -- ``roc_auc_score(y, clf.predict_proba(X)[:, 1])``
    of ``LogisticRegression(C=C)``, sigma being monotone.  ``flags`` as in ``ridge_probe_auroc``; ``kw``: ``C``,
    ``fit_rows``, ``max_iter``, ``cg_iter``, ``tol``, ``early_stop``.  From ``engine.probe.logistic_probes``: the
    kernels of ``csrc/probe.hip`` on a GPU, the torch oracle elsewhere."""
    from ..engine.probe import logistic_probes

    return logistic_probes(sparse_codes, flags, n_concepts, nactive=nactive, **kw).auroc()


def ensemble_logistic_regression_auroc(engine, activations: torch.Tensor, labels: torch.Tensor,
                                       **kw) -> torch.Tensor:
    """``logistic_regression_auroc`` for a whole ensemble, on the device: fp64 [G] (``labels`` [N], one concept) or
    [G, K] (``labels`` [N, K]) -- the AUROC of the predicted probabilities of ``LogisticRegression(C=C)`` fitted
    on the codes of every model of ``engine`` (a fused engine or an ``EnsembleTrainer``) on ``activations``
    [N, d], ranked exactly through the logits.  ``labels``: bool, or numbers with positives > 0.  ``kw``: ``C``,
    ``max_iter``, ``cg_iter``, ``tol``, ``early_stop``, ``budget``."""
    labels = labels if labels.dtype == torch.bool else labels > 0
    one = labels.dim() == 1
    out = engine.logistic_probes(activations, labels.unsqueeze(1) if one else labels, **kw).auroc()
    return out[:, 0] if one else out


def cluster_vectors(learned_dict: LearnedDict, n_clusters: int = 100, top_clusters: int = 10,
                    seed: int = 0) -> List[List[int]]:
    """K-means over dictionary atoms; returns the feature indices of the largest clusters
    (reference standard_metrics.py:532-577, without the plotting)."""
    from sklearn.cluster import KMeans

    D = learned_dict.get_learned_dict().detach().float().cpu().numpy()
    km = KMeans(n_clusters=min(n_clusters, D.shape[0]), n_init=3, random_state=seed).fit(D)
    labels = km.labels_
    sizes = np.bincount(labels)
    order = np.argsort(-sizes)[:top_clusters]
    return [np.nonzero(labels == k)[0].tolist() for k in order]
