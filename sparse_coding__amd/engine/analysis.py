"""The analyses on top of ``encode_sparse``, written once for every engine that has sparse codes.

``CodeAnalyses`` is a mixin: ``interference``, ``recon_profile``, ``feature_examples``, ``coactivation``,
``label_profile``, ``value_order``, ``feature_auroc``, ``ridge_probes``, ``logistic_probes``, ``attribution``,
``fvu_top_activating`` and ``atom_matches`` are each one composition of ``encode_sparse`` with the route of its module
(``engine/interference.py`` .. ``engine/atom_match.py``).  A
provider keeps what really differs between engines:

* ``encode_sparse(rows, *, budget=None)`` and ``feature_stats(rows, ...)``: its own loops over the pool;
* ``_analysis_refusal(what)``: raises ``NotImplementedError(f"{what}: {why}")`` for a kind of model the
  analyses do not cover, or returns -- the first thing every analysis does;
* ``_dictionaries()``: the ``[G, n, d]`` unit-norm dictionaries the decoder reads;
* ``_live_counts()``: the live atoms per model of a masked ensemble, or ``None``;
* ``_decoder_batches(rows)``: the rows as the decoder sees them, in the order of the CSR's rows;
* ``_kernels``: which half of each ``*_fused`` / ``*_reference`` pair runs.

The providers: ``FusedSAEEnsemble`` and ``FusedTopKEnsemble`` (the kernels, on their bf16 shadows) and
``TorchCodeAnalyses`` below, the analytic / eager engines' fp32 torch route (the oracles, on any device).
``EnsembleTrainer`` forwards to whichever its engine is.
"""

from __future__ import annotations

from functools import cached_property
from typing import Optional

import torch


class CodeAnalyses:
    _kernels = True  # the kernel routes (``*_fused``); False: the torch oracles (``*_reference``)

    # ------------------------------------------------------------------ what a provider supplies
    def _analysis_refusal(self, what: str) -> None:
        """Raise ``NotImplementedError(f"{what}: {why}")`` if this provider's models are not covered."""

    def _dictionaries(self) -> torch.Tensor:
        raise NotImplementedError

    def _live_counts(self):
        return None

    def _decoder_batches(self, rows: torch.Tensor):
        raise NotImplementedError

    def _check_rows(self, rows: torch.Tensor, what: str) -> int:
        if rows.dim() != 2 or rows.shape[1] != self.d:
            raise ValueError(f"rows must be [N, {self.d}], got {tuple(rows.shape)}")
        N = rows.shape[0]
        if N <= 0 or N % self.batch_size:
            raise ValueError(f"{what} needs a positive multiple of the batch size ({self.batch_size}) rows, got {N}")
        return N

    def _decoder_rows(self, rows: torch.Tensor) -> torch.Tensor:
        """``_decoder_batches(rows)`` as one tensor: the oracles take the pool whole."""
        batches = list(self._decoder_batches(rows))
        return batches[0] if len(batches) == 1 else torch.cat(batches, dim=-2)

    # ------------------------------------------------------------------ the analyses
    @torch.no_grad()
    def interference(self, rows: torch.Tensor, *, budget: Optional[int] = None, state=None):
        """Expected interference of every feature of every model on ``rows`` [N, d] (N a positive multiple
        of the batch size): an ``engine.interference.Interference`` whose ``expected`` [G, n] is the
        activity-weighted capacity ``c_a / sum_b cos^2(a, b) c_b`` averaged over the rows on which the
        feature fires (``eval.metrics.calc_expected_interference``), and ``capacity`` the static capacity.

        ``encode_sparse(rows, budget=budget)`` under its budget contract (``budget=int`` never
        synchronises, ``None`` synchronises once), then ONE ``active_capacity`` launch over the result
        (``csrc/interference.hip``) against the unit-norm bf16 shadow that ``atom_matches`` reads: the
        cosines are those of the bf16-rounded dictionaries.  With a ``budget`` that is too small the rows
        whose entries were dropped are left out and counted in ``skipped`` (``check()`` raises).
        ``state``: the result of an earlier call to continue -- integer sums: chunk by chunk gives the
        bits of one call on the whole pool.  Masked ensembles: atoms at or past ``dict_size[g]`` take no
        part.  Parameters, moments, shadows, ``feature_counts``, ``rows_seen``, the step counter and
        captured graphs are left as they are."""
        from . import interference as ic

        self._analysis_refusal("interference")
        if state is not None:
            ic.check_state(state, self.n_models, self.n)
        codes = self.encode_sparse(rows, budget=budget)
        route = ic.interference_fused if self._kernels else ic.interference_reference
        return route(codes, self._dictionaries(), self._live_counts(), state)

    @torch.no_grad()
    def recon_profile(self, rows: torch.Tensor, *, max_kept: int = 32, keep=None, budget: Optional[int] = None,
                      state=None):
        """Truncated and ablated reconstruction error of every model on ``rows`` [N, d] (N a positive
        multiple of the batch size): an ``engine.sparse_recon.ReconProfile`` whose ``fvu_prefix`` [G, J + 1]
        is the FVU when only the j largest codes of every row are kept (j = 0 .. ``max_kept`` <= 64; equal
        codes go to the lower feature index), ``fvu_full`` the FVU from all codes and -- with ``keep``, a
        bool [G, n] feature mask or its ``keep_words`` -- ``fvu_keep`` / ``fvu_rest`` the FVU from the kept
        features' codes and from the others'.

        ``encode_sparse(rows, budget=budget)`` under its budget contract, then per batch ``prepare()``, one
        ``recon_curve`` and one ``recon_split`` launch on the batch's row window (``csrc/sparse_recon.hip``)
        against the unit-norm bf16 shadow that ``interference`` reads, and the variance bookkeeping of
        ``evaluate()``; the per-row values are summed in fp64.  With a ``budget`` that is too small the rows
        whose entries were dropped are left out and counted in ``skipped`` (``check()`` raises).  ``state``:
        the result of an earlier call to continue -- chunk by chunk gives the bits of one call on the whole
        pool.  Tied models with a fixed affine centering are measured in the centred space, as
        ``evaluate()``.  Parameters, moments, shadows, ``feature_counts``, ``rows_seen``, the step counter
        and captured graphs are left as they are."""
        from . import sparse_recon as sr

        self._analysis_refusal("recon_profile")
        J = sr.check_max_kept(max_kept)
        if state is not None:
            sr.check_state(state, self.n_models, J, keep is not None, self.d)
        codes = self.encode_sparse(rows, budget=budget)
        D, live = self._dictionaries(), self._live_counts()
        if self._kernels:
            return sr.recon_profile_fused(codes, D, self._decoder_batches(rows), J, keep, live, state)
        return sr.recon_profile_reference(codes.to(D.device), D, self._decoder_rows(rows), J, keep, live, state)

    @torch.no_grad()
    def feature_examples(self, rows: torch.Tensor, fragment_len: int = 64, n_top: int = 20, n_random: int = 20,
                         seed: int = 0, budget: Optional[int] = None):
        """Feature-major codes and example fragments of every feature of every model on ``rows`` [N, d] (N a
        positive multiple of the batch size and of ``fragment_len``; row i is token ``i % fragment_len`` of
        fragment ``i // fragment_len``): an ``engine.feature_codes.FeatureCodes`` and its ``FragmentExamples``
        -- per feature the ``n_top`` fragments with the largest maximum code (ties to the lower fragment) and
        a hash sample of ``n_random`` fragments on which it fires (both in 0..32).

        ``encode_sparse(rows, budget=budget)`` under its budget contract, then the transposition and one walk
        over every feature's list (``csrc/feature_codes.hip``); no dense codes.  With a ``budget`` that is too
        small the rows whose entries were dropped are left out whole and counted in ``skipped`` (``check()``
        raises).  Masked ensembles: features at or past ``dict_size[g]`` have empty lists.  Parameters,
        moments, shadows, ``feature_counts``, ``rows_seen``, the step counter and captured graphs are left as
        they are."""
        from . import feature_codes as fc

        self._analysis_refusal("feature_examples")
        fc.check_fragments(rows.shape[0], fragment_len)
        codes = self.encode_sparse(rows, budget=budget)
        if self._kernels:
            return fc.feature_examples(codes, self._live_counts(), fragment_len, n_top, n_random, seed)
        feats = fc.feature_codes_reference(codes, self._live_counts())
        return feats, fc.fragment_examples_reference(feats, fragment_len, n_top, n_random, seed)

    @torch.no_grad()
    def coactivation(self, rows: torch.Tensor, *, m: int = 4, score: str = "pearson", min_both: int = 1,
                     budget: Optional[int] = None):
        """Co-activation partners across the models of the ensemble on ``rows`` [N, d] (N a positive multiple of
        the batch size): an ``engine.coactivation.CoActivation`` holding, for every ordered pair (g, h), the
        ``m`` (0..32) features of model h that fire with each feature of model g on at least ``min_both`` rows
        and score best (``score``: "pearson", "cosine" or "jaccard" of their codes; for g == h the best *other*
        features): what the atoms alone cannot tell -- feature splitting, or two close atoms that fire on
        different rows.

        ``encode_sparse(rows, budget=budget)`` under its budget contract, then the transposition, the list
        moments and one walk per (feature, model) over the feature's list (``csrc/coactivation.hip``); no dense
        codes and no [n, n] matrix.  With a ``budget`` that is too small the rows whose entries were dropped are
        left out whole and counted in ``skipped_a`` / ``skipped_b`` (``check()`` raises).  Masked ensembles:
        features at or past ``dict_size[g]`` have no partners and are nobody's.  There is no ``state=``: the m
        best of a sum cannot be merged across chunks, so the pool is given whole.  Parameters, moments,
        shadows, ``feature_counts``, ``rows_seen``, the step counter and captured graphs are left as they are."""
        from . import coactivation as co

        self._analysis_refusal("coactivation")
        codes = self.encode_sparse(rows, budget=budget)
        route = co.coactivation if self._kernels else co.coactivation_reference
        return route(codes, m=m, score=score, min_both=min_both, nactive_a=self._live_counts())

    @torch.no_grad()
    def label_profile(self, rows: torch.Tensor, labels: torch.Tensor, *, budget: Optional[int] = None, **kw):
        """Per feature of every model the labels that carry its activations on ``rows`` [N, d] (N a positive
        multiple of the batch size): an ``engine.label_profile.LabelProfile``.  ``labels`` int32 / int64 [N]
        gives every row a label -- its token id, its position, a concept flag; a negative one leaves the row out
        -- and the profile holds per feature its ``m`` best labels by ``rank_by`` with their counts, fp64 sums
        and maxima, and the totals that turn them into shares, precision and recall (keywords ``m``,
        ``rank_by``, ``n_classes`` of ``engine.label_profile.label_profile``).

        ``encode_sparse(rows, budget=budget)`` under its budget contract, the kept rows gathered in label order
        (``SparseCodes.take_rows``), the transposition and one walk per feature list
        (``csrc/label_profile.hip``); no dense codes and no global sort of the entries.  The codes must be
        complete: a ``budget`` that is too small raises ``SparseCodesOverflow``.  Masked ensembles: features at
        or past ``dict_size[g]`` have empty profiles.  Parameters, moments, shadows, ``feature_counts``,
        ``rows_seen``, the step counter and captured graphs are left as they are."""
        from . import label_profile as lp

        self._analysis_refusal("label_profile")
        codes = self.encode_sparse(rows, budget=budget)
        route = lp.label_profile if self._kernels else lp.label_profile_reference
        return route(codes, labels, nactive=self._live_counts(), **kw)

    @torch.no_grad()
    def value_order(self, rows: torch.Tensor, *, budget: Optional[int] = None):
        """Every feature's activations on ``rows`` [N, d] (N a positive multiple of the batch size) in value
        order: an ``engine.value_order.ValueOrdered`` -- per model and feature the rows on which it fires with
        their codes, smallest code first -- whose ``quantiles(Q)``, ``histogram(edges)`` and
        ``strata(n_strata, per_stratum)`` say how the activations are distributed and which rows are typical of
        every range, by index arithmetic on the device.

        ``encode_sparse(rows, budget=budget)`` under its budget contract, then the transposition and one
        segmented sort, one wave per list (``csrc/value_order.hip``); no dense codes and no global sort of the
        entries.  With a ``budget`` that is too small the rows whose entries were dropped are left out whole and
        counted in ``skipped`` (``check()`` raises).  Masked ensembles: features at or past ``dict_size[g]`` have
        empty lists, so their quantiles are NaN.  There is no ``state=``: an order cannot be merged across
        chunks, so the pool is given whole.  Parameters, moments, shadows, ``feature_counts``, ``rows_seen``,
        the step counter and captured graphs are left as they are."""
        from . import value_order as vo

        self._analysis_refusal("value_order")
        codes = self.encode_sparse(rows, budget=budget)
        return vo.value_order(codes, self._live_counts(), kernels=self._kernels)

    @torch.no_grad()
    def feature_auroc(self, rows: torch.Tensor, flags: torch.Tensor, *, n_concepts: Optional[int] = None,
                      budget: Optional[int] = None):
        """How well every feature of every model detects each of up to 32 concepts on ``rows`` [N, d] (N a
        positive multiple of the batch size), thresholded at any level: an ``engine.value_order.FeatureAuroc``
        whose ``auroc()`` [G, n, K] is the exact AUROC of the feature's code as a score for the concept, ties
        counting half, and ``best(m)`` the m best features per concept.  ``flags``: int32 words [N], bit k set
        where the row is a positive of concept k (``n_concepts`` of them, default 32), or a bool [N, K] matrix.
        Every row counts; a row on which the feature does not fire scores 0.

        ``encode_sparse(rows, budget=budget)`` under its budget contract, the transposition, the segmented sort
        and one walk per value-ordered list with integer sums (``csrc/value_order.hip``).  The codes must be
        complete: a ``budget`` that is too small raises ``SparseCodesOverflow``.  Masked ensembles: features at
        or past ``dict_size[g]`` have empty lists and read exactly 0.5.  There is no ``state=``.  Parameters,
        moments, shadows, ``feature_counts``, ``rows_seen``, the step counter and captured graphs are left as
        they are."""
        from . import value_order as vo

        self._analysis_refusal("feature_auroc")
        codes = self.encode_sparse(rows, budget=budget)
        return vo.feature_auroc(codes, flags, n_concepts, self._live_counts(), kernels=self._kernels)

    @torch.no_grad()
    def ridge_probes(self, rows: torch.Tensor, flags: torch.Tensor, *, n_concepts: Optional[int] = None,
                     alpha: float = 1.0, fit_rows: Optional[torch.Tensor] = None, max_iter: int = 64,
                     tol: float = 1e-5, budget: Optional[int] = None):
        """Is each of up to 32 concepts linearly readable from the code of every model as a whole on ``rows``
        [N, d] (N a positive multiple of the batch size), and which features carry it: an
        ``engine.probe.LinearProbes`` -- exactly ``RidgeClassifier(alpha)`` per (model, concept), the reference's
        whole-dictionary probe (``ridge_regression_auroc``) for the whole ensemble -- with ``weight`` [G, n, K],
        ``intercept``, ``auroc()`` / ``auroc_heldout()`` (exact, ties counting half), ``auroc_predicted()`` (the
        reference's number) and ``top_features(m)``.  ``flags``: int32 words [N], bit k set where the row is a
        positive of concept k (``n_concepts`` of them, default 32), or a bool [N, K] matrix.  ``fit_rows``: bool
        [N], the rows the fit sees (default all); the others are held out and only scored.

        ``encode_sparse(rows, budget=budget)`` under its budget contract, the transposition, then CGLS for all
        models and concepts in lockstep: per iteration one product over the CSR rows and one over the feature
        lists, 32 right-hand sides each, with fp64 sums (``csrc/probe.hip``); no dense codes, and the loop reads
        nothing to the host.  The codes must be complete: a ``budget`` that is too small raises
        ``SparseCodesOverflow``.  Masked ensembles: features at or past ``dict_size[g]`` have weight 0.  There is
        no ``state=``.  Parameters, moments, shadows, ``feature_counts``, ``rows_seen``, the step counter and
        captured graphs are left as they are."""
        from . import probe as pb

        self._analysis_refusal("ridge_probes")
        codes = self.encode_sparse(rows, budget=budget)
        return pb.ridge_probes(codes, flags, n_concepts, alpha=alpha, fit_rows=fit_rows, max_iter=max_iter, tol=tol,
                               nactive=self._live_counts(), kernels=self._kernels)

    @torch.no_grad()
    def logistic_probes(self, rows: torch.Tensor, flags: torch.Tensor, *, n_concepts: Optional[int] = None,
                        C: float = 1.0, fit_rows: Optional[torch.Tensor] = None, max_iter: int = 12,
                        cg_iter: int = 16, tol: float = 1e-4, early_stop: bool = True,
                        budget: Optional[int] = None):
        """The logistic counterpart of ``ridge_probes`` on ``rows`` [N, d] (N a positive multiple of the batch
        size): an ``engine.probe.LogisticProbes`` -- exactly ``LogisticRegression(C=C)`` per (model, concept), the
        reference's ``logistic_regression_auroc`` for the whole ensemble -- with ``weight`` [G, n, K],
        ``intercept``, ``auroc()`` / ``auroc_heldout()`` (of the logits: the AUROC of ``predict_proba``, exact),
        ``auroc_predicted()``, ``predict_proba(codes)`` and ``top_features(m)``.  ``flags`` and ``fit_rows`` as in
        ``ridge_probes``.

        ``encode_sparse(rows, budget=budget)`` under its budget contract, the transposition, then truncated
        Newton-CG for all models and concepts in lockstep: ``max_iter`` outer steps of ``cg_iter`` Hessian
        products each, every product one pass over the CSR rows and one over the feature lists with fp64 sums,
        and a line search over eight step candidates in one pass (``csrc/probe.hip``); no dense codes.  With
        ``early_stop`` the loop reads one bool per outer step to the host, without it nothing; the result is the
        same.  The codes must be complete: a ``budget`` that is too small raises ``SparseCodesOverflow``.  Masked
        ensembles: features at or past ``dict_size[g]`` have weight 0.  There is no ``state=``.  Parameters,
        moments, shadows, ``feature_counts``, ``rows_seen``, the step counter and captured graphs are left as they
        are."""
        from . import probe as pb

        self._analysis_refusal("logistic_probes")
        codes = self.encode_sparse(rows, budget=budget)
        return pb.logistic_probes(codes, flags, n_concepts, C=C, fit_rows=fit_rows, max_iter=max_iter,
                                  cg_iter=cg_iter, tol=tol, early_stop=early_stop, nactive=self._live_counts(),
                                  kernels=self._kernels)

    @torch.no_grad()
    def attribution(self, rows: torch.Tensor, *, budget: Optional[int] = None, state=None,
                    return_proj: bool = False):
        """What every feature of every model does for the reconstruction of ``rows`` [N, d] (N a positive
        multiple of the batch size): an ``engine.attribution.Attribution`` whose ``delta_sse`` [G, n] is the
        exact rise of the summed squared error when the feature alone is removed, ``rescale`` the least-squares
        factor on its codes (the shrinkage diagnostic of L1-trained SAEs), ``harmful_fraction`` how often its
        firing makes its row worse, and ``top_mask(k)`` a keep mask for ``recon_profile``.

        ``encode_sparse(rows, budget=budget)`` under its budget contract, then per batch ``prepare()`` and one
        ``residual_proj`` launch on the batch's row window against the unit-norm bf16 shadow that
        ``recon_profile`` reads, then ``by_feature`` and one ``attr_list_sums`` launch
        (``csrc/attribution.hip``), and the variance bookkeeping of ``evaluate()``.  With a ``budget`` that is
        too small the rows whose entries were dropped are left out and counted in ``skipped`` (``check()``
        raises).  ``state``: the result of an earlier call to merge with (``Attribution.merge``).
        ``return_proj``: keep the per-entry projections, aligned with the codes' ``col`` / ``val``.  Tied models
        with a fixed affine centering are measured in the centred space.  Parameters, moments, shadows,
        ``feature_counts``, ``rows_seen``, the step counter and captured graphs are left as they are."""
        from . import attribution as at

        self._analysis_refusal("attribution")
        if state is not None:
            at.check_state(state, self.n_models, self.n, self.d)
        codes = self.encode_sparse(rows, budget=budget)
        D, live = self._dictionaries(), self._live_counts()
        if self._kernels:
            return at.attribution_fused(codes, D, self._decoder_batches(rows), live, None, state,
                                        return_proj=return_proj)
        return at.attribution_reference(codes.to(D.device), D, self._decoder_rows(rows), live, state=state,
                                        return_proj=return_proj)

    @torch.no_grad()
    def fvu_top_activating(self, rows: torch.Tensor, n_top: int = 2, *, budget: Optional[int] = None, stats=None,
                           rank_by: str = "sum"):
        """FVU of every model on ``rows`` when only its ``n_top`` most active features are kept, and the FVU
        of the rest (``eval.metrics.fraction_variance_unexplained_top_activating`` for the whole ensemble):
        (fvu_top [G], fvu_rest [G]) in fp64 on the device.  The features are ordered by the sum of their
        codes on ``rows`` descending, then feature index ascending -- from ``feature_stats(rows)``, or from
        ``stats``, an earlier ``FeatureStats`` of the same rows, to save that pass; masked ensembles rank
        only the features below ``dict_size[g]``.  ``rank_by="delta_sse"`` ranks by the exact ablation effect
        instead (``attribution(rows).top_mask(n_top)``).  The mask goes through ``recon_profile(rows,
        max_kept=0, keep=mask, budget=budget)``."""
        from . import sparse_recon as sr

        self._analysis_refusal("fvu_top_activating")
        if rank_by == "delta_sse":
            mask = self.attribution(rows, budget=budget).top_mask(n_top)
        elif rank_by != "sum":
            raise ValueError(f"rank_by must be 'sum' or 'delta_sse', got {rank_by!r}")
        else:
            if stats is None:
                stats = self.feature_stats(rows)
            mask = sr.top_features(stats.sums[:, 0].to(self.device), n_top, self._live_counts())
        prof = self.recon_profile(rows, max_kept=0, keep=mask, budget=budget)
        return prof.fvu_keep, prof.fvu_rest

    @torch.no_grad()
    def atom_matches(self, m: int = 1):
        """Nearest atoms across the models of the ensemble: an ``engine.atom_match.AtomMatches`` holding, for
        every ordered pair (g, h), the ``m`` (1..8) nearest atoms of model h for each atom of model g (cosine
        descending, lowest index among equal cosines), and for g == h the nearest *other* atoms.

        Reads the bf16 shadow that holds the unit-norm dictionaries in place (the decoder shadow of untied
        models, the encoder shadow of tied ones): the matches are those of the bf16-rounded dictionaries.
        G launches of G problems per pass on the row-argmax epilogue of the grouped GEMM
        (``ops.gemm.rowargmax_nt``).  Masked ensembles: atoms at or past ``dict_size[g]`` read (0.0, -1)
        and are never a match.  Never synchronises; parameters, moments, shadows, counts, the step
        counter and captured graphs are left as they are."""
        from . import atom_match as am

        self._analysis_refusal("atom_matches")
        D, live = self._dictionaries(), self._live_counts()
        if self._kernels:
            return am.atom_matches_fused(D, live, m)
        if live is not None:
            D = D[:, :max(live)]  # (no codes to line up with: as wide as the largest dictionary)
        return am.atom_matches_reference(D, live, m, True)


class TorchCodeAnalyses(CodeAnalyses):
    """The analytic / eager engines as a provider: the fp32 torch codes of the stacked untied / tied SAE
    parameters of ``impl`` (``feature_stats.stacked_codes``), the fp32 unit-norm dictionaries of its
    ``to_learned_dicts`` and the torch oracles, on whatever device the parameters are.  A view of the engine
    for one call: the dictionaries are exported once, when an analysis first asks for them.  ``kind``:
    "untied" / "tied"; ``None`` (a signature without an SAE encoder) leaves ``atom_matches`` alone."""

    _kernels = False

    def __init__(self, impl, kind: Optional[str], batch_size: int, device):
        self.impl, self.kind, self.batch_size, self.device = impl, kind, int(batch_size), torch.device(device)

    @property
    def n_models(self) -> int:
        return self.impl.n_models

    @property
    def n(self) -> int:
        """The width of the codes; without an encoder, that of the largest dictionary."""
        return self.impl.params["encoder"].shape[-2] if self.kind else max(self._live_counts())

    @property
    def d(self) -> int:
        return self.impl.params["encoder"].shape[-1]

    @cached_property
    def _learned(self):
        with torch.no_grad():
            return self.impl.to_learned_dicts(self.device)

    @cached_property
    def _stacked(self):
        """(fp32 [G, n, d] dictionaries, zero rows past each model's own; the models' dictionary sizes)."""
        dicts = [ld.get_learned_dict().detach().float() for ld in self._learned]
        live = [D.shape[0] for D in dicts]
        stacked = torch.zeros(len(dicts), self.n if self.kind else max(live), dicts[0].shape[1],
                              device=dicts[0].device)
        for g, D in enumerate(dicts):
            stacked[g, :D.shape[0]] = D
        return stacked, live

    def _dictionaries(self):
        return self._stacked[0]

    def _live_counts(self):
        return self._stacked[1]

    def _decoder_batches(self, rows):
        D = self._dictionaries()
        yield torch.stack([ld.center(rows.to(D.device, torch.float32)) for ld in self._learned])

    def _check_rows(self, rows, what):
        if rows.dim() != 2 or rows.shape[1] != self.d or rows.shape[0] < 1:
            raise ValueError(f"rows must be [N, {self.d}] with N >= 1, got {tuple(rows.shape)}")
        return rows.shape[0]

    def _codes(self, rows):
        from . import feature_stats as fs

        buffers, B = getattr(self.impl, "buffers", {}), self.batch_size
        return (fs.stacked_codes(self.impl.params, buffers, self.kind, rows[i:i + B])
                for i in range(0, rows.shape[0], B))

    @torch.no_grad()
    def feature_stats(self, rows: torch.Tensor, *, topk: int = 0, row_offset: int = 0, state=None):
        """The fp64 oracle on the fp32 torch codes, ``batch_size`` rows at a time (N >= 1)."""
        from . import feature_stats as fs

        self._check_rows(rows, "feature_stats")
        return fs.feature_stats_reference(self._codes(rows), topk, row_offset, state)

    @torch.no_grad()
    def encode_sparse(self, rows: torch.Tensor, *, budget: Optional[int] = None):
        """The oracle on the fp32 torch codes, ``batch_size`` rows at a time (N >= 1)."""
        from . import sparse_codes as sc

        N = self._check_rows(rows, "encode_sparse")
        return sc.sparse_codes_reference(self._codes(rows), sc.check_budget(budget, N, self.n))
