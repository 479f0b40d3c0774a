"""Feature-activation datasets: per-fragment, per-token dictionary activations.

Reference: ``interpret.py:82-212`` (``make_feature_activation_dataset``) and
``:215-253`` (``get_df``): 50k random 64-token fragments (one per document), the
LM activation at (layer, loc) encoded by the dictionary, stored as a pandas table
with a ``feature_i_max`` column and 64 ``feature_i_activation_j`` columns per feature.

MI355X design: fragments run through the LM in large batches; the activations are
encoded on the device and written straight into preallocated fp16 tensors
``acts [F, L, n_feats]`` / ``maxes [F, n_feats]`` (no per-fragment Python loop, no
wide DataFrame).  The dataset saves as a dict of tensors (loads with
``weights_only=True``); ``to_dataframe`` produces the reference's column layout
when a pandas table is wanted.
"""

from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Callable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .hooked import HookedLM, tensor_name

FRAGMENT_LEN = 64
MAX_FRAGMENTS = 50000


@dataclass
class FeatureActivationDataset:
    token_ids: torch.Tensor     # [F, L] int32
    acts: torch.Tensor          # [F, L, n] fp16
    maxes: torch.Tensor         # [F, n] fp16
    token_strs: Optional[List[List[str]]] = None

    @property
    def n_feats(self) -> int:
        return self.acts.shape[-1]

    def __len__(self):
        return self.acts.shape[0]

    def save(self, path: str):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save({"token_ids": self.token_ids, "acts": self.acts, "maxes": self.maxes,
                    "token_strs": self.token_strs}, path)

    @classmethod
    def load(cls, path: str) -> "FeatureActivationDataset":
        d = torch.load(path, weights_only=True)
        return cls(d["token_ids"], d["acts"], d["maxes"], d.get("token_strs"))

    def top_fragments(self, feat: int, k: int) -> torch.Tensor:
        """Indices of the ``k`` fragments with the largest max activation of ``feat``."""
        return torch.topk(self.maxes[:, feat].float(), min(k, len(self))).indices

    def random_active_fragments(self, feat: int, k: int, generator: Optional[torch.Generator] = None
                                ) -> Optional[torch.Tensor]:
        """``k`` random fragments on which ``feat`` fires at all; None if fewer exist."""
        active = torch.nonzero(self.maxes[:, feat] > 0).flatten()
        if active.numel() < k:
            return None
        return active[torch.randperm(active.numel(), generator=generator)[:k]]

    def fragment_acts(self, feat: int, idx: int) -> torch.Tensor:
        """The [L] activations of ``feat`` on fragment ``idx``."""
        return self.acts[idx, :, feat]

    def to_dataframe(self):
        """Reference column layout (``fragment_token_ids``, ``feature_i_max``,
        ``feature_i_activation_j``)."""
        import pandas as pd

        F, L, n = self.acts.shape
        cols = {"fragment_token_ids": [r.tolist() for r in self.token_ids]}
        if self.token_strs is not None:
            cols["fragment_token_strs"] = self.token_strs
        df = pd.DataFrame(cols)
        maxes = pd.DataFrame(self.maxes.float().numpy(), columns=[f"feature_{i}_max" for i in range(n)])
        acts = pd.DataFrame(self.acts.reshape(F, L * n).float().numpy(),  # column j*n + i
                            columns=[f"feature_{i}_activation_{j}" for j in range(L) for i in range(n)])
        return pd.concat([df, maxes, acts], axis=1)


def random_fragments(token_docs: Iterator[torch.Tensor], n: int, fragment_len: int = FRAGMENT_LEN,
                     rng: Optional[np.random.Generator] = None, random_start: bool = True) -> torch.Tensor:
    """One random ``fragment_len`` window per document (reference :136-157); documents shorter
    than a fragment are skipped."""
    rng = rng or np.random.default_rng(0)
    out = []
    for doc in token_docs:
        doc = doc.flatten()
        if doc.numel() < fragment_len:
            continue
        s = int(rng.integers(0, doc.numel() - fragment_len + 1)) if random_start else 0
        out.append(doc[s:s + fragment_len])
        if len(out) >= n:
            break
    return torch.stack(out)


@torch.no_grad()
def make_feature_activation_dataset(lm: HookedLM, learned_dict, layer: int, layer_loc: str,
                                    fragments: torch.Tensor, max_features: int = 0, batch_size: int = 256,
                                    tokenizer=None, store_device="cpu") -> FeatureActivationDataset:
    """Encode every fragment's activations at (layer, layer_loc) with ``learned_dict``."""
    dev = lm.device
    learned_dict.to_device(dev)
    name = tensor_name(layer, layer_loc)
    n_all = learned_dict.get_learned_dict().shape[0]
    n = min(max_features, n_all) if max_features else n_all
    F, L = fragments.shape
    acts = torch.empty(F, L, n, dtype=torch.float16, device=store_device)
    maxes = torch.empty(F, n, dtype=torch.float16, device=store_device)
    for i in range(0, F, batch_size):
        toks = fragments[i:i + batch_size].to(dev)
        _, cache = lm.run_with_cache(toks, names_filter=[name], return_type=None)
        h = cache[name]
        b = h.shape[0]
        c = learned_dict.encode(h.reshape(b * L, -1).float())[:, :n].reshape(b, L, n)
        acts[i:i + b] = c.to(store_device, torch.float16)
        maxes[i:i + b] = c.max(dim=1).values.to(store_device, torch.float16)
    strs = None
    if tokenizer is not None and hasattr(tokenizer, "convert_ids_to_tokens"):
        strs = [tokenizer.convert_ids_to_tokens(r.tolist()) for r in fragments]
    return FeatureActivationDataset(fragments.to(torch.int32).cpu(), acts, maxes, strs)


def feature_activation_dataset_from_sparse(sc, g: int, fragments: torch.Tensor, max_features: int = 0,
                                           token_strs: Optional[List[List[str]]] = None
                                           ) -> FeatureActivationDataset:
    """The activation dataset of model ``g`` from the sparse codes ``sc`` (``engine.sparse_codes.SparseCodes``)
    of the fragments' tokens: row ``i`` of ``sc`` is token ``i % L`` of fragment ``i // L``.  The same
    ``acts`` / ``maxes`` (fp16, on the CPU) that ``make_feature_activation_dataset`` builds from dense
    codes, features ``0 .. max_features - 1`` when ``max_features`` is set."""
    F, L = fragments.shape
    if sc.n_rows != F * L:
        raise ValueError(f"the codes have {sc.n_rows} rows, {F} fragments of {L} tokens need {F * L} "
                         "(narrow_rows drops padding rows)")
    sc.check()
    n = min(max_features, sc.n) if max_features else sc.n
    stored = int(sc.row_ptr[g, -1])
    cols, vals = sc.col[g, :stored].long(), sc.val[g, :stored]
    rows = sc.entry_rows(g)
    if n < sc.n:
        keep = cols < n
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
    acts = torch.zeros(F * L, n, dtype=torch.float16)
    acts[rows.cpu(), cols.cpu()] = vals.to("cpu", torch.float16)
    acts = acts.view(F, L, n)
    # (fp16 rounding is monotone: the max of the rounded values is the rounded max)
    return FeatureActivationDataset(fragments.to(torch.int32).cpu(), acts, acts.max(dim=1).values, token_strs)


@torch.no_grad()
def ensemble_feature_activation_datasets(lm: HookedLM, trainer, layer: int, layer_loc: str, fragments: torch.Tensor,
                                         max_features: int = 0, batch_size: int = 256, tokenizer=None,
                                         budget: Optional[int] = None) -> List[FeatureActivationDataset]:
    """One activation dataset per model of ``trainer`` (an ``EnsembleTrainer``) from ONE pass of the LM over
    the fragments: the activations at (layer, layer_loc) are collected on the device, padded with zero rows
    up to a multiple of the trainer's batch size, encoded by ``trainer.encode_sparse`` for all models at
    once (``budget`` as there) and cut back to the fragments' rows -- no unstacking, no dense codes on the
    device."""
    dev = lm.device
    name = tensor_name(layer, layer_loc)
    F, L = fragments.shape
    B = int(getattr(trainer.impl, "batch_size", trainer.batch_size))
    n_pad = -(-F * L // B) * B
    dtype = torch.bfloat16 if trainer.kind in ("fused-sae", "fused-topk") else torch.float32
    rows = None
    for i in range(0, F, batch_size):
        toks = fragments[i:i + batch_size].to(dev)
        _, cache = lm.run_with_cache(toks, names_filter=[name], return_type=None)
        h = cache[name]
        h = h.reshape(h.shape[0] * L, -1)
        if rows is None:
            rows = torch.zeros(n_pad, h.shape[-1], dtype=dtype, device=dev)
        rows[i * L: i * L + h.shape[0]] = h.to(dtype)
    sc = trainer.encode_sparse(rows, budget=budget).narrow_rows(0, F * L)
    strs = None
    if tokenizer is not None and hasattr(tokenizer, "convert_ids_to_tokens"):
        strs = [tokenizer.convert_ids_to_tokens(r.tolist()) for r in fragments]
    return [feature_activation_dataset_from_sparse(sc, g, fragments, max_features, strs)
            for g in range(sc.n_models)]


@dataclass
class FeatureExampleSet:
    """What auto-interpretation reads of one model, without the dense ``acts``: per feature the number of
    fragments on which it fires, its top fragments (largest maximum first, ties to the lower fragment) and a
    hash sample of its active fragments (``engine.feature_codes``), each with its [L] activation record.
    ``autointerp.feature_record`` / ``interpret`` run on it as on a ``FeatureActivationDataset``."""

    token_ids: torch.Tensor     # [F, L] int32
    n_frags: torch.Tensor       # [n] int64
    top_frag: torch.Tensor      # [n, K] int32, -1: empty slot
    top_acts: torch.Tensor      # [n, K, L] fp16
    rand_frag: torch.Tensor     # [n, K] int32, -1: empty slot
    rand_acts: torch.Tensor     # [n, K, L] fp16
    token_strs: Optional[List[List[str]]] = None

    @property
    def n_feats(self) -> int:
        return self.n_frags.shape[0]

    def __len__(self):
        return self.token_ids.shape[0]

    def save(self, path: str):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save({"token_ids": self.token_ids, "n_frags": self.n_frags, "top_frag": self.top_frag,
                    "top_acts": self.top_acts, "rand_frag": self.rand_frag, "rand_acts": self.rand_acts,
                    "token_strs": self.token_strs}, path)

    @classmethod
    def load(cls, path: str) -> "FeatureExampleSet":
        d = torch.load(path, weights_only=True)
        return cls(d["token_ids"], d["n_frags"], d["top_frag"], d["top_acts"], d["rand_frag"], d["rand_acts"],
                   d.get("token_strs"))

    def _first(self, table: torch.Tensor, feat: int, k: int, what: str) -> torch.Tensor:
        if k > table.shape[1]:
            raise ValueError(f"{k} {what} fragments asked for, {table.shape[1]} are stored per feature")
        t = table[feat, :k]
        return t[t >= 0].long()

    def top_fragments(self, feat: int, k: int) -> torch.Tensor:
        """Indices of the (at most) ``k`` active fragments with the largest max activation of ``feat``."""
        return self._first(self.top_frag, feat, k, "top")

    def random_active_fragments(self, feat: int, k: int, generator: Optional[torch.Generator] = None
                                ) -> Optional[torch.Tensor]:
        """``k`` fragments on which ``feat`` fires; None if fewer exist.  The sample is the stored hash sample's
        first ``k`` (itself a sample of size k, fixed by the seed the set was built with): ``generator`` is
        accepted for the dense dataset's signature and not used."""
        if int(self.n_frags[feat]) < k:
            return None
        return self._first(self.rand_frag, feat, k, "random")

    def fragment_acts(self, feat: int, idx: int) -> torch.Tensor:
        """The [L] activations of ``feat`` on fragment ``idx``, one of its stored top or random fragments."""
        for frag, acts in ((self.top_frag, self.top_acts), (self.rand_frag, self.rand_acts)):
            hit = torch.nonzero(frag[feat] == int(idx)).flatten()
            if hit.numel():
                return acts[feat, int(hit[0])]
        raise KeyError(f"fragment {idx} is not among the stored examples of feature {feat}")


def feature_example_sets_from_codes(fc, ex, fragments: torch.Tensor, token_strs: Optional[List[List[str]]] = None,
                                    feature_chunk: int = 256) -> List[FeatureExampleSet]:
    """One ``FeatureExampleSet`` per model from feature-major codes ``fc`` (``engine.feature_codes.FeatureCodes``)
    and their ``FragmentExamples`` ``ex``.  The records are gathered ``feature_chunk`` features at a time
    (``FeatureCodes.fragment_acts``), so the fp32 staging stays at G * chunk * K * L values."""
    F, L = fragments.shape
    if fc.n_rows != F * L or ex.fragment_len != L:
        raise ValueError(f"the codes have {fc.n_rows} rows in fragments of {ex.fragment_len}, {F} fragments of {L} "
                         "tokens were given")
    G, n = fc.n_models, fc.n
    tables = {"top": ex.top_frag, "rand": ex.rand_frag}
    acts = {k: torch.empty(G, n, t.shape[2], L, dtype=torch.float16) for k, t in tables.items()}
    for f0 in range(0, n, feature_chunk):
        f1 = min(n, f0 + feature_chunk)
        for k, t in tables.items():
            rec = fc.fragment_acts(t[:, f0:f1].contiguous(), slice(f0, f1), L)
            acts[k][:, f0:f1] = rec.to("cpu", torch.float16)
    ids = fragments.to(torch.int32).cpu()
    n_frags, top, rnd = ex.n_frags.cpu(), ex.top_frag.cpu(), ex.rand_frag.cpu()
    return [FeatureExampleSet(ids, n_frags[g], top[g], acts["top"][g], rnd[g], acts["rand"][g], token_strs)
            for g in range(G)]


@torch.no_grad()
def ensemble_feature_example_sets(lm: HookedLM, trainer, layer: int, layer_loc: str, fragments: torch.Tensor,
                                  n_examples: Optional[int] = None, seed: int = 0, budget: Optional[int] = None,
                                  tokenizer=None, batch_size: int = 256) -> List[FeatureExampleSet]:
    """One ``FeatureExampleSet`` per model of ``trainer`` (an ``EnsembleTrainer``) from ONE pass of the LM over
    the fragments, with no dense ``[F * L, n]`` code tensor on any device: the activations at (layer,
    layer_loc) are collected on the device and go through ``trainer.feature_examples`` (sparse codes for all
    models at once, the feature-major transposition, ``n_examples`` -- default ``autointerp.TOTAL_EXAMPLES`` --
    top and random fragments per feature).  When the fragments' rows are no multiple of the trainer's batch
    size they are padded with zero rows for ``encode_sparse``, the codes are cut back to the fragments' rows
    (``narrow_rows``) and transposed from there, so a padding row is never an example."""
    from ..engine import feature_codes as fcm

    if n_examples is None:
        from .autointerp import TOTAL_EXAMPLES as n_examples
    dev = lm.device
    name = tensor_name(layer, layer_loc)
    F, L = fragments.shape
    B = int(getattr(trainer.impl, "batch_size", trainer.batch_size))
    n_pad = -(-F * L // B) * B
    dtype = torch.bfloat16 if trainer.kind in ("fused-sae", "fused-topk") else torch.float32
    rows = None
    for i in range(0, F, batch_size):
        toks = fragments[i:i + batch_size].to(dev)
        _, cache = lm.run_with_cache(toks, names_filter=[name], return_type=None)
        h = cache[name]
        h = h.reshape(h.shape[0] * L, -1)
        if rows is None:
            rows = torch.zeros(n_pad, h.shape[-1], dtype=dtype, device=dev)
        rows[i * L: i * L + h.shape[0]] = h.to(dtype)
    if n_pad == F * L:
        fc, ex = trainer.feature_examples(rows, fragment_len=L, n_top=n_examples, n_random=n_examples, seed=seed,
                                          budget=budget)
    else:
        sc = trainer.encode_sparse(rows, budget=budget).narrow_rows(0, F * L)
        fc, ex = fcm.feature_examples(sc, getattr(trainer.impl, "nactive", None), L, n_examples, n_examples, seed)
    strs = None
    if tokenizer is not None and hasattr(tokenizer, "convert_ids_to_tokens"):
        strs = [tokenizer.convert_ids_to_tokens(r.tolist()) for r in fragments]
    return feature_example_sets_from_codes(fc, ex, fragments, strs)


def token_labels(fragments: torch.Tensor, context: str = "self", ignore: Sequence[int] = ()) -> torch.Tensor:
    """One label per token of ``fragments`` [F, L], int64 [F * L] in row order: the token's own id (``context``
    "self") or the id of the token before it ("prev"; the first token of a fragment has none and reads -1).
    Token ids in ``ignore`` read -1: a negative label leaves the row out of a label profile."""
    if context not in ("self", "prev"):
        raise ValueError(f"context must be 'self' or 'prev', got {context!r}")
    ids = fragments.to(torch.int64)
    if context == "prev":
        ids = torch.cat([torch.full_like(ids[:, :1], -1), ids[:, :-1]], dim=1)
    for t in ignore:
        ids = torch.where(ids == int(t), torch.full_like(ids, -1), ids)
    return ids.reshape(-1)


@torch.no_grad()
def ensemble_token_profiles(lm: HookedLM, trainer, layer: int, layer_loc: str, fragments: torch.Tensor, m: int = 8,
                            context: str = "self", ignore: Sequence[int] = (), rank_by: str = "sum",
                            n_classes: Optional[int] = None, budget: Optional[int] = None, batch_size: int = 256):
    """The token profile of every feature of every model of ``trainer`` (an ``EnsembleTrainer``): an
    ``engine.label_profile.LabelProfile`` whose labels are token ids -- per feature the ``m`` tokens that carry
    most of its activation over ALL fragments, where ``TokenStatsExplainer`` guesses them from a handful of
    example fragments.  ONE pass of the LM over the fragments and ONE ``encode_sparse`` for all models: the
    activations at (layer, layer_loc) are collected on the device, padded with zero rows up to a multiple of the
    trainer's batch size (their label is -1, so a padding row is in no profile) and go through
    ``trainer.label_profile`` with the labels of ``token_labels(fragments, context, ignore)``."""
    dev = lm.device
    name = tensor_name(layer, layer_loc)
    F, L = fragments.shape
    B = int(getattr(trainer.impl, "batch_size", trainer.batch_size))
    n_pad = -(-F * L // B) * B
    dtype = torch.bfloat16 if trainer.kind in ("fused-sae", "fused-topk") else torch.float32
    rows = None
    for i in range(0, F, batch_size):
        toks = fragments[i:i + batch_size].to(dev)
        _, cache = lm.run_with_cache(toks, names_filter=[name], return_type=None)
        h = cache[name]
        h = h.reshape(h.shape[0] * L, -1)
        if rows is None:
            rows = torch.zeros(n_pad, h.shape[-1], dtype=dtype, device=dev)
        rows[i * L: i * L + h.shape[0]] = h.to(dtype)
    labels = torch.full((n_pad,), -1, dtype=torch.int64)
    labels[:F * L] = token_labels(fragments.cpu(), context, ignore)
    return trainer.label_profile(rows, labels, m=m, rank_by=rank_by, n_classes=n_classes, budget=budget)


def concept_flags(tokens: torch.Tensor, concepts) -> Tuple[torch.Tensor, List[str]]:
    """Flag words for ``ValueOrdered.auroc`` / ``trainer.feature_auroc`` from token ids: ``concepts`` maps up to 32
    concept names to the token ids that make a row a positive of the concept.  Returns ``(flags int32 [numel],
    names)``: bit k of word r is set when token r (``tokens`` of any shape, in row order) is one of the ids of
    ``names[k]``, the k-th key of ``concepts``."""
    from ..engine.value_order import concept_words

    names = list(concepts)
    ids = tokens.reshape(-1).to(torch.int64)
    hit = torch.zeros(ids.numel(), len(names), dtype=torch.bool, device=ids.device)
    for k, name in enumerate(names):
        hit[:, k] = torch.isin(ids, torch.as_tensor(list(concepts[name]), dtype=torch.int64, device=ids.device))
    return concept_words(hit), names


def stratified_examples(fc, vo, n_strata: int, per_stratum: int, fragment_len: int, features: slice = slice(None)):
    """Quantile-binned example fragments of the features ``features`` (a contiguous slice, F of them): from the
    value-ordered lists ``vo`` (``fc.by_value()``), per feature and stratum of its sorted activations (stratum
    ``n_strata - 1`` holds the largest) ``per_stratum`` evenly spaced entries -- ``(frags int32, vals fp32) [G, F,
    S, r]``, the fragment ``row // fragment_len`` of each picked row and its code, (-1, 0.0) in empty slots -- and
    ``acts`` fp32 [G, F, S, r, L], the feature's activation record on each of those fragments
    (``FeatureCodes.fragment_acts`` of the row-ordered ``fc``).  ``FragmentExamples`` shows a feature's top and
    a random sample; this shows what is typical of its middle range."""
    f0, f1, step = features.indices(fc.n)
    if step != 1:
        raise ValueError("features must be a contiguous slice")
    f1 = max(f1, f0)
    rows, vals = vo.strata(n_strata, per_stratum)
    rows, vals = rows[:, f0:f1], vals[:, f0:f1]
    L = int(fragment_len)
    frags = torch.where(rows >= 0, torch.div(rows, L, rounding_mode="floor"), rows)
    G, F, S, r = frags.shape
    acts = fc.fragment_acts(frags.reshape(G, F, S * r).contiguous(), slice(f0, f1), L)
    return frags, vals.contiguous(), acts.view(G, F, S, r, L)


def get_dataset(learned_dict, lm: HookedLM, layer: int, layer_loc: str, n_feats: int, save_loc: str,
                fragments: Callable[[], torch.Tensor], force_refresh: bool = False, **kw) -> FeatureActivationDataset:
    """Cached ``make_feature_activation_dataset`` (reference get_df)."""
    path = os.path.join(save_loc, "activation_dataset.pt")
    if os.path.exists(path) and not force_refresh:
        ds = FeatureActivationDataset.load(path)
        if ds.n_feats >= n_feats:
            return ds
    ds = make_feature_activation_dataset(lm, learned_dict, layer, layer_loc, fragments(), max_features=n_feats, **kw)
    ds.save(path)
    return ds
