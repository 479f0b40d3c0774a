"""``FusedTopKEnsemble``: top-k dictionary learning for many k in one pass (MI355X path).

Per step, for all models at once (reference runs a Python loop over models because
k differs, ``autoencoders/ensemble.py:100-116``; math of ``autoencoders/topk_encoder.py:19-40``):

1. scores = x D_hat^T                     grouped MFMA GEMM, bf16 epilogue (fp32 accumulation)
2. (idx, val) = top-k(scores), ReLU       per-model k on device; the picks are the fp32 top-k:
                                           bf16 rounding is monotone, so only keys equal to the
                                           k-th largest bf16 key are ambiguous, and those are
                                           ranked by exact fp32 recomputes <x, D_hat[j]>
                                           (``scores_dtype='fp32'``: the fp32 score matrix and
                                           its select; a select fused into the scores GEMM --
                                           candidate append above a sampled bound -- measured
                                           1.51 vs 1.01 ms/step, profiles/r5/topk_candidates/)
3. x_hat = sum val D_hat[idx]; R = x_hat - x; code gradients <R, D_hat[idx]>
                                           one wave per row (sparse gather from L2); the
                                           previous step's dense-buffer picks are cleared here
4. dD_hat = code^T R + dscore^T x          models with small k: feature-major slot lists built
                                           on the device (counting sort) and one wave per
                                           dictionary row summing its picks; the others: ONE
                                           MFMA GEMM with two K segments over the scattered
                                           (dense bf16) code / dscore
5. the step tail, ONE launch (csrc/adam.hip ``sc_topk_tail``): Adam with the row-norm Jacobian
   (D_hat = dict / |dict|) + bf16 shadow, the per-model MSE from the decode's per-row squared errors,
   the next step's batch gather (multi-step source graphs) and the device step counter

``enable_graph()`` captures the whole step as one HIP graph (two, alternating the pick buffers:
step t clears step t-1's picks).

Per-feature quantities come from the picks, never from a dense [G, B, n] code matrix
(``ops/topk_stats.py``): window fire counts inside the step (``count_every``), ``evaluate``,
``resample_dead`` and ``feature_stats`` on a forward-only pass with pick buffers of its own.
"""

from __future__ import annotations

import os
from typing import Optional, Union

import torch

from ..ops import adam as adam_ops
from ..ops import gemm as gemm_ops
from ..ops import topk as topk_ops
from ..ops import topk_stats as tstats_ops
from .analysis import CodeAnalyses

# Cost model of the weight gradient per model (MI355X, measured on config 4): the slot-list
# kernel moves ~4 d bytes per pick at ~5 TB/s from L2 / MALL; the dense two-segment GEMM does
# 4 B n d FLOPs at ~0.9 PF.  A model takes the sparse path when that is clearly cheaper.
_SPARSE_BW = 5.0e12
_DENSE_FLOPS = 0.9e15


def auto_sparse_k(B: int, n: int, d: int, margin: float = 1.3) -> int:
    """Largest k whose slot-list weight gradient beats the dense GEMM by ``margin``."""
    dense = 4.0 * B * n * d / _DENSE_FLOPS
    per_k = B * 4.0 * d / _SPARSE_BW
    return int(dense / (per_k * margin))


class FusedTopKEnsemble(CodeAnalyses):
    def __init__(self, models, sig=None, lr=1e-3, batch_size=256, device="cuda", betas=(0.9, 0.999), eps=1e-8,
                 grad_dtype: str = "bf16", sparse_k: Union[int, str] = "auto", scores_dtype: Optional[str] = None,
                 fused_tail: bool = True, count_every: int = 0):
        from ..models.topk import TopKEncoder

        self.sig = sig or TopKEncoder
        self.device = dev = torch.device(device)
        self.n_models = G = len(models)
        self.batch_size = B = int(batch_size)
        self.n, self.d = models[0][0]["dict"].shape
        n, d = self.n, self.d
        if B % 128 or n % 128 or d % 256:
            raise ValueError(f"fused top-k needs B%128==0, n%128==0, d%256==0 (B={B}, n={n}, d={d})")
        if not adam_ops.row_width_supported(d):
            raise ValueError(f"fused top-k: the row-Adam kernels support the row widths {adam_ops.ROW_WIDTHS} "
                             f"only (got d={d})")
        self.params = {"dict": torch.stack([m[0]["dict"].detach().float() for m in models]).to(dev).contiguous()}
        self.m = {"dict": torch.zeros_like(self.params["dict"])}
        self.v = {"dict": torch.zeros_like(self.params["dict"])}
        ks = [int(m[1]["sparsity"]) for m in models]
        self.k = torch.tensor(ks, dtype=torch.int32, device=dev)
        self.kmax = kmax = max(ks)
        self.meta = [dict(m[1]) for m in models]
        lrs = lr if isinstance(lr, (list, tuple)) else [lr] * G
        self.lr = torch.tensor([float(x) for x in lrs], device=dev)
        self.betas, self.eps = betas, eps
        self.step_count = 0
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)

        bf = torch.bfloat16
        self.shadow = torch.empty(G, n, d, device=dev, dtype=bf)
        self.norms = torch.ones(G, n, device=dev)
        adam_ops.shadow_rows(self.params["dict"], self.shadow, self.norms, normalize=True)
        # score matrix: bf16 by default (half the HBM round trip of fp32; SC_TOPK_SCORES=fp32 to compare)
        sdt = scores_dtype or os.environ.get("SC_TOPK_SCORES", "bf16")
        if sdt not in ("fp32", "bf16"):
            raise ValueError(f"scores_dtype must be 'fp32' or 'bf16', got {sdt!r}")
        # (a hipBLASLt scores GEMM over the stacked dictionaries with a [B, G, n] select measured no
        # consistent gain over four boxes: scripts/lab/topk_blas_gemmk_r5.patch)
        self.scores = torch.empty(G, B, n, device=dev, dtype=torch.bfloat16 if sdt == "bf16" else torch.float32)
        # pick buffers, alternating per step: the decode of step t zeroes step t-1's picks in the
        # dense code / dscore buffers (no separate clear launch)
        self.idx_buf = torch.zeros(2, G, B, kmax, device=dev, dtype=torch.int32)
        self.val = torch.zeros(G, B, kmax, device=dev)
        self._cur = 0
        self.idx = self.idx_buf[0]
        self.r = torch.empty(G, B, d, device=dev, dtype=bf)
        self.row_se = torch.empty(G, B, device=dev)
        self.codebuf = torch.zeros(G, B, n, device=dev, dtype=bf)
        self.dscbuf = torch.zeros(G, B, n, device=dev, dtype=bf)
        # weight gradient: the leading models with k <= sparse_k from slot lists, the rest dense
        if sparse_k == "auto":
            sparse_k = auto_sparse_k(B, n, d)
        gs = 0
        while gs < G and ks[gs] <= int(sparse_k) and d <= 1024:
            gs += 1
        self.sparse_g = gs
        # the decode scatters codes / code gradients only for the dense-wgrad models (config 4:
        # 1.054 vs 1.059 ms/step scattering for all, profiles/r4/topk_scatter/)
        self._dense_from = gs
        # (decoding the large-k models as dense MFMA GEMMs over the scattered codes measured +3-5 %:
        # scripts/lab/topk_blas_gemmk_r5.patch; every model decodes by the per-row gather)
        self.lists = topk_ops.SlotLists(gs, B, n, ks, kmax, dev) if gs else None
        self.dscv = torch.zeros(G, B, kmax, device=dev) if gs else None
        # bf16 dictionary gradient by default: the dense GEMM's bf16 epilogue + Adam's bf16 loads
        # (config 4: 1.178 -> 1.133 ms/step, profiles/grad_dtype_ab_r2.json); Adam math stays fp32
        if grad_dtype not in ("fp32", "bf16"):
            raise ValueError(f"grad_dtype must be 'fp32' or 'bf16', got {grad_dtype!r}")
        self.g = torch.empty(G, n, d, device=dev, dtype=bf if grad_dtype == "bf16" else torch.float32)
        self.mse = torch.zeros(G, device=dev)
        # fused tail (``fused_tail=False``: Adam + torch reductions + counter increment as separate launches)
        self._tail = bool(fused_tail) and adam_ops.tail_width_supported(d)
        self._ticket = torch.zeros(adam_ops.TICKET_INTS, device=dev, dtype=torch.int32)
        self.x_static = torch.zeros(B, d, device=dev, dtype=bf)
        self.use_graph = False
        self._graphs = None
        self._src_graphs = None
        # window fire counts: every `count_every`-th step histograms its picks (0: off -- nothing is
        # allocated and the step launches what it always did); `rows_seen` counts those steps' rows
        self.count_every = int(count_every)
        if self.count_every < 0:
            raise ValueError(f"count_every must be >= 0, got {count_every}")
        self.feature_counts = torch.zeros(G, n, device=dev, dtype=torch.int64) if self.count_every else None
        self.rows_seen = 0
        self._ks = ks
        self._fwd = None    # (idx, val) of the forward-only pass
        self._stat_lists = None

    # ------------------------------------------------------------------ the step
    def _step_kernels(self, x, cur: int, gather=None):
        G, B, n, d = self.n_models, self.batch_size, self.n, self.d
        idx, prev = self.idx_buf[cur], self.idx_buf[1 - cur]
        gemm_ops.matmul_nt(x, self.shadow, self.scores)
        topk_ops.topk_select(self.scores, self.k, self.kmax, out=(idx, self.val), x=x, D=self.shadow)
        if self.count_every:
            # the device decides (step_dev % count_every == 0): one captured graph serves every step
            tstats_ops.pick_counts(idx, self.val, self.k, self.feature_counts, self.step_dev, self.count_every)
        topk_ops.decode_grad(idx, self.val, self.k, self.shadow, x, self.r, self.row_se, self.codebuf,
                             self.dscbuf, dscv=self.dscv, prev_idx=prev, dense_from=self._dense_from)
        alpha = 2.0 / (B * d)
        gs = self.sparse_g
        if gs:
            topk_ops.slot_lists(idx, self.k, self.lists)
            topk_ops.sparse_wgrad(self.lists, self.val, self.dscv, self.r, x, self.g[:gs], alpha)
        if gs < G:
            gemm_ops.weight_grads([[(self.codebuf[gs:], self.r[gs:]), (self.dscbuf[gs:], x)]], [self.g[gs:]], alpha)
        if self._tail:
            adam_ops.topk_tail(self.params["dict"], self.g, self.m["dict"], self.v["dict"], self.shadow, self.norms,
                               self.lr, *self.betas, self.eps, self.step_dev, self.row_se, self.mse, 1.0 / (B * d),
                               self._ticket, gather=gather)
            return
        torch.mul(torch.sum(self.row_se, dim=1), 1.0 / (B * d), out=self.mse)
        adam_ops.adam_rows([dict(p=self.params["dict"], g=self.g, m=self.m["dict"], v=self.v["dict"],
                                 shadow=self.shadow, norms=self.norms, norm=True)],
                           self.lr, self.step_count + 1, *self.betas, self.eps, step_dev=self.step_dev)
        self.step_dev.add_(1)
        if gather is not None:
            raise RuntimeError("the next-batch gather needs the fused tail")

    def enable_graph(self, enabled: bool = True):
        """Replay the whole step from a HIP graph (one per pick-buffer parity); the batch goes
        through ``x_static``."""
        self.use_graph = enabled
        self._graphs = None
        return self

    def _capture(self):
        torch.cuda.synchronize(self.device)
        self._graphs = []
        for cur in (0, 1):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._step_kernels(self.x_static, cur)
            self._graphs.append(g)

    def step_batch(self, batch):
        """One Adam step of every model; returns the per-model MSE (the reference's loss) on device."""
        x = batch if batch is self.x_static else batch.to(self.device, torch.bfloat16).contiguous()
        if self.use_graph:
            if x is not self.x_static:
                self.x_static.copy_(x)
            if self._graphs is None:
                self._capture()
            self._graphs[self._cur].replay()
        else:
            self._step_kernels(x, self._cur)
        self.idx = self.idx_buf[self._cur]
        self._cur ^= 1
        self.rows_seen += self.batch_size * self._counting_steps(self.step_count, 1)
        self.step_count += 1
        return self.mse

    def _counting_steps(self, t0: int, steps: int) -> int:
        """How many of the steps t0 .. t0 + steps - 1 count their picks (t % count_every == 0)."""
        c = self.count_every
        if not c:
            return 0
        return (t0 + steps + c - 1) // c - (t0 + c - 1) // c

    def _capture_source(self, source, steps: int, cur0: int):
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            # each step's batch: the first step's own gather kernel; later steps' rows are fetched by the
            # previous step's tail (one launch fewer per step) when the source allows it
            nxt = source.tail_gather(self.x_static) if (self._tail and hasattr(source, "tail_gather")) else None
            for i in range(steps):
                if i == 0 or nxt is None:
                    source.gather(self.x_static, self.step_dev)
                self._step_kernels(self.x_static, cur0 ^ (i & 1), gather=nxt if i + 1 < steps else None)
        return g

    def run_source(self, source, steps: int):
        """``steps`` optimizer steps as ONE graph replay with every batch fetched INSIDE the graph
        (``data.ring.RingGraphSource``: one gather kernel per step on the device step counter), so
        no host sampling or replay boundary sits between steps.  The pick-buffer parity follows the
        step index; graphs are cached per (steps, starting parity)."""
        steps = int(steps)
        if steps < 1:
            raise ValueError("steps must be >= 1")
        if getattr(source, "B", self.batch_size) != self.batch_size:
            raise ValueError("the source's batch size differs from the engine's")
        if self._src_graphs is None or self._src_graphs[0] is not source:
            self._src_graphs = (source, {})
        key = (steps, self._cur)
        graphs = self._src_graphs[1]
        source.prepare(self.step_count, steps)
        if key not in graphs:
            graphs[key] = self._capture_source(source, steps, self._cur)
        graphs[key].replay()
        last = self._cur ^ ((steps - 1) & 1)
        self.idx = self.idx_buf[last]
        self._cur = last ^ 1
        self.rows_seen += self.batch_size * self._counting_steps(self.step_count, steps)
        self.step_count += steps
        return self.mse

    # ------------------------------------------------------------------ fire counts, evaluation, resampling, statistics
    def feature_frequency(self) -> torch.Tensor:
        """Per-feature firing frequency [G, n] = feature_counts / rows_seen over the steps that counted
        (every ``count_every``-th; exact for ``count_every=1``) since the last reset.  A firing is a pick
        with a positive code: a pick whose score the ReLU clamped to 0 does not count."""
        if self.feature_counts is None:
            raise RuntimeError("feature counting is off (count_every=0)")
        return self.feature_counts / max(1, self.rows_seen)

    def _x_bf16(self, rows):
        return rows.to(self.device, torch.bfloat16).contiguous()

    def _forward_only(self, x, decode: bool = True):
        """Scores, select and (``decode``) residual of one bf16 batch ``x`` [B, d] without gradients, as
        the training step computes them (the scores GEMM into ``scores``, the select with the exact tie
        resolve) but with pick buffers of its own: ``idx_buf``, the parity, the dense code / code-gradient
        buffers, ``dscv``, ``mse``, the step counter, the parameters and captured graphs are untouched
        (the dense buffers must keep holding exactly the previous parity's picks).  Overwrites the
        scratch ``scores`` / ``r`` / ``row_se``, which every training step rewrites before reading.
        Returns the picks (idx, val)."""
        if self._fwd is None:
            G, B, kmax = self.n_models, self.batch_size, self.kmax
            self._fwd = (torch.zeros(G, B, kmax, device=self.device, dtype=torch.int32),
                         torch.zeros(G, B, kmax, device=self.device))
        idx, val = self._fwd
        gemm_ops.matmul_nt(x, self.shadow, self.scores)
        topk_ops.topk_select(self.scores, self.k, self.kmax, out=(idx, val), x=x, D=self.shadow)
        if decode:  # (no dense buffers: the kernel returns after row_se, nothing is scattered or cleared)
            topk_ops.decode_grad(idx, val, self.k, self.shadow, x, self.r, self.row_se, None, None)
        return idx, val

    # the hooks of ``CodeAnalyses`` (engine/analysis.py: ``interference`` .. ``atom_matches``).  Nothing is
    # refused and nothing is masked; the decoder reads the pool's bf16 rows as they are
    def _dictionaries(self):
        return self.shadow

    def _decoder_batches(self, rows):
        B, pool = self.batch_size, self._x_bf16(rows)
        return (pool[i:i + B] for i in range(0, rows.shape[0], B))

    @torch.no_grad()
    def evaluate(self, rows: torch.Tensor):
        """FVU and mean L0 of every model on ``rows`` [N, d] (trimmed to a multiple of the batch size):
        the squared error from the decode's per-row sums, the variance bookkeeping in fp64, L0 the mean
        number of positive codes per row.  Returns (fvu [G], l0 [G]) on the device; never synchronises."""
        B, G = self.batch_size, self.n_models
        if rows.dim() != 2 or rows.shape[1] != self.d:
            raise ValueError(f"rows must be [N, {self.d}], got {tuple(rows.shape)}")
        N = rows.shape[0] - rows.shape[0] % B
        if N == 0:
            raise ValueError(f"need at least {B} rows")
        f64 = torch.float64
        se = torch.zeros(G, device=self.device, dtype=f64)
        l0 = torch.zeros(G, device=self.device, dtype=f64)
        s1 = torch.zeros(self.d, device=self.device, dtype=f64)
        s2 = torch.zeros((), device=self.device, dtype=f64)
        for i in range(0, N, B):
            x = self._x_bf16(rows[i:i + B])
            _, val = self._forward_only(x)
            se += self.row_se.sum(1, dtype=f64)
            l0 += (val > 0).sum((1, 2)).double()  # (the padded slots hold 0.0)
            xf = x.double()
            s1 += xf.sum(0)
            s2 += xf.pow(2).sum()
        var = s2 - s1.pow(2).sum() / N  # total sum of squares about the mean
        return (se / var).float(), (l0 / N).float()

    @torch.no_grad()
    def resample_dead(self, rows: torch.Tensor, *, pick: str = "worst", ratio: float = 1.0,
                      use_window_counts: bool = True, generator: Optional[torch.Generator] = None,
                      rule: Optional[str] = None) -> torch.Tensor:
        """Re-seed dead atoms from badly reconstructed rows of the candidate pool ``rows`` [N, d] (N a
        positive multiple of the batch size); returns the per-model number of resampled atoms as a
        device tensor [G].  Never synchronises; captured step graphs stay valid.

        The pool is scored forward-only, batch by batch: the decode's per-row squared errors and the
        fire counts of the picks (a pick with code 0 is not a firing).  Atom (g, f) is dead when it never
        fires on the pool and -- ``use_window_counts``, if the engine counts (``count_every > 0``) and has
        counted rows since the last reset -- has ``feature_counts[g, f] == 0`` too.
        ``engine.resample.plan_resample`` pairs the dead atoms (ascending) with pool rows (``pick``), and
        one ``sc_resample_dict_rows`` launch writes master row <- unit pool row x scale[g], zeroes its
        Adam moments and rewrites its bf16 shadow row and row norm.  scale[g] = ``ratio`` x the mean
        master-row norm of the alive atoms (of all atoms if none is alive): the dictionary is used
        normalised, so the master norm does not change the forward pass -- it only sets Adam's RELATIVE
        step on the row, and ``ratio = 1.0`` keeps that the same as for the row's neighbours.  There is
        one rewrite rule here: ``rule`` (the SAE engines' keyword, which the sweep driver passes) is
        accepted and ignored.  Afterwards ``feature_counts`` and ``rows_seen`` are reset."""
        from ..ops import resample as rs_ops
        from . import resample as rs
        from . import topk_stats as ts

        if pick not in rs.PICKS:
            raise ValueError(f"pick must be one of {rs.PICKS}, got {pick!r}")
        N = self._check_rows(rows, "the pool")
        B, G, n, dev = self.batch_size, self.n_models, self.n, self.device
        pool = self._x_bf16(rows)
        err = torch.empty(G, N, device=dev)
        fired = torch.zeros(G, n, device=dev, dtype=torch.int64)
        for i in range(0, N, B):
            idx, val = self._forward_only(pool[i:i + B])
            err[:, i:i + B].copy_(self.row_se)
            tstats_ops.pick_counts(idx, val, self.k, fired)
        dead = fired == 0
        if use_window_counts and self.feature_counts is not None and self.rows_seen > 0:
            dead &= self.feature_counts == 0
        dead_idx, src_idx, cnt = rs.plan_resample(dead, err, pick=pick, generator=generator)
        scale = ts.resample_dict_scales(self.params["dict"], dead, ratio)
        rs_ops.resample_dict_rows(dead_idx, src_idx, cnt, pool, scale, self.params["dict"], self.m["dict"],
                                  self.v["dict"], self.shadow, self.norms, normalize_src=True)
        if self.feature_counts is not None:
            self.feature_counts.zero_()
        self.rows_seen = 0
        return cnt

    @torch.no_grad()
    def feature_stats(self, rows: torch.Tensor, *, topk: int = 0, row_offset: int = 0, state=None):
        """Per-feature activation statistics of every model on ``rows`` [N, d] (N a positive multiple of
        the batch size): an ``engine.feature_stats.FeatureStats`` with the SAE engine's argument contract
        (``topk`` in 0..32, ``row_offset``, continuation through ``state``).  Never synchronises.

        Per batch: the forward-only select (no decode), the feature-major slot lists of ALL models
        (``sc_topk_slot_lists`` into buffers of this method's own, not the training step's) and one
        ``pick_stats`` launch that walks every feature's list in row order -- no dense code matrix.  Only
        positive codes take part; a feature nobody picks reads count 0, max 0.0 and rows of -1, as
        the dense reduction would.  Bit-reproducible, and chunk by chunk through ``state`` gives the
        bits of one call on the whole pool.  Parameters, moments, shadows, window counts, the step
        counter and captured graphs are left as they are."""
        from . import feature_stats as fs

        N = self._check_rows(rows, "feature_stats")
        B, G, n, dev = self.batch_size, self.n_models, self.n, self.device
        topk, row_offset = fs.check_request(topk, row_offset, state, G, n)
        if self._stat_lists is None:
            self._stat_lists = topk_ops.SlotLists(G, B, n, self._ks, self.kmax, dev)
        acc, mx, tv, tr, seen = fs.open_accumulators(state, G, n, topk, dev, 0.0)
        pool = self._x_bf16(rows)
        for i in range(0, N, B):
            idx, val = self._forward_only(pool[i:i + B], decode=False)
            topk_ops.slot_lists(idx, self.k, self._stat_lists)  # (leaves its counters zero for the next batch)
            tstats_ops.pick_stats(self._stat_lists, val, acc, mx, tv, tr, row_offset + i)
        return fs.FeatureStats(seen + N, acc[:, 0].round().to(torch.int64), acc[:, 1:].contiguous(), mx, tv, tr)

    @torch.no_grad()
    def encode_sparse(self, rows: torch.Tensor, *, budget: Optional[int] = None):
        """The codes of every model on ``rows`` [N, d] (N a positive multiple of the batch size) as an
        ``engine.sparse_codes.SparseCodes`` with the SAE engine's contract: per-model CSR of the picks
        with a positive code (a pick the ReLU clamped to 0 is no entry), columns ascending within a row.

        Per batch: the forward-only select (no decode); the kept picks of each row are sorted by column
        with torch ops on the [G, B, kmax] pick buffers -- no dense code matrix, no new kernel.
        ``budget=int``: buffers of ``min(N * budget, N * n)`` entries per model, never synchronises,
        overflow is reported through ``row_ptr`` / ``overflow()``.  ``budget=None`` (default): ONE
        synchronisation reads the per-model totals and the buffers are sized to the largest model.
        Equals the oracle on ``engine.topk_stats.dense_codes_from_picks`` of the same picks.  Parameters,
        moments, shadows, window counts, the step counter and captured graphs are left as they are."""
        from . import sparse_codes as sc

        N = self._check_rows(rows, "encode_sparse")
        B = self.batch_size
        cap = sc.check_budget(budget, N, self.n)
        pool = self._x_bf16(rows)

        def picks():
            for i in range(0, N, B):
                idx, val = self._forward_only(pool[i:i + B], decode=False)
                yield idx, val  # (consumed before the next batch overwrites the pick buffers)

        return sc.sparse_codes_from_picks(picks(), self.k, self.n, cap)

    def state_dict(self):
        """Masters, moments and the step; with ``count_every > 0`` also the window counts."""
        sd = {"params": self.params, "m": self.m, "v": self.v, "step": self.step_count}
        if self.feature_counts is not None:
            sd["feature_counts"], sd["rows_seen"] = self.feature_counts, self.rows_seen
        return sd

    def load_state_dict(self, sd):
        """Counts and ``rows_seen`` are optional (checkpoints from before the engine counted)."""
        for d_ in ("params", "m", "v"):
            for k, t in sd[d_].items():
                getattr(self, d_)[k].copy_(t)
        self.step_count = int(sd["step"])
        self.step_dev.fill_(self.step_count)
        adam_ops.shadow_rows(self.params["dict"], self.shadow, self.norms, normalize=True)
        if self.feature_counts is not None:
            if sd.get("feature_counts") is not None:
                self.feature_counts.copy_(sd["feature_counts"])
                self.rows_seen = int(sd.get("rows_seen", 0))
            else:
                self.feature_counts.zero_()
                self.rows_seen = 0

    # ------------------------------------------------------------------ inference / export
    def encode(self, x):
        """Dense top-k codes [G, B, n] for ``x`` [B, d] with the current dictionaries."""
        xb = x.to(self.device, torch.bfloat16).contiguous()
        # (inference: fp32 scores, so the codes carry the GEMM's fp32 values)
        scores = torch.empty(self.n_models, x.shape[0], self.n, device=self.device)
        gemm_ops.matmul_nt(xb, self.shadow, scores)
        idx, val = topk_ops.topk_select(scores, self.k, self.kmax)
        # slots >= k[g] are padded with (index 0, value 0): scatter_add keeps a real pick of
        # feature 0 intact (real indices are unique, the padded values add 0)
        return torch.zeros_like(scores).scatter_add_(-1, idx.long(), val)

    def unstack(self, device="cpu"):
        return [({"dict": self.params["dict"][i].detach().to(device).clone()},
                 {k: (v.detach().to(device).clone() if torch.is_tensor(v) else v) for k, v in self.meta[i].items()})
                for i in range(self.n_models)]

    def to_learned_dicts(self, device="cpu"):
        return [self.sig.to_learned_dict(p, b) for p, b in self.unstack(device)]
