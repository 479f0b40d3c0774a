"""Time the feature-major transposition of an ensemble's sparse codes and the example-fragment walk on the GPU.

Paths over the sparse codes of one pool, alternated, each timed with a host clock around work that ends in a
device synchronise:

(a) ``by_feature``          the three kernels of ``csrc/feature_codes.hip`` and the cumsums between them,
    ``torch_sort``          against the same lists from existing ops, per model: ``repeat_interleave`` for the
                            entry rows, a stable ``torch.sort`` of the entry columns, two gathers and a
                            ``bincount`` (the per-model entry counts are handed to it: no synchronisation)
(b) ``feature_all``         ``FeatureCodes.feature(g, f)`` for every model and feature (slices),
    ``feature_entries``     against ``SparseCodes.feature_entries(g, f)``, SAMPLED over ``--entries_sample``
                            features of every model and scaled to all n
(c) ``examples``            ``fragment_examples`` (K top + K random) and ``fragment_acts`` for both tables, all
                            features, records staged ``--feature_chunk`` features at a time,
    ``dense``               against the dense route on the device: ``to_dense``, the per-fragment maxima,
                            ``topk`` on them, a random pick among the active fragments and the records by
                            indexing -- for ``--dense_models`` models, scaled to G

``--engine sae`` is the headline shape (G = 8, d = 512, n = 2048, B = 2048, 64 pool batches read as fragments
of 64 rows, biases shifted to about ``--l0`` features per row), ``--engine topk`` config 4's (G = 8, d = 768,
n = 6144, k = 8..128, 16 pool batches).  Prints one JSON line.

    python scripts/feature_codes_bench.py
    python scripts/feature_codes_bench.py --engine topk
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from interference_bench import build_sae, build_topk
from sparse_coding__amd.engine import feature_codes as fcm


def torch_sort(sc, nnz):
    out = []
    rows_all = torch.arange(sc.n_rows, device=sc.col.device, dtype=torch.int32)
    for g, k in enumerate(nnz):
        cols = sc.col[g, :k]
        rows = torch.repeat_interleave(rows_all, sc.row_ptr[g, 1:] - sc.row_ptr[g, :-1], output_size=k)
        order = torch.sort(cols, stable=True).indices
        col_ptr = torch.zeros(sc.n + 1, device=cols.device, dtype=torch.int64)
        col_ptr[1:] = torch.cumsum(torch.bincount(cols, minlength=sc.n), 0)
        out.append((col_ptr, rows[order], sc.val[g, :k][order]))
    return out


def feature_all(fc):
    fc.host_ptr(refresh=True)
    last = None
    for g in range(fc.n_models):
        for f in range(fc.n):
            last = fc.feature(g, f)
    return last


def feature_entries(sc, feats):
    last = None
    for g in range(sc.n_models):
        for f in feats:
            last = sc.feature_entries(g, f)
    return last


def examples(fc, L, K, chunk):
    ex = fc.fragment_examples(L, K, K, 0)
    last = None
    for f0 in range(0, fc.n, chunk):
        f1 = min(fc.n, f0 + chunk)
        for t in (ex.top_frag, ex.rand_frag):
            last = fc.fragment_acts(t[:, f0:f1].contiguous(), slice(f0, f1), L).to(torch.float16)
    return ex, last


def dense(sc, models, L, K):
    n, F = sc.n, sc.n_rows // L
    feats = torch.arange(n, device=sc.col.device).unsqueeze(1)
    last = None
    for g in range(models):
        acts = sc.to_dense(g).view(F, L, n)
        maxes = acts.amax(1)
        top = torch.topk(maxes, K, dim=0)
        keys = torch.where(maxes > 0, torch.rand(F, n, device=maxes.device), torch.full((), 2.0, device=maxes.device))
        rnd = torch.topk(keys, K, dim=0, largest=False).indices
        last = (top.values, acts[top.indices.T, :, feats].to(torch.float16), acts[rnd.T, :, feats].to(torch.float16))
    return last


def event_ms(fn, reps):
    fn()
    windows = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        windows.append(e0.elapsed_time(e1) / reps)
    return round(statistics.median(windows), 4)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--engine", choices=["sae", "topk"], default="sae")
    ap.add_argument("--models", type=int, default=8)
    ap.add_argument("--d", type=int)
    ap.add_argument("--n", type=int)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--pool_batches", type=int)
    ap.add_argument("--l0", type=float, default=24.0)
    ap.add_argument("--budget", type=int)
    ap.add_argument("--fragment_len", type=int, default=64)
    ap.add_argument("--examples", type=int, default=20)
    ap.add_argument("--feature_chunk", type=int, default=256)
    ap.add_argument("--entries_sample", type=int, default=64)
    ap.add_argument("--dense_models", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel_reps", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated paths to run (default: all)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("feature_codes_bench needs the GPU: there is no CPU timing of this path")
    sae = args.engine == "sae"
    args.d = args.d or (512 if sae else 768)
    args.n = args.n or (2048 if sae else 6144)
    args.pool_batches = args.pool_batches or (64 if sae else 16)
    args.budget = args.budget or (64 if sae else 128)
    dev = "cuda:0"
    torch.manual_seed(0)
    eng, pool, _, _ = (build_sae if sae else build_topk)(args, dev)
    G, n, L, K = eng.n_models, args.n, args.fragment_len, args.examples
    sc = eng.encode_sparse(pool, budget=args.budget)
    nnz = sc.nnz().clamp(max=sc.cap).tolist()
    fc = sc.by_feature().check()
    sample = torch.linspace(0, n - 1, args.entries_sample).long().tolist()

    paths = {
        "by_feature": lambda: sc.by_feature(),
        "torch_sort": lambda: torch_sort(sc, nnz),
        "feature_all": lambda: feature_all(fc),
        "feature_entries": lambda: feature_entries(sc, sample),
        "examples": lambda: examples(fc, L, K, args.feature_chunk),
        "dense": lambda: dense(sc, args.dense_models, L, K),
    }
    if args.only:
        paths = {k: v for k, v in paths.items() if k in args.only.split(",")}
    times = {k: [] for k in paths}
    last = {}
    for it in range(args.warmup + args.reps):
        for name, fn in paths.items():
            last.pop(name, None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)

    agrees = {}
    if "torch_sort" in last and "by_feature" in last:
        got = last["by_feature"]
        agrees["lists_equal_torch_sort"] = all(
            torch.equal(got.col_ptr[g], cp) and torch.equal(got.row[g, :r.numel()], r)
            and torch.equal(got.val[g, :v.numel()], v) for g, (cp, r, v) in enumerate(last["torch_sort"]))
    if "dense" in last and "examples" in last:
        agrees["top_max_equal_dense"] = bool(torch.equal(last["examples"][0].top_max[args.dense_models - 1],
                                                         last["dense"][0].T.contiguous()))
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    ex = fc.fragment_examples(L, K, K, 0)
    tables = (ex.top_frag.contiguous(), ex.rand_frag.contiguous())
    out = {
        "engine": args.engine,
        "shape": {"G": G, "d": args.d, "n": n, "B": args.batch, "pool_rows": pool.shape[0], "budget": args.budget,
                  "fragment_len": L, "examples": K, "feature_chunk": args.feature_chunk,
                  "entries_sample": args.entries_sample, "dense_models": args.dense_models},
        "entries_per_model": nnz, "skipped": fc.skipped.tolist(), "reps": args.reps,
        "raw_ms": {k: [round(t, 3) for t in v] for k, v in times.items()},
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "spread_ms": {k: round(v, 3) for k, v in spread.items()},
        "agrees": agrees,
        "kernel": {"by_feature_ms": event_ms(lambda: sc.by_feature(), args.kernel_reps),
                   "fragment_examples_ms": event_ms(lambda: fc.fragment_examples(L, K, K, 0), args.kernel_reps),
                   "fragment_acts_all_features_ms": event_ms(
                       lambda: [fc.fragment_acts(t, slice(None), L) for t in tables], 1)},
    }
    if "feature_entries" in med:
        out["feature_entries_all_features_ms"] = round(med["feature_entries"] * n / args.entries_sample, 3)
    if "dense" in med:
        out["dense_all_models_ms"] = round(med["dense"] * G / args.dense_models, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
