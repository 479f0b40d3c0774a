"""Time the value order of an ensemble's feature lists and the per-feature AUROC on the GPU.

Steps over the feature-major codes of one pool, alternated, each timed with a host clock around work that ends in
a device synchronise:

``by_feature``      the transposition of the pool's sparse codes, for scale
``by_value``        ``FeatureCodes.by_value()``: one ``sc_list_sort_by_value`` launch (and its scratch buffer)
``torch_sort``      the same lists from existing torch ops on the same ``FeatureCodes``: one stable ``torch.sort``
                    of the composite int64 keys ``feature 2^32 + key`` of every model's buffer and two gathers
``auroc_k1`` / ``auroc_k8`` / ``auroc_k32``   ``ValueOrdered.auroc`` for 1, 8 and 32 concepts
``worst_by_value`` / ``worst_auroc_k32``      the same on a planted worst case: the lists of model 0 replaced by
                    one feature that fires on every row (one wave walks N entries) and nothing else

Concept k marks a random ``2^-(1 + k % 6)`` of the rows from a fixed seed.  ``--engine sae`` is the feature-stats
bench shape (G = 8, d = 512, n = 2048, B = 2048, 64 pool batches, biases shifted to about ``--l0`` features per row,
``budget=64``).  Prints one JSON line.

    python scripts/value_order_bench.py
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
from sparse_coding__amd.engine.feature_codes import FeatureCodes
from sparse_coding__amd.engine.value_order import concept_words, float_keys
from sparse_coding__amd.ops.value_order import stored_ptr


def torch_sort(fc):
    """(vrow, vval) of ``fc`` from one stable global sort per model buffer."""
    b = stored_ptr(fc.col_ptr, fc.cap)
    p = torch.arange(fc.cap, device=b.device).expand(fc.n_models, -1).contiguous()
    feat = torch.searchsorted(b, p, right=True) - 1            # the tail sorts behind every list and stays put
    order = torch.sort((feat << 32) + float_keys(fc.val), dim=1, stable=True).indices
    return torch.gather(fc.row, 1, order), torch.gather(fc.val, 1, order)


def worst_case(fc):
    """``fc`` with model 0 holding one list of all rows (feature 0, values drawn from the pool's) and no other."""
    N = fc.n_rows
    col_ptr, row, val = fc.col_ptr.clone(), fc.row.clone(), fc.val.clone()
    if fc.cap < N:
        raise SystemExit("the buffers are shorter than the pool: no room for the planted list")
    col_ptr[0, 1:] = N
    row[0, :N] = torch.arange(N, device=row.device, dtype=torch.int32)
    src = fc.val[0, :max(int(fc.col_ptr[0, -1]), 1)]
    val[0, :N] = src[torch.arange(N, device=row.device) * 7919 % src.numel()].clamp(min=2 ** -20)
    row[0, N:], val[0, N:] = 0, 0.0
    return FeatureCodes(N, fc.n, col_ptr, row, val, fc.skipped)


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
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="", help="comma-separated steps to run (default: all)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("value_order_bench needs the GPU: there is no CPU timing of this path")
    sae = args.engine == "sae"
    args.d = args.d or (512 if sae else 768)
    args.n = args.n or (2048 if sae else 6144)
    args.pool_batches = args.pool_batches or (64 if sae else 16)
    args.budget = args.budget or (64 if sae else 128)
    dev = "cuda:0"
    torch.manual_seed(0)
    eng, pool, _, _ = (build_sae if sae else build_topk)(args, dev)
    sc = eng.encode_sparse(pool, budget=args.budget).check()
    nactive = getattr(eng, "nactive", None)
    N = sc.n_rows
    gen = torch.Generator().manual_seed(args.seed)
    rate = torch.tensor([2.0 ** -(1 + k % 6) for k in range(32)])
    words = {K: concept_words(torch.rand(N, K, generator=gen) < rate[:K]).to(dev) for K in (1, 8, 32)}

    fc = sc.by_feature(nactive)
    vo = fc.by_value()
    worst = worst_case(fc)
    worst_vo = worst.by_value()
    steps = {
        "by_feature": lambda: sc.by_feature(nactive),
        "by_value": lambda: fc.by_value(),
        "torch_sort": lambda: torch_sort(fc),
        "auroc_k1": lambda: vo.auroc(words[1], 1),
        "auroc_k8": lambda: vo.auroc(words[8], 8),
        "auroc_k32": lambda: vo.auroc(words[32], 32),
        "worst_by_value": lambda: worst.by_value(),
        "worst_auroc_k32": lambda: worst_vo.auroc(words[32], 32),
    }
    if args.only:
        steps = {k: v for k, v in steps.items() if k in args.only.split(",")}
    times = {k: [] for k in steps}
    last = {}
    for it in range(args.warmup + args.reps):
        for name, fn in steps.items():
            last.pop(name, None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)

    agrees = {}
    if "by_value" in last and "torch_sort" in last:
        got, (trow, tval) = last["by_value"], last["torch_sort"]
        agrees["rows_equal"] = bool(torch.equal(got.row, trow))
        agrees["values_equal"] = bool(torch.equal(got.val.view(torch.int32), tval.view(torch.int32)))
    if "worst_by_value" in last:
        w = last["worst_by_value"]
        agrees["worst_sorted"] = bool((w.val[0, 1:N] >= w.val[0, :N - 1]).all())
    med = {k: statistics.median(v) for k, v in times.items()}
    a = vo.auroc(words[8], 8).auroc()
    out = {
        "engine": args.engine,
        "shape": {"G": eng.n_models, "d": args.d, "n": args.n, "B": args.batch, "pool_rows": N, "budget": args.budget},
        "entries_per_model": sc.nnz().tolist(), "reps": args.reps,
        "longest_list": fc.counts().max(1).values.tolist(),
        "mean_list": [round(x, 1) for x in fc.counts().double().mean(1).tolist()],
        "bf16_valued": bool(torch.equal(fc.val, fc.val.to(torch.bfloat16).float())),
        "auroc_k8_range": [float(a[~a.isnan()].min()), float(a[~a.isnan()].max())],
        "raw_ms": {k: [round(t, 3) for t in v] for k, v in times.items()},
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "spread_ms": {k: round(max(v) - min(v), 3) for k, v in times.items()},
        "agrees": agrees,
    }
    if "by_value" in med and "torch_sort" in med:
        out["torch_sort_over_by_value"] = round(med["torch_sort"] / med["by_value"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
