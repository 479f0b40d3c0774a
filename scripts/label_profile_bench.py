"""Time the label profile of an ensemble's sparse codes on the GPU against the torch sort route.

Steps over the sparse codes of one pool and one label per row, alternated, each timed with a host clock around
work that ends in a device synchronise:

``take_rows``       ``SparseCodes.take_rows`` of the kept rows in label order (``sc_csr_take_rows``)
``by_feature``      the transposition of the gathered codes
``kernel``          one ``sc_label_profile`` launch on the transposed lists
``label_profile``   ``SparseCodes.label_profile(labels, m, n_classes)`` end to end: the label checks, the stable
                    argsort, the three steps above and ``bincount``
``torch_sort``      the same profile from existing torch ops on the same entries, model by model: a global sort of
                    the keys ``feature * L + label``, ``unique_consecutive``, segment sums (``index_add_`` in
                    fp64: their order is not reproducible), ``scatter_reduce`` maxima and a ragged top-m from
                    two more sorts

Labels are Zipf-distributed over ``--classes`` classes from a fixed seed; one row in 64 is labelled -1.
``--engine sae`` is the headline shape (G = 8, d = 512, n = 2048, B = 2048, 64 pool batches, biases shifted to
about ``--l0`` features per row, ``budget=64``), ``--engine topk`` config 4's (G = 8, d = 768, n = 6144,
k = 8..128, 16 pool batches).  Prints one JSON line.

    python scripts/label_profile_bench.py
    python scripts/label_profile_bench.py --engine topk
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
from sparse_coding__amd.engine.feature_codes import _place
from sparse_coding__amd.ops import label_profile as lp_ops


def zipf_labels(N, classes, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    p = 1.0 / torch.arange(1, classes + 1, dtype=torch.float64)
    lab = torch.multinomial(p, N, replacement=True, generator=gen)
    lab[torch.randperm(N, generator=gen)[:N // 64]] = -1
    return lab.to(dev)


def torch_sort(sc, labels, L, m):
    """(top_label, top_count, top_sum, top_max, total), per model, from global sorts over all entries."""
    n, dev = sc.n, sc.col.device
    outs = []
    for g in range(sc.n_models):
        stored = int(sc.row_ptr[g, -1])
        rows, cols, vals = sc.entry_rows(g), sc.col[g, :stored].long(), sc.val[g, :stored]
        lab = labels[rows]
        keep = lab >= 0
        key, order = torch.sort(cols[keep] * L + lab[keep], stable=True)
        v = vals[keep][order]
        runs, inv, cnt = torch.unique_consecutive(key, return_inverse=True, return_counts=True)
        rsum = torch.zeros(runs.numel(), dtype=torch.float64, device=dev).index_add_(0, inv, v.double())
        rmax = torch.zeros(runs.numel(), device=dev).scatter_reduce(0, inv, v, "amax")
        feat, rlab = runs // L, runs % L
        total = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, feat, rsum)
        o = torch.sort(rsum, descending=True, stable=True).indices
        o = o[torch.sort(feat[o], stable=True).indices]
        pf = feat[o]
        outs.append((_place(pf, rlab[o], n, m, -1, torch.int32), _place(pf, cnt[o], n, m, 0, torch.int32),
                     _place(pf, rsum[o], n, m, 0.0, torch.float64), _place(pf, rmax[o], n, m, 0.0, torch.float32),
                     total))
    return tuple(torch.stack([o[i] for o in outs]) for i in range(5))


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
    ap.add_argument("--classes", type=int, default=50000)
    ap.add_argument("--m", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="", help="comma-separated steps to run (default: all)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("label_profile_bench needs the GPU: there is no CPU timing of this path")
    sae = args.engine == "sae"
    args.d = args.d or (512 if sae else 768)
    args.n = args.n or (2048 if sae else 6144)
    args.pool_batches = args.pool_batches or (64 if sae else 16)
    args.budget = args.budget or (64 if sae else 128)
    dev = "cuda:0"
    torch.manual_seed(0)
    eng, pool, _, _ = (build_sae if sae else build_topk)(args, dev)
    G, n, m, L = eng.n_models, args.n, args.m, args.classes
    sc = eng.encode_sparse(pool, budget=args.budget).check()
    labels = zipf_labels(sc.n_rows, L, args.seed, dev)
    nactive = getattr(eng, "nactive", None)

    kept = torch.nonzero(labels >= 0).flatten()
    lab, order = torch.sort(labels[kept], stable=True)
    index, lab32 = kept[order], lab.to(torch.int32).contiguous()
    taken = sc.take_rows(index)
    fc = taken.by_feature(nactive)
    steps = {
        "take_rows": lambda: sc.take_rows(index),
        "by_feature": lambda: taken.by_feature(nactive),
        "kernel": lambda: lp_ops.label_profile(fc.col_ptr, fc.row, fc.val, lab32, m, "sum"),
        "label_profile": lambda: sc.label_profile(labels, m=m, n_classes=L, nactive=nactive),
        "torch_sort": lambda: torch_sort(sc, labels, L, m),
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
    if "label_profile" in last and "torch_sort" in last:   # the sort route's sums run in another order
        got, (tl, tc, ts, tm, tot) = last["label_profile"], last["torch_sort"]
        agrees["top_label_equal_share"] = round(float((got.top_label == tl).float().mean()), 6)
        agrees["top_count_equal_share"] = round(float((got.top_count == tc).float().mean()), 6)
        agrees["top_max_equal"] = bool(torch.equal(got.top_max, tm))
        agrees["total_max_rel_diff"] = float(((got.total - tot).abs() / tot.clamp(min=1e-300)).max())
    prof = sc.label_profile(labels, m=m, n_classes=L, nactive=nactive)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {
        "engine": args.engine,
        "shape": {"G": G, "d": args.d, "n": n, "B": args.batch, "pool_rows": pool.shape[0], "budget": args.budget,
                  "m": m, "classes": L, "kept_rows": prof.n_rows},
        "entries_per_model": sc.nnz().tolist(), "skipped": prof.skipped.tolist(), "reps": args.reps,
        "longest_list": fc.counts().max(1).values.tolist(),
        "most_labels_in_a_list": prof.n_labels.amax(1).tolist(),
        "longest_top_run": prof.top_count.amax((1, 2)).tolist(),
        "labels_present": int((prof.label_rows > 0).sum()),
        "raw_ms": {k: [round(t, 3) for t in v] for k, v in times.items()},
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "spread_ms": {k: round(max(v) - min(v), 3) for k, v in times.items()},
        "agrees": agrees,
    }
    if "label_profile" in med and "torch_sort" in med:
        out["torch_sort_over_label_profile"] = round(med["torch_sort"] / med["label_profile"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
