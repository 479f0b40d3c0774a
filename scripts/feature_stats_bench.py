"""Time per-feature activation statistics of a fused SAE ensemble on the GPU.

Five paths over the same pool, alternated, each timed with a host clock around work that ends in a
device synchronise:

1. ``evaluate``                        the forward-only floor (encoder + decoder launches)
2. ``feature_stats(topk=0)``           encoder launch + ``col_moments``
3. ``feature_stats(topk=K)``           ... + ``col_topk``
4. a torch baseline of 2 / 3          the same outputs from ``engine.c`` after each encoder launch:
                                       ``c.float()`` powers and sums, ``torch.topk`` over the concatenated state
5. ``calc_moments_streaming``          one unstacked fp32 model at a time (moments only)

The models' biases are shifted so that about ``--l0`` features fire per row (0: leave the fresh
initialisation, about half of them).  Prints one JSON line.  ``--profile`` runs a single
``feature_stats(topk=K)`` pass instead, for a kernel trace:

    python scripts/feature_stats_bench.py                  # G=8 d=512 n=2048 B=2048, 64 pool batches
    rocprofv3 --kernel-trace --stats -d out -- python scripts/feature_stats_bench.py --profile
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

from sparse_coding__amd.engine import feature_stats as fs
from sparse_coding__amd.engine.fused import FusedSAEEnsemble
from sparse_coding__amd.eval import metrics as M
from sparse_coding__amd.models.signatures import FunctionalSAE


def torch_stats(eng: FusedSAEEnsemble, pool: torch.Tensor, K: int):
    """The outputs of ``feature_stats`` from torch ops on the engine's codes."""
    B, G, n = eng.batch_size, eng.n_models, eng.n
    dev = eng.device
    acc = torch.zeros(G, 5, n, device=dev, dtype=torch.float64)
    mx = torch.full((G, n), float("-inf"), device=dev)
    tv = tr = None
    if K:
        tv, tr = fs.empty_topk(G, n, K, dev)
    for i in range(0, pool.shape[0], B):
        eng._encode_only(pool[i:i + B])
        c = eng.c.float()
        c2 = c * c
        acc[:, 0] += (c != 0).sum(1)
        acc[:, 1] += c.sum(1)
        acc[:, 2] += c2.sum(1)
        acc[:, 3] += (c2 * c).sum(1)
        acc[:, 4] += (c2 * c2).sum(1)
        mx = torch.maximum(mx, c.amax(1))
        if K:
            rows = torch.arange(i, i + B, device=dev).expand(G, n, B)
            top = torch.topk(torch.cat([tv, c.transpose(1, 2)], dim=-1), K, dim=-1)
            tr = torch.gather(torch.cat([tr, rows], dim=-1), -1, top.indices)
            tv = top.values
            tr = torch.where(tv > 0, tr, torch.full_like(tr, -1))
    return fs.FeatureStats(pool.shape[0], acc[:, 0].round().long(), acc[:, 1:], mx, tv, tr)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", type=int, default=8)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--pool_batches", type=int, default=64)
    ap.add_argument("--topk", type=int, default=16)
    ap.add_argument("--l0", type=float, default=24.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("feature_stats_bench needs the GPU: there is no CPU timing of this path")
    dev = "cuda:0"
    torch.manual_seed(0)
    G, d, n, B, K = args.models, args.d, args.n, args.batch, args.topk
    l1s = torch.logspace(-4, -2, G).tolist()
    models = [FunctionalSAE.init(d, n, l1, device=dev) for l1 in l1s]
    N = args.pool_batches * B
    feats = torch.nn.functional.normalize(torch.randn(4 * d, d, device=dev), dim=-1)
    pool = torch.cat([(torch.relu(torch.randn(B, 4 * d, device=dev) - 2.0) @ feats).to(torch.bfloat16)
                      for _ in range(args.pool_batches)])
    if args.l0 > 0:  # one bias per model: the pre-activation quantile that leaves about l0 features firing
        with torch.no_grad():
            for p, _ in models:
                pre = pool[:B].float() @ p["encoder"].float().T
                k = max(1, int(round(pre.numel() * (1.0 - args.l0 / n))))
                p["encoder_bias"].fill_(-float(pre.flatten().kthvalue(k).values))
    eng = FusedSAEEnsemble(models, FunctionalSAE, lr=1e-3, batch_size=B, device=dev)
    _, l0 = eng.evaluate(pool[: 4 * B])

    if args.profile:
        eng.feature_stats(pool[: 2 * B], topk=K)  # warm
        torch.cuda.synchronize()
        eng.feature_stats(pool, topk=K)
        torch.cuda.synchronize()
        print(json.dumps({"profiled": "feature_stats", "topk": K, "batches": args.pool_batches + 2,
                          "l0": [round(float(v), 1) for v in l0]}))
        return

    lds = eng.to_learned_dicts(device=dev)
    poolf = pool.float()
    paths = {
        "evaluate": lambda: eng.evaluate(pool),
        "feature_stats_topk0": lambda: eng.feature_stats(pool),
        f"feature_stats_topk{K}": lambda: eng.feature_stats(pool, topk=K),
        "torch_topk0": lambda: torch_stats(eng, pool, 0),
        f"torch_topk{K}": lambda: torch_stats(eng, pool, K),
        "calc_moments_streaming_x_models": lambda: [M.calc_moments_streaming(ld, poolf) for ld in lds],
    }
    times = {k: [] for k in paths}
    keep = {}
    for it in range(args.warmup + args.reps):
        for name, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keep[name] = fn()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)

    # the two implementations computed the same thing
    ours, base = keep[f"feature_stats_topk{K}"], keep[f"torch_topk{K}"]
    same = {"count": bool(torch.equal(ours.count, base.count)), "max": bool(torch.equal(ours.max, base.max)),
            "top_vals": bool(torch.equal(ours.top_vals, base.top_vals)),
            "sums_max_rel_diff": float(((ours.sums - base.sums).abs() / base.sums.abs().clamp(min=1e-30)).max())}
    med = {k: statistics.median(v) for k, v in times.items()}
    floor = med["evaluate"]
    print(json.dumps({
        "shape": {"G": G, "d": d, "n": n, "B": B, "pool_rows": N, "topk": K},
        "l0": [round(float(v), 1) for v in l0], "reps": args.reps,
        "raw_ms": {k: [round(t, 3) for t in v] for k, v in times.items()},
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "per_batch_us": {k: round(v * 1e3 / args.pool_batches, 1) for k, v in med.items()},
        "vs_evaluate": {k: round(v / floor, 3) for k, v in med.items()},
        "speedup_vs_torch": {"topk0": round(med["torch_topk0"] / med["feature_stats_topk0"], 2),
                             f"topk{K}": round(med[f"torch_topk{K}"] / med[f"feature_stats_topk{K}"], 2)},
        "speedup_vs_calc_moments_streaming": round(med["calc_moments_streaming_x_models"]
                                                   / med["feature_stats_topk0"], 2),
        "agrees_with_torch": same}))


if __name__ == "__main__":
    main()
