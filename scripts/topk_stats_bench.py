"""Time the per-feature quantities of a fused top-k ensemble on the GPU (config 4's shape by default).

``pool`` mode (default): paths over the same pool, alternated, each timed with a host clock around
work that ends in a device synchronise:

1. ``select_only``                 the floor: scores GEMM + select per pool batch
2. ``feature_stats(topk=0 / K)``   the sparse route: select, slot lists of all models, ``pick_stats``
3. ``dense(topk=0 / K)``           the same outputs from existing ops: select, ``scatter`` into a bf16
                                   [G, B, n] buffer, ``col_moments`` (/ ``col_topk``), ``clear``
4. ``evaluate``                    select + decode
5. ``resample_dead``               one event on the pool (every repeat is a new event on the state the
                                   previous one left)

``step`` mode: the in-step cost of the window counts -- three engines from the same models with
``count_every`` 0 / 1 / 8, multi-step source graphs as ``bench_configs.py topk``, alternated.

``--profile feature_stats|resample_dead|evaluate``: one warmed pass of that call, for a kernel trace:

    python scripts/topk_stats_bench.py
    python scripts/topk_stats_bench.py step --steps 200
    rocprofv3 --kernel-trace --stats -d out -- python scripts/topk_stats_bench.py --profile resample_dead

Prints one JSON line.
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

from bench_configs import _ring
from sparse_coding__amd.engine import feature_stats as fs
from sparse_coding__amd.engine.topk import FusedTopKEnsemble
from sparse_coding__amd.models.topk import TopKEncoder
from sparse_coding__amd.ops import feature_stats as fs_ops
from sparse_coding__amd.ops import topk as topk_ops

KS = [8, 16, 24, 32, 48, 64, 96, 128]


def dense_stats(eng: FusedTopKEnsemble, pool: torch.Tensor, K: int, code: torch.Tensor, part: torch.Tensor):
    """The outputs of ``feature_stats`` by the dense route: the picks scattered into the zeroed bf16 buffer
    ``code`` [G, B, n], the SAE engines' column reductions over it, and the picks cleared again."""
    B, G, n, dev = eng.batch_size, eng.n_models, eng.n, eng.device
    acc = torch.zeros(G, 5, n, device=dev, dtype=torch.float64)
    mx = torch.zeros(G, n, device=dev)
    tv = tr = None
    if K:
        tv, tr = fs.empty_topk(G, n, K, dev)
    for i in range(0, pool.shape[0], B):
        idx, val = eng._forward_only(pool[i:i + B], decode=False)
        topk_ops.scatter(idx, val, eng.k, code)
        fs_ops.col_moments(code, part)
        if K:
            fs_ops.col_topk(code, tv, tr, i)
        topk_ops.clear(idx, code, code)  # (one buffer in both slots: the same zero is stored twice)
        acc += part[:, :, :5].sum(1, dtype=torch.float64)
        mx = torch.maximum(mx, part[:, :, 5].amax(1))
    return fs.FeatureStats(pool.shape[0], acc[:, 0].round().to(torch.int64), acc[:, 1:].contiguous(), mx, tv, tr)


def _select_only(eng, pool):
    for i in range(0, pool.shape[0], eng.batch_size):
        eng._forward_only(pool[i:i + eng.batch_size], decode=False)


def _spread(v):
    return round((max(v) - min(v)) / statistics.median(v), 4)


def run_pool(args, eng, pool):
    B, G, n, K = eng.batch_size, eng.n_models, eng.n, args.topk
    code = torch.zeros(G, B, n, device=eng.device, dtype=torch.bfloat16)
    part = torch.empty(G, fs_ops.moment_slabs(G, B, n), fs_ops.N_STATS, n, device=eng.device)
    paths = {
        "select_only": lambda: _select_only(eng, pool),
        "feature_stats_topk0": lambda: eng.feature_stats(pool),
        f"feature_stats_topk{K}": lambda: eng.feature_stats(pool, topk=K),
        "dense_topk0": lambda: dense_stats(eng, pool, 0, code, part),
        f"dense_topk{K}": lambda: dense_stats(eng, pool, K, code, part),
        "evaluate": lambda: eng.evaluate(pool),
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
    ours, base = keep[f"feature_stats_topk{K}"], keep[f"dense_topk{K}"]
    same = {"count": bool(torch.equal(ours.count, base.count)), "max": bool(torch.equal(ours.max, base.max)),
            "top_vals": bool(torch.equal(ours.top_vals, base.top_vals)),
            "top_rows": bool(torch.equal(ours.top_rows, base.top_rows)),
            "sums_max_rel_diff": float(((ours.sums - base.sums).abs() / base.sums.abs().clamp(min=1e-30)).max())}
    # resampling events last: they change the dictionaries
    events, counts = [], []
    for _ in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cnt = eng.resample_dead(pool)
        torch.cuda.synchronize()
        events.append((time.perf_counter() - t0) * 1e3)
        counts.append(int(cnt.sum()))
    times["resample_dead"] = events[args.warmup:]
    med = {k: statistics.median(v) for k, v in times.items()}
    fvu, l0 = keep["evaluate"]
    return {"mode": "pool", "shape": {"G": G, "d": eng.d, "n": n, "B": B, "k": KS[:G], "pool_batches": args.pool_batches,
                                      "topk": K},
            "l0": [round(float(v), 1) for v in l0], "reps": args.reps,
            "raw_ms": {k: [round(t, 3) for t in v] for k, v in times.items()},
            "median_ms": {k: round(v, 3) for k, v in med.items()},
            "spread": {k: _spread(v) for k, v in times.items()},
            "per_batch_us": {k: round(v * 1e3 / args.pool_batches, 1) for k, v in med.items()},
            "sparse_over_dense": {"topk0": round(med["feature_stats_topk0"] / med["dense_topk0"], 3),
                                  f"topk{K}": round(med[f"feature_stats_topk{K}"] / med[f"dense_topk{K}"], 3)},
            "resampled_per_event": counts, "sparse_agrees_with_dense": same}


def run_step(args, models, ring):
    B, gs = args.batch, max(1, args.graph_steps)
    steps = max(1, args.steps // gs) * gs
    engs, srcs = {}, {}
    for ce in (0, 1, 8):
        engs[ce] = FusedTopKEnsemble(models, lr=1e-3, batch_size=B, device="cuda:0", count_every=ce)
        srcs[ce] = ring.graph_source(B)
        for _ in range(max(1, args.warmup)):
            engs[ce].run_source(srcs[ce], gs)
    times = {ce: [] for ce in engs}
    for _ in range(args.reps):
        for ce, eng in engs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps // gs):
                eng.run_source(srcs[ce], gs)
            torch.cuda.synchronize()
            times[ce].append((time.perf_counter() - t0) * 1e3 / steps)
    med = {ce: statistics.median(v) for ce, v in times.items()}
    return {"mode": "step", "shape": {"G": len(models), "d": engs[0].d, "n": engs[0].n, "B": B, "k": KS[:len(models)]},
            "steps": steps, "graph_steps": gs, "reps": args.reps,
            "raw_ms_per_step": {f"count_every_{ce}": [round(t, 4) for t in v] for ce, v in times.items()},
            "median_ms_per_step": {f"count_every_{ce}": round(v, 4) for ce, v in med.items()},
            "spread": {f"count_every_{ce}": _spread(v) for ce, v in times.items()},
            "vs_count_every_0": {f"count_every_{ce}": round(med[ce] / med[0], 4) for ce in med},
            "rows_seen": {f"count_every_{ce}": e.rows_seen for ce, e in engs.items()}}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", nargs="?", default="pool", choices=["pool", "step"])
    ap.add_argument("--models", type=int, default=8)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--ratio", type=int, default=8)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--pool_batches", type=int, default=16)
    ap.add_argument("--topk", type=int, default=16)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--graph-steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--profile", choices=["feature_stats", "resample_dead", "evaluate"])
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("topk_stats_bench needs the GPU: there is no CPU timing of this path")
    dev = "cuda:0"
    torch.manual_seed(0)
    d, B = args.d, args.batch
    n = d * args.ratio
    models = [TopKEncoder.init(d, n, k, device=dev) for k in KS[:args.models]]
    ring = _ring(d, dev)
    if args.mode == "step" and not args.profile:
        print(json.dumps(run_step(args, models, ring)))
        return
    eng = FusedTopKEnsemble(models, lr=1e-3, batch_size=B, device=dev)
    pool = ring.view()[: args.pool_batches * B].contiguous()
    if args.profile:
        call = {"feature_stats": lambda p: eng.feature_stats(p, topk=args.topk),
                "resample_dead": eng.resample_dead, "evaluate": eng.evaluate}[args.profile]
        call(pool[: 2 * B])  # warm
        torch.cuda.synchronize()
        call(pool)
        torch.cuda.synchronize()
        print(json.dumps({"profiled": args.profile, "topk": args.topk, "batches": args.pool_batches + 2}))
        return
    print(json.dumps(run_pool(args, eng, pool)))


if __name__ == "__main__":
    main()
