"""Time the expected interference of a fused ensemble on the GPU.

Three paths over the same pool, alternated, each timed with a host clock around work that ends in a
device synchronise:

1. ``encode_sparse(budget=b)``      the sparse codes alone (the input of the kernel)
2. ``interference(budget=b)``       end to end: ``encode_sparse``, ``row_norm2``, ONE ``active_capacity`` launch
                                    over the pool, the low-rank static capacity
3. ``dense_torch``                  ``eval.metrics.calc_expected_interference`` per unstacked model and batch on
                                    the device, in fp32, on the engine's dense codes and the same shadow
                                    (``--dense_batches`` limits it to the first batches of the pool)

The kernel's own time comes from device events around ``--kernel_reps`` launches over the whole pool's sparse
codes.  ``--engine sae`` is the headline shape (G = 8, d = 512, n = 2048, B = 2048, 64 pool batches, biases
shifted to about ``--l0`` features per row), ``--engine topk`` config 4's (G = 8, d = 768, n = 6144,
k = 8..128, 16 pool batches).  Prints one JSON line.  ``--profile`` runs one ``interference`` call instead,
for a kernel trace:

    python scripts/interference_bench.py
    python scripts/interference_bench.py --engine topk
    rocprofv3 --kernel-trace --stats -d out -- python scripts/interference_bench.py --profile
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

from sparse_coding__amd.eval.metrics import calc_expected_interference
from sparse_coding__amd.ops import interference as ic_ops

KS = [8, 16, 24, 32, 48, 64, 96, 128]


def build_sae(args, dev):
    from sparse_coding__amd.engine.fused import FusedSAEEnsemble
    from sparse_coding__amd.models.signatures import FunctionalSAE

    G, d, n, B = args.models, args.d, args.n, args.batch
    models = [FunctionalSAE.init(d, n, l1, device=dev) for l1 in torch.logspace(-4, -2, G).tolist()]
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

    def dense_codes(x):
        eng._encode_only(eng.prepare(x))
        return eng.c

    return eng, pool, eng.dec_shadow, dense_codes


def build_topk(args, dev):
    from bench_configs import _ring
    from sparse_coding__amd.engine.topk import FusedTopKEnsemble
    from sparse_coding__amd.engine.topk_stats import dense_codes_from_picks
    from sparse_coding__amd.models.topk import TopKEncoder

    d, n, B = args.d, args.n, args.batch
    models = [TopKEncoder.init(d, n, k, device=dev) for k in KS[:args.models]]
    eng = FusedTopKEnsemble(models, lr=1e-3, batch_size=B, device=dev)
    pool = _ring(d, dev).view()[: args.pool_batches * B].contiguous()

    def dense_codes(x):
        idx, val = eng._forward_only(x, decode=False)
        return dense_codes_from_picks(idx, val, eng.k, n)

    return eng, pool, eng.shadow, dense_codes


def dense_torch(dense_codes, shadow, pool, B, batches):
    """Per-feature sums and fire counts of the dense route over the first ``batches`` batches, accumulated from
    ``calc_expected_interference`` (its per-batch mean times its clamped count is the batch's sum)."""
    G, n, _ = shadow.shape
    sums = torch.zeros(G, n, device=shadow.device, dtype=torch.float64)
    counts = torch.zeros(G, n, device=shadow.device, dtype=torch.float64)
    for i in range(0, batches * B, B):
        c = dense_codes(pool[i:i + B])
        for g in range(G):
            cg = c[g].float()
            fired = torch.count_nonzero(cg, dim=0).double()
            sums[g] += calc_expected_interference(shadow[g].float(), cg).double() * fired.clamp(min=1.0)
            counts[g] += fired
    return sums, counts


def kernel_time(codes, shadow, reps):
    """Milliseconds per ``active_capacity`` launch over all rows of ``codes`` (and per ``row_norm2`` launch),
    from device events around ``reps`` launches, median of five windows."""
    G, n, _ = shadow.shape
    dev = shadow.device
    norm2 = ic_ops.row_norm2(shadow)
    qsum = torch.zeros(G, n, device=dev, dtype=torch.int64)
    count, skipped = torch.zeros_like(qsum), torch.zeros(G, device=dev, dtype=torch.int64)
    out = {}
    for name, fn in (("row_norm2", lambda: ic_ops.row_norm2(shadow, norm2)),
                     ("active_capacity", lambda: ic_ops.active_capacity(codes.row_ptr, codes.col, codes.val, shadow,
                                                                        norm2, qsum, count, skipped))):
        fn()
        windows = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            windows.append(a.elapsed_time(b) / reps)
        out[name + "_ms"] = round(statistics.median(windows), 4)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--engine", choices=["sae", "topk"], default="sae")
    ap.add_argument("--models", type=int, default=8)
    ap.add_argument("--d", type=int)
    ap.add_argument("--n", type=int)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--pool_batches", type=int)
    ap.add_argument("--dense_batches", type=int, help="batches of the pool the dense route covers (default: all)")
    ap.add_argument("--l0", type=float, default=24.0)
    ap.add_argument("--budget", type=int)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel_reps", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("interference_bench needs the GPU: there is no CPU timing of this path")
    sae = args.engine == "sae"
    args.d = args.d or (512 if sae else 768)
    args.n = args.n or (2048 if sae else 6144)
    args.pool_batches = args.pool_batches or (64 if sae else 16)
    args.budget = args.budget or (64 if sae else 128)
    args.dense_batches = min(args.dense_batches or args.pool_batches, args.pool_batches)
    dev = "cuda:0"
    torch.manual_seed(0)
    eng, pool, shadow, dense_codes = (build_sae if sae else build_topk)(args, dev)
    B = args.batch

    if args.profile:
        eng.interference(pool[: 2 * B], budget=args.budget)  # warm
        torch.cuda.synchronize()
        eng.interference(pool, budget=args.budget)
        torch.cuda.synchronize()
        print(json.dumps({"profiled": "interference", "engine": args.engine, "budget": args.budget}))
        return

    paths = {
        "encode_sparse": lambda: eng.encode_sparse(pool, budget=args.budget),
        "interference": lambda: eng.interference(pool, budget=args.budget),
        "dense_torch": lambda: dense_torch(dense_codes, shadow, pool, B, args.dense_batches),
    }
    times = {k: [] for k in paths}
    keep = {}
    for it in range(args.warmup + args.reps):
        for name, fn in paths.items():
            keep.pop(name, None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keep[name] = fn()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)

    codes, res = keep["encode_sparse"], keep["interference"]
    lens = (codes.row_ptr[:, 1:] - codes.row_ptr[:, :-1]).double()
    # the two routes on the rows both covered
    part = eng.interference(pool[: args.dense_batches * B], budget=args.budget)
    sums, counts = keep["dense_torch"]
    dense_expected = sums / counts.clamp(min=1.0)
    med = {k: statistics.median(v) for k, v in times.items()}
    scale = args.pool_batches / args.dense_batches
    print(json.dumps({
        "engine": args.engine,
        "shape": {"G": eng.n_models, "d": args.d, "n": args.n, "B": B, "pool_rows": pool.shape[0],
                  "budget": args.budget, "dense_batches": args.dense_batches},
        "entries_per_row": {"mean": [round(float(v), 1) for v in lens.mean(1)], "max": int(lens.max())},
        "skipped": res.skipped.tolist(), "reps": args.reps,
        "raw_ms": {k: [round(t, 3) for t in v] for k, v in times.items()},
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "dense_torch_whole_pool_ms": round(med["dense_torch"] * scale, 3),
        "interference_minus_encode_ms": round(med["interference"] - med["encode_sparse"], 3),
        "speedup_vs_dense": round(med["dense_torch"] * scale / med["interference"], 2),
        "kernel": kernel_time(codes, shadow, args.kernel_reps),
        "agrees": {"counts_equal": bool(torch.equal(part.count.double(), counts)),
                   "max_abs_expected_diff": float((part.expected - dense_expected).abs().max()),
                   "mean_expected": float(part.expected[part.count > 0].mean())}}))


if __name__ == "__main__":
    main()
