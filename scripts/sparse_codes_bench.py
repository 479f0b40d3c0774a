"""Time the sparse export of a fused SAE ensemble's codes on the GPU.

Five paths over the same pool, alternated, each timed with a host clock around work that ends in a
device synchronise:

1. ``encode_only``                     the floor: the encoder launch per batch, nothing read back
2. ``encode_sparse(budget=b)``         one sweep: encoder + ``code_row_counts`` + cumsum + ``code_compact``
3. ``encode_sparse(budget=None)``      count sweep, one synchronisation, fill sweep (the pool is encoded twice)
4. ``torch_nonzero``                   existing ops on the same engine: ``_encode_only``, then
                                       ``torch.nonzero(engine.c > 0)`` plus a gather of the values, per batch
5. ``torch_to_sparse_csr``             ... ``engine.c[g].float().to_sparse_csr()`` per model and batch

The two kernels' own times come from device events around ``--kernel_reps`` back-to-back launches on one
batch of codes.  The models' biases are shifted so that about ``--l0`` features fire per row.  Prints one
JSON line.  ``--profile`` runs a single ``encode_sparse`` pass per mode instead, for a kernel trace:

    python scripts/sparse_codes_bench.py                   # G=8 d=512 n=2048 B=2048, 64 pool batches
    rocprofv3 --kernel-trace --stats -d out -- python scripts/sparse_codes_bench.py --profile
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

from sparse_coding__amd.engine import sparse_codes as sc
from sparse_coding__amd.engine.fused import FusedSAEEnsemble
from sparse_coding__amd.models.signatures import FunctionalSAE
from sparse_coding__amd.ops import sparse_codes as sc_ops


def encode_only(eng: FusedSAEEnsemble, pool: torch.Tensor):
    B = eng.batch_size
    for i in range(0, pool.shape[0], B):
        eng._encode_only(pool[i:i + B])


def torch_nonzero(eng: FusedSAEEnsemble, pool: torch.Tensor):
    """(model, row, column) triples and values per batch from ``torch.nonzero`` (it synchronises to size its
    output) and a gather."""
    B = eng.batch_size
    out = []
    for i in range(0, pool.shape[0], B):
        eng._encode_only(pool[i:i + B])
        idx = torch.nonzero(eng.c > 0)
        out.append((idx, eng.c[idx[:, 0], idx[:, 1], idx[:, 2]].float()))
    return out


def torch_csr(eng: FusedSAEEnsemble, pool: torch.Tensor):
    B = eng.batch_size
    out = []
    for i in range(0, pool.shape[0], B):
        eng._encode_only(pool[i:i + B])
        out.append([eng.c[g].float().to_sparse_csr() for g in range(eng.n_models)])
    return out


def kernel_times(c: torch.Tensor, reps: int):
    """Microseconds per launch of the two kernels on the codes ``c``, from device events around ``reps``
    back-to-back launches (median of five such windows)."""
    G, B, n = c.shape
    nnz = torch.empty(G, B, device=c.device, dtype=torch.int32)
    rp = torch.zeros(G, B + 1, device=c.device, dtype=torch.int64)
    sc_ops.code_row_counts(c, nnz)
    sc_ops.extend_row_ptr(rp, nnz, 0)
    cap = int(rp[:, -1].max())
    col = torch.zeros(G, cap, device=c.device, dtype=torch.int32)
    val = torch.zeros(G, cap, device=c.device)
    out = {}
    for name, fn in (("code_row_counts", lambda: sc_ops.code_row_counts(c, nnz)),
                     ("code_compact", lambda: sc_ops.code_compact(c, rp, col, val, 0))):
        fn()
        windows = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            windows.append(a.elapsed_time(b) * 1e3 / reps)
        out[name] = round(statistics.median(windows), 2)
    out["bytes_read"] = c.numel() * 2
    out["entries"] = int(rp[:, -1].sum())
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", type=int, default=8)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--pool_batches", type=int, default=64)
    ap.add_argument("--l0", type=float, default=24.0)
    ap.add_argument("--budget", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel_reps", type=int, default=50)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("sparse_codes_bench needs the GPU: there is no CPU timing of this path")
    dev = "cuda:0"
    torch.manual_seed(0)
    G, d, n, B = args.models, args.d, args.n, args.batch
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
        eng.encode_sparse(pool[: 2 * B])  # warm
        torch.cuda.synchronize()
        eng.encode_sparse(pool, budget=args.budget)
        eng.encode_sparse(pool)
        torch.cuda.synchronize()
        print(json.dumps({"profiled": "encode_sparse", "budget": args.budget,
                          "l0": [round(float(v), 1) for v in l0]}))
        return

    paths = {
        "encode_only": lambda: encode_only(eng, pool),
        f"encode_sparse_budget{args.budget}": lambda: eng.encode_sparse(pool, budget=args.budget),
        "encode_sparse_exact": lambda: eng.encode_sparse(pool),
        "torch_nonzero": lambda: torch_nonzero(eng, pool),
        "torch_to_sparse_csr": lambda: torch_csr(eng, pool),
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

    # the routes computed the same thing
    exact, roomy = keep["encode_sparse_exact"], keep[f"encode_sparse_budget{args.budget}"]
    nnz = exact.nnz()
    tn_counts = torch.stack([torch.bincount(idx[:, 0], minlength=G) for idx, _ in keep["torch_nonzero"]]).sum(0)
    g0 = torch.cat([v[idx[:, 0] == 0] for idx, v in keep["torch_nonzero"]])
    same = {"budget_vs_exact_row_ptr": bool(torch.equal(exact.row_ptr, roomy.row_ptr)),
            "budget_vs_exact_entries": bool(torch.equal(exact.col, roomy.col[:, :exact.cap])
                                            and torch.equal(exact.val, roomy.val[:, :exact.cap])),
            "budget_overflowed": bool(roomy.overflow().any()),
            "torch_nonzero_counts": bool(torch.equal(tn_counts, nnz)),
            "torch_nonzero_values_model0": bool(torch.equal(g0, exact.val[0, :int(nnz[0])]))}
    med = {k: statistics.median(v) for k, v in times.items()}
    floor = med["encode_only"]
    eng._encode_only(pool[:B])
    print(json.dumps({
        "shape": {"G": G, "d": d, "n": n, "B": B, "pool_rows": N, "budget": args.budget},
        "l0": [round(float(v), 1) for v in l0], "reps": args.reps,
        "entries_per_model": nnz.tolist(),
        "bytes": {"dense_bf16_pool": G * N * n * 2, "sparse_pairs_pool": int(nnz.sum()) * 8 + G * (N + 1) * 8},
        "raw_ms": {k: [round(t, 3) for t in v] for k, v in times.items()},
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "per_batch_us": {k: round(v * 1e3 / args.pool_batches, 1) for k, v in med.items()},
        "over_floor_per_batch_us": {k: round((v - floor) * 1e3 / args.pool_batches, 1) for k, v in med.items()},
        "speedup_vs_torch_nonzero": {k: round(med["torch_nonzero"] / med[k], 2) for k in med if "sparse_" in k},
        "kernel_us": kernel_times(eng.c, args.kernel_reps),
        "agrees": same}))


if __name__ == "__main__":
    main()
