"""Time the whole-dictionary ridge probes of an ensemble on the GPU.

Steps over the sparse codes of one pool, alternated, each timed with a host clock around work that ends in a device
synchronise:

``fit``             ``SparseCodes.ridge_probes`` whole: the two ``check()`` synchronisations, ``by_feature``, the
                    CGLS loop (``--max_iter``), the scores and the exact AUROC of both row sets
``solve_1`` / ``solve_9``   the solver alone (``engine.probe._cgls`` on the kernels) with 1 and 9 iterations;
                    ``iteration`` = their difference / 8
``rows_matmul`` / ``lists_matmul`` / ``col_dots`` / ``axpby``   each op alone on operands of the loop's shapes
``torch_1`` / ``torch_9``   the same recurrence on ``torch.sparse`` CSR matmuls (``SparseCodes.to_torch_csr`` and its
                    transpose, one model at a time; fp32 torch vector updates, fp64 sums): the route a user could
                    assemble without the kernels; ``torch_iteration`` = their difference / 8
``torch_rows`` / ``torch_lists``   its two products alone
``lists_seg<S>``    ``lists_matmul`` on the pool's own lists for segments of S entries (``--segments``)
``worst_seg<S>`` / ``worst_unsegmented``   ``lists_matmul`` on a planted pool whose model 0 holds one feature that
                    fires on every second row and nothing else, for segments of S entries and for one segment per
                    list

Concept k marks a random ``2^-(1 + k % 6)`` of the rows from a fixed seed; a quarter of the rows is held out.  The
shape is the feature-stats bench's (G = 8, d = 512, n = 2048, B = 2048, 64 pool batches, biases shifted to about
``--l0`` features per row, ``budget=64``).  Prints one JSON line.

    python scripts/probes_bench.py
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

from interference_bench import build_sae
from sparse_coding__amd.engine import probe as pb
from sparse_coding__amd.engine.feature_codes import FeatureCodes
from sparse_coding__amd.engine.value_order import concept_words
from sparse_coding__amd.ops import probe as pr


class TorchSparseOps:
    """The operator of ``engine.probe._cgls`` on ``torch.sparse`` CSR matmuls, one model at a time."""

    def __init__(self, sc, fit, dtype=torch.float32):
        self.dtype = dtype
        self.C = [sc.to_torch_csr(g).to(dtype) for g in range(sc.n_models)]
        self.CT = [c.to_sparse_coo().t().to_sparse_csr() for c in self.C]
        self.m = fit.to(dtype).view(1, -1, 1)
        nfit = fit.sum().double()
        ones = fit.to(dtype).unsqueeze(1)
        self.mu = torch.stack([(ct @ ones)[:, 0] for ct in self.CT]).double().div(nfit).to(dtype).unsqueeze(-1)

    def scalar(self, x):
        return x.to(torch.float64)

    def rows(self, v):
        return torch.stack([c @ v[g] for g, c in enumerate(self.C)])

    def lists(self, u):
        return torch.stack([c @ u[g] for g, c in enumerate(self.CT)])

    def forward(self, v):
        return (self.rows(v) - (self.mu * v).sum(1, keepdim=True)) * self.m

    def adjoint(self, u, w, alpha):
        return self.lists(u) - self.mu * u.sum(1, keepdim=True) - alpha * w

    def dots(self, a, b):
        return (a * b).sum(1, dtype=torch.float64)

    def axpby_(self, y, x, a, b):
        return y.mul_(b.to(self.dtype).unsqueeze(1)).addcmul_(x, a.to(self.dtype).unsqueeze(1))


def worst_case(fc):
    """``fc`` with model 0 holding one list of every second row (feature 0) and no other."""
    N = fc.n_rows
    half = N // 2
    col_ptr, row, val = fc.col_ptr.clone(), fc.row.clone(), fc.val.clone()
    if fc.cap < half:
        raise SystemExit("the buffers are shorter than half the pool: no room for the planted list")
    col_ptr[0, 1:] = half
    row[0, :half] = torch.arange(0, 2 * half, 2, device=row.device, dtype=torch.int32)
    val[0, :half] = 1.0 + (torch.arange(half, device=row.device) % 7).float() / 8
    row[0, half:], val[0, half:] = 0, 0.0
    return FeatureCodes(N, fc.n, col_ptr, row, val, fc.skipped)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", type=int, default=8)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--pool_batches", type=int, default=64)
    ap.add_argument("--l0", type=float, default=24.0)
    ap.add_argument("--budget", type=int, default=64)
    ap.add_argument("--concepts", type=int, default=32)
    ap.add_argument("--max_iter", type=int, default=64)
    ap.add_argument("--segments", default="128,256,512,1024,2048,4096,8192")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="", help="comma-separated steps to run (default: all)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("probes_bench needs the GPU: there is no CPU timing of this path")
    dev = "cuda:0"
    torch.manual_seed(0)
    eng, pool, _, _ = build_sae(args, dev)
    sc = eng.encode_sparse(pool, budget=args.budget).check()
    nactive = getattr(eng, "nactive", None)
    G, N, n, K = sc.n_models, sc.n_rows, sc.n, args.concepts
    gen = torch.Generator().manual_seed(args.seed)
    rate = torch.tensor([2.0 ** -(1 + k % 6) for k in range(32)])
    bits = torch.rand(N, K, generator=gen) < rate[:K]
    flags = concept_words(bits).to(dev)
    fit = (torch.rand(N, generator=gen) < 0.75).to(dev)

    fc = sc.by_feature(nactive).check()
    kops = pb._KernelOps(sc, fc, fit, pb._nactive(nactive, sc), None)
    tops = TorchSparseOps(sc, fit)
    yc = pb._pad(pb._targets(bits.to(dev), fit, torch.float64)[1].float()).unsqueeze(0).expand(G, -1, -1).contiguous()
    P = torch.randn(G, n, 32, device=dev)
    R = torch.randn(G, N, 32, device=dev) * fit.view(1, N, 1)
    y = torch.randn(G, N, 32, device=dev)
    coef = torch.rand(G, 32, device=dev, dtype=torch.float64)
    worst = worst_case(fc)
    segments = [int(x) for x in args.segments.split(",")]
    plans = {s: pr.lists_plan(worst.col_ptr, worst.cap, s) for s in segments}
    own = {s: pr.lists_plan(fc.col_ptr, fc.cap, s) for s in segments}
    plans["unsegmented"] = pr.lists_plan(worst.col_ptr, worst.cap, 2 ** 30)

    def solve(ops, iters):
        return pb._cgls(ops, yc, n, 1.0, iters, 1e-5)[0]

    steps = {
        "fit": lambda: sc.ridge_probes(flags, K, fit_rows=fit, max_iter=args.max_iter, nactive=nactive),
        "solve_1": lambda: solve(kops, 1),
        "solve_9": lambda: solve(kops, 9),
        "rows_matmul": lambda: kops.forward(P),
        "lists_matmul": lambda: kops.lists(R),
        "col_dots": lambda: pr.col_dots(R, R),
        "axpby": lambda: pr.axpby_(y, R, coef, coef),
        "torch_1": lambda: solve(tops, 1),
        "torch_9": lambda: solve(tops, 9),
        "torch_rows": lambda: tops.rows(P),
        "torch_lists": lambda: tops.lists(R),
    }
    for s, plan in own.items():
        steps[f"lists_seg{s}"] = lambda plan=plan: pr.lists_matmul(fc.col_ptr, fc.row, fc.val, R, plan=plan)
    for s, plan in plans.items():
        name = f"worst_seg{s}" if isinstance(s, int) else "worst_unsegmented"
        steps[name] = lambda plan=plan: pr.lists_matmul(worst.col_ptr, worst.row, worst.val, R, plan=plan)
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

    med = {k: statistics.median(v) for k, v in times.items()}
    agrees = {}
    if "rows_matmul" in steps and "torch_rows" in steps:
        a, b = pr.rows_matmul(kops.row_ptr, sc.col, sc.val, P)[0], tops.rows(P)
        agrees["rows_max_abs_diff"] = float((a - b).abs().max())
    if "lists_matmul" in steps and "torch_lists" in steps:
        agrees["lists_max_abs_diff"] = float((kops.lists(R) - tops.lists(R)).abs().max())
    if not args.only:  # the converged weights of the three routes, against the torch.sparse route in fp64
        w64 = pb._cgls(TorchSparseOps(sc, fit, torch.float64), yc.double(), n, 1.0, args.max_iter, 1e-5)[0]
        for name, w in (("kernels", solve(kops, args.max_iter)), ("torch_fp32", solve(tops, args.max_iter))):
            agrees[f"w_{name}_vs_torch_fp64_rel"] = float((w.double() - w64).abs().max() / w64.abs().max())
    if "worst_unsegmented" in last and f"worst_seg{pr.PROBE_SEG}" in last:
        a, b = last["worst_unsegmented"], last[f"worst_seg{pr.PROBE_SEG}"]
        agrees["worst_rel_diff"] = float((a - b).abs().max() / a.abs().max())
    out = {
        "shape": {"G": G, "d": args.d, "n": n, "B": args.batch, "pool_rows": N, "budget": args.budget, "K": K},
        "entries_per_model": sc.nnz().tolist(), "reps": args.reps, "probe_seg": pr.PROBE_SEG,
        "longest_list": fc.counts().max(1).values.tolist(),
        "raw_ms": {k: [round(t, 3) for t in v] for k, v in times.items()},
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "spread_ms": {k: round(max(v) - min(v), 3) for k, v in times.items()},
        "agrees": agrees,
    }
    if "fit" in last:
        res = last["fit"]
        a = res.auroc()
        out["fit"] = {"iters_max": int(res.iters.max()), "converged": int(res.converged.sum()), "of": G * K,
                      "auroc_range": [float(a[~a.isnan()].min()), float(a[~a.isnan()].max())]}
    if "solve_1" in med and "solve_9" in med:
        out["iteration_ms"] = round((med["solve_9"] - med["solve_1"]) / 8, 3)
    if "torch_1" in med and "torch_9" in med:
        out["torch_iteration_ms"] = round((med["torch_9"] - med["torch_1"]) / 8, 3)
    if "iteration_ms" in out and "torch_iteration_ms" in out:
        out["torch_over_kernels"] = round(out["torch_iteration_ms"] / out["iteration_ms"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
