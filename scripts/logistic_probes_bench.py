"""Time the whole-dictionary logistic probes of an ensemble on the GPU.

Steps over the sparse codes of one pool, alternated, each timed with a host clock around work that ends in a device
synchronise:

``fit`` / ``fit_no_early_stop``   ``SparseCodes.logistic_probes`` whole, with the one bool per outer step read to the
                    host and without: the two ``check()`` synchronisations, ``by_feature``, the Newton-CG loop, the
                    logits and the exact AUROC of both row sets
``hess_1`` / ``hess_9``   1 and 9 Hessian products (``rows_matmul(scale=D)``, ``lists_matmul``, the column sums and the
                    centring arithmetic); ``hessian_product`` = their difference / 8
``rows_scaled`` / ``rows_then_mul``   the fused ``rows_matmul(scale=D)`` against ``rows_matmul`` and a torch multiply
``logit_terms`` / ``torch_logit``   ``sc_probe_logit`` against the same terms in torch (fp32 sigmoid, fp64 loss sums)
``line_losses`` / ``torch_line``    ``sc_probe_line`` against eight torch evaluations of the loss sums
``sklearn``         ``LogisticRegression(C)`` on the dense fp32 codes of model 0 for concept 0, on the host, for
                    scale: once with its defaults and once with ``tol=1e-8, max_iter=1000``, each with the largest
                    weight difference to the device fit; left out with ``--no_sklearn``

The pool, the concepts and the held-out quarter are those of ``probes_bench.py`` (G = 8, d = 512, n = 2048, B = 2048,
64 pool batches).  Prints one JSON line and writes it, with a table, under ``--out``.

    python scripts/logistic_probes_bench.py
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
from sparse_coding__amd.engine.value_order import concept_words
from sparse_coding__amd.ops import probe as pr


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
    ap.add_argument("--C", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no_sklearn", action="store_true")
    ap.add_argument("--only", default="", help="comma-separated steps to run (default: all)")
    ap.add_argument("--out", default=os.path.join("profiles", "r26", "logistic_probes"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("logistic_probes_bench needs the GPU: there is no CPU timing of this path")
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
    mask = fit.to(torch.uint8)
    tbits = pb.concept_bits(flags, 32).float()

    fc = sc.by_feature(nactive).check()
    kops = pb._KernelLogitOps(sc, fc, fit, pb._nactive(nactive, sc), None, flags)
    P = torch.randn(G, n, 32, device=dev) * 0.05
    pb_ = torch.zeros(G, 32, device=dev, dtype=torch.float64)
    Z = kops.margins(P, pb_).clone()
    U = torch.randn(G, N, 32, device=dev)
    D = kops.terms(Z)[1].clone()
    Q = torch.empty_like(Z)
    m = fit.view(1, N, 1)

    def hess(times):
        for _ in range(times):
            out = kops.hess(D, P, pb_, 1.0 / args.C)
        return out

    def rows_then_mul():
        q, _ = pr.rows_matmul(kops.row_ptr, sc.col, sc.val, P, mask=mask, out=Q)
        return q.mul_(D)

    def torch_logit():
        p = torch.sigmoid(Z)
        r = torch.where(m, p - tbits, torch.zeros_like(p))
        return r, torch.where(m, p * (1 - p), torch.zeros_like(p)), torch_loss(Z)

    def torch_loss(z):
        z = z.double()
        return torch.where(m, torch.logaddexp(z, torch.zeros_like(z)) - tbits * z, torch.zeros_like(z)).sum(1)

    fit_kw = dict(fit_rows=fit, C=args.C, nactive=nactive)
    steps = {
        "fit": lambda: sc.logistic_probes(flags, K, **fit_kw),
        "fit_no_early_stop": lambda: sc.logistic_probes(flags, K, early_stop=False, **fit_kw),
        "hess_1": lambda: hess(1),
        "hess_9": lambda: hess(9),
        "rows_scaled": lambda: pr.rows_matmul(kops.row_ptr, sc.col, sc.val, P, mask=mask, out=Q, scale=D),
        "rows_then_mul": rows_then_mul,
        "logit_terms": lambda: pr.logit_terms(Z, flags, mask),
        "torch_logit": torch_logit,
        "line_losses": lambda: pr.line_losses(Z, U, flags, mask),
        "torch_line": lambda: torch.stack([torch_loss(Z + 2.0 ** -j * U) for j in range(pr.LINE_STEPS)], 1),
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

    med = {k: statistics.median(v) for k, v in times.items()}
    agrees = {}
    if "line_losses" in last and "torch_line" in last:
        a, b = last["line_losses"], last["torch_line"]
        agrees["line_rel_diff"] = float(((a - b).abs() / b.abs().clamp(min=1.0)).max())
    if "fit" in last and "fit_no_early_stop" in last:
        a, b = last["fit"], last["fit_no_early_stop"]
        agrees["early_stop_same_bits"] = all(torch.equal(getattr(a, k).nan_to_num(), getattr(b, k).nan_to_num())
                                             for k in a._TENSORS if getattr(a, k).is_floating_point())
    out = {
        "shape": {"G": G, "d": args.d, "n": n, "B": args.batch, "pool_rows": N, "budget": args.budget, "K": K,
                  "C": args.C},
        "entries_per_model": sc.nnz().tolist(), "reps": args.reps,
        "raw_ms": {k: [round(t, 3) for t in v] for k, v in times.items()},
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "spread_ms": {k: round(max(v) - min(v), 3) for k, v in times.items()},
        "agrees": agrees,
    }
    if "fit" in last:
        res = last["fit"]
        a = res.auroc()
        out["fit"] = {"outer_max": int(res.iters.max()), "cg_max": int(res.cg_iters.max()),
                      "converged": int(res.converged.sum()), "stalled": int(res.stalled.sum()), "of": G * K,
                      "auroc_range": [float(a[~a.isnan()].min()), float(a[~a.isnan()].max())]}
    if "hess_1" in med and "hess_9" in med:
        out["hessian_product_ms"] = round((med["hess_9"] - med["hess_1"]) / 8, 3)
    if not args.no_sklearn and not args.only:
        from sklearn.linear_model import LogisticRegression

        host = sc.to("cpu")
        X = pb._dense_codes(host, nactive, torch.float32)[0][0][fit.cpu()].numpy()
        y = bits[:, 0][fit.cpu()].numpy()
        sk = {}
        for name, kw in (("defaults", {}), ("tight", {"tol": 1e-8, "max_iter": 1000})):
            t0 = time.perf_counter()
            clf = LogisticRegression(C=args.C, **kw).fit(X, y)
            sk[name] = {"fit_s": round(time.perf_counter() - t0, 2), "iters": int(clf.n_iter_[0])}
            if "fit" in last:       # (the concepts are random: the weights are small, so the difference is absolute)
                w = last["fit"].weight[0, :, 0].cpu().double()
                coef = torch.from_numpy(clf.coef_).reshape(-1).double()
                sk[name].update(max_abs_weight_diff=float((w - coef).abs().max()),
                                max_abs_weight=float(w.abs().max()), sklearn_max_abs_weight=float(coef.abs().max()))
        out["sklearn_one_fit"] = sk
    print(json.dumps(out))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "logistic_probes_bench.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    lines = ["| step | median ms | spread ms |", "|---|---|---|"]
    lines += [f"| `{k}` | {out['median_ms'][k]} | {out['spread_ms'][k]} |" for k in out["median_ms"]]
    with open(os.path.join(args.out, "table.md"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
