"""Nearest-atom matching timing: the row-argmax kernel vs the value-only kernel vs torch.

At the two shapes of ``profiles/mmcs_bench_r1.jsonl`` (16k x 16k x 512 and 32k x 32k x 2048), for unit-norm
bf16 dictionaries: ``gemm.rowargmax_nt`` with m = 1 and m = 4, ``gemm.rowmax_nt`` (the value without the
index) and the torch route that materialises the fp32 [n1, n2] matrix and takes ``max(dim=-1)``.  Then, at
the headline ensemble (G = 8, n = 2048, d = 512), ``FusedSAEEnsemble.atom_matches()`` against
``eval.metrics.mmcs_from_list`` on the unstacked models.

Every candidate of a group is timed in 5 rounds that alternate between the candidates (one warmed window
per candidate and round, sized to about 0.3 s, ended by a device synchronise); the median and the spread
(max - min over the rounds) are reported, one JSON line per group.  ``--out FILE`` appends the lines there.
"""

from __future__ import annotations

import argparse
import json
import statistics
import time

import torch

from sparse_coding__amd.ops import gemm

ROUNDS = 5


def _window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def alternate(cands, target_s=0.3, max_reps=200):
    """{name: fn} -> {name: {"ms": median, "spread_ms": max - min, "runs": [...]}} over ROUNDS alternating rounds."""
    reps = {}
    for name, fn in cands.items():
        fn()  # warm-up: code objects, allocator
        t1 = _window(fn, 1)
        reps[name] = max(3, min(max_reps, int(target_s * 1e3 / max(t1, 1e-3))))
    runs = {name: [] for name in cands}
    for _ in range(ROUNDS):
        for name, fn in cands.items():
            runs[name].append(_window(fn, reps[name]))
    return {name: {"ms": round(statistics.median(r), 4), "spread_ms": round(max(r) - min(r), 4),
                   "runs": [round(v, 4) for v in r], "reps": reps[name]} for name, r in runs.items()}


def kernel_shapes(out):
    torch.manual_seed(0)
    for n, d in ((16384, 512), (32768, 2048)):
        a = torch.nn.functional.normalize(torch.randn(n, d, device="cuda"), dim=-1)
        b = torch.nn.functional.normalize(torch.randn(n, d, device="cuda"), dim=-1)
        ab, bb = a.to(torch.bfloat16), b.to(torch.bfloat16)
        # what is timed agrees: the kernel's value is rowmax_nt's to the bit, its column the fp32 argmax
        # up to near-ties
        val, idx = gemm.rowargmax_nt(ab, bb)
        same_bits = bool(torch.equal(val[:, 0], gemm.rowmax_nt(ab, bb)))
        ev, ei = (ab.float() @ bb.float().T).max(dim=-1)
        agree = float((idx[:, 0].long() == ei).double().mean())
        err = float((val[:, 0] - ev).abs().max())
        del ev, ei
        res = alternate({
            "rowargmax_m1": lambda: gemm.rowargmax_nt(ab, bb),
            "rowargmax_m4": lambda: gemm.rowargmax_nt(ab, bb, m=4),
            "rowmax": lambda: gemm.rowmax_nt(ab, bb),
            "torch_fp32_max": lambda: (a @ b.T).max(dim=-1),
        })
        flop = 2.0 * n * n * d
        line = {"group": "kernel", "n1": n, "n2": n, "d": d, **res,
                "rowargmax_m1_tflops": round(flop / res["rowargmax_m1"]["ms"] / 1e9, 1),
                "value_equals_rowmax_bits": same_bits, "index_agrees_with_fp32_torch": round(agree, 5),
                "max_abs_err_vs_torch": round(err, 6)}
        emit(line, out)
        del a, b, ab, bb
        torch.cuda.empty_cache()


def ensemble(out, G=8, n=2048, d=512, B=2048):
    from sparse_coding__amd.engine.fused import FusedSAEEnsemble
    from sparse_coding__amd.eval import metrics
    from sparse_coding__amd.models.signatures import FunctionalSAE

    torch.manual_seed(0)
    l1s = [10 ** (-4 + 2 * i / max(1, G - 1)) for i in range(G)]
    models = [FunctionalSAE.init(d, n, l1, device="cuda") for l1 in l1s]
    eng = FusedSAEEnsemble(models, FunctionalSAE, lr=1e-3, batch_size=B, device="cuda")
    eng.step_batch(torch.randn(B, d, device="cuda").to(torch.bfloat16))
    got = eng.atom_matches().mmcs().cpu()
    want = metrics.mmcs_from_list(eng.to_learned_dicts("cuda"))
    dev = max(abs(float(got[j, i]) - float(want[i, j])) for i in range(G) for j in range(i))
    res = alternate({
        "atom_matches_m1": lambda: eng.atom_matches(),
        "atom_matches_m1_mmcs": lambda: eng.atom_matches().mmcs(),
        "atom_matches_m4": lambda: eng.atom_matches(m=4),
        "mmcs_from_list_device": lambda: metrics.mmcs_from_list(eng.to_learned_dicts("cuda")),
        "mmcs_from_list_host": lambda: metrics.mmcs_from_list(eng.to_learned_dicts("cpu")),
    }, max_reps=50)
    emit({"group": "ensemble", "G": G, "n": n, "d": d, **res, "max_mmcs_dev_vs_fp32": round(dev, 6)}, out)


def emit(line, out):
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--skip-ensemble", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("atom_match_bench needs the GPU: nothing is measured without one")
    emit({"group": "box", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
          "hip": torch.version.hip}, args.out)
    kernel_shapes(args.out)
    if not args.skip_ensemble:
        ensemble(args.out)


if __name__ == "__main__":
    main()
