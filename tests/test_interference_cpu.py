"""Expected interference without a GPU: the fp64 oracle against the dense reference formula, the dense
formula against a hand-computed case, the low-rank static capacity against the [n, n] formula, the
``Interference`` result type, and the properties the GPU tests rely on in the fixtures of
``interference_cases.py``."""

import math

import pytest
import torch

import interference_cases as C
from sparse_coding__amd.engine import interference as ic
from sparse_coding__amd.engine.sparse_codes import sparse_codes_reference
from sparse_coding__amd.eval import metrics as M


def _pow2(t):
    """Every element of ``t`` (> 0) is a power of two."""
    m, _ = torch.frexp(t.double())
    return bool((t > 0).all()) and bool((m == 0.5).all())


# ----------------------------------------------------------------------------- oracle vs the dense formula
@pytest.mark.parametrize("n,d", [(48, 32), (128, 96)])
def test_oracle_matches_dense_formula(n, d):
    gen = torch.Generator().manual_seed(n + d)
    D = torch.randn(C.G, n, d, generator=gen, dtype=torch.float64)
    D[:, 3] *= 1e-3  # (norms far from 1: the formula normalises)
    codes = torch.rand(C.G, 64, n, generator=gen, dtype=torch.float64)
    codes = torch.where(torch.rand(C.G, 64, n, generator=gen) < 0.15, codes, torch.zeros_like(codes))
    codes[:, 0] = 0
    codes[:, 1] = torch.rand(C.G, n, generator=gen, dtype=torch.float64) + 0.1
    codes[:, :, 5] = 0  # a feature that never fires reads 0
    codes = codes.float().double()  # (SparseCodes stores fp32 values)
    sc = sparse_codes_reference([codes])
    ref = ic.active_capacity_reference(sc, D)
    assert not ref.skipped.any()
    got = M.expected_interference(sc, D)
    assert isinstance(got, ic.Interference) and got.n_rows == 64
    for g in range(C.G):
        want = M.calc_expected_interference(D[g], codes[g])
        assert torch.equal(got.count[g], torch.count_nonzero(codes[g], dim=0))
        # every entry is rounded to a multiple of 2^-32: at most 2^-33 each, so 2^-33 on their mean
        assert float((got.expected[g] - want).abs().max()) <= 1e-12 + 2.0 ** -33
        assert float(got.expected[g, 5]) == 0.0 and float(want[5]) == 0.0
        # the per-entry capacities are the dense ones
        dense_cap = codes[g] / torch.clamp(codes[g] @ _cos2(D[g]).T, min=1e-8)
        k = int(sc.nnz()[g])
        rows = sc.entry_rows(g)
        assert float((ref.entry_cap[g, :k] - dense_cap[rows, sc.col[g, :k].long()]).abs().max()) <= 1e-12


def _cos2(D):
    Dn = D / D.norm(dim=-1, keepdim=True).clamp(min=1e-8)
    return (Dn @ Dn.T) ** 2


def test_dense_formula_by_hand():
    """Atoms e0, e0 (a duplicate), (e0 + e1) / sqrt(2), e2: cos^2 = [[1, 1, 1/2, 0], [1, 1, 1/2, 0],
    [1/2, 1/2, 1, 0], [0, 0, 0, 1]]."""
    D = torch.tensor([[2.0, 0, 0], [0.5, 0, 0], [3.0, 3.0, 0], [0, 0, 1.0]], dtype=torch.float64)
    batch = torch.tensor([[1.0, 1.0, 0.0, 0.0],     # totals 2, 2, 1, 0     -> capacities 1/2, 1/2, 0, 0
                          [2.0, 0.0, 4.0, 1.0],     # totals 4, 4, 5, 1     -> 1/2, 0, 4/5, 1
                          [0.0, 0.0, 0.0, 0.0],     # nothing fires
                          [0.0, 2.0, 2.0, 0.0]],    # totals 3, 3, 3, 0     -> 0, 2/3, 2/3, 0
                         dtype=torch.float64)
    want = torch.tensor([(0.5 + 0.5) / 2, (0.5 + 2 / 3) / 2, (0.8 + 2 / 3) / 2, 1.0], dtype=torch.float64)
    got = M.calc_expected_interference(D, batch)
    assert float((got - want).abs().max()) < 1e-14
    # a feature that never fires divides by the clamped count
    assert float(M.calc_expected_interference(D, batch[2:3]).abs().max()) == 0.0
    # the sparse route on the same numbers
    sp = M.expected_interference(sparse_codes_reference([batch.unsqueeze(0)]), D.unsqueeze(0))
    assert float((sp.expected[0] - want).abs().max()) <= 2.0 ** -33 + 1e-14
    assert sp.count[0].tolist() == [2, 2, 2, 1]


# ----------------------------------------------------------------------------- static capacity
def test_lowrank_capacity_matches_the_square_formula():
    gen = torch.Generator().manual_seed(5)
    D = torch.randn(C.G, 96, 24, generator=gen, dtype=torch.float64)

    def square(A):
        sq = (A @ A.T) ** 2
        return torch.diagonal(sq) / sq.sum(-1)

    got = M.capacity_per_feature_lowrank(D)
    assert got.dtype == torch.float64 and tuple(got.shape) == (C.G, 96)
    for g in range(C.G):
        assert float((got[g] - square(D[g])).abs().max()) <= 1e-12
        assert float((M.capacity_per_feature_lowrank(D[g]) - square(D[g])).abs().max()) <= 1e-12
    live = [96, 40, 1]
    got = M.capacity_per_feature_lowrank(D, live)
    for g, k in enumerate(live):
        assert float((got[g, :k] - square(D[g, :k])).abs().max()) <= 1e-12
        assert not got[g, k:].any()
    assert float((M.capacity_per_feature_lowrank(D[1], 40)[:40] - square(D[1, :40])).abs().max()) <= 1e-12
    # fp32 / bf16 inputs are read in fp64; an all-zero atom reads 0
    Db = D.to(torch.bfloat16)
    Db[0, 7] = 0
    got = M.capacity_per_feature_lowrank(Db)
    assert float(got[0, 7]) == 0.0
    keep = [i for i in range(96) if i != 7]
    assert float((got[0, keep] - square(Db[0].double())[keep]).abs().max()) <= 1e-12


# ----------------------------------------------------------------------------- the result type
def _result(seed, n_rows=64, n=48, d=32):
    gen = torch.Generator().manual_seed(seed)
    D = torch.randn(C.G, n, d, generator=gen).to(torch.bfloat16)
    codes = torch.relu(torch.randn(C.G, n_rows, n, generator=gen) - 1.0)
    return D, codes


def test_interference_merge_save_load_check(tmp_path):
    D, codes = _result(3, n_rows=96)
    whole = M.expected_interference(sparse_codes_reference([codes]), D)
    a = M.expected_interference(sparse_codes_reference([codes[:, :32]]), D)
    b = M.expected_interference(sparse_codes_reference([codes[:, 32:]]), D)
    for merged in (a.merge(b), b.merge(a)):
        assert merged.n_rows == 96
        for k in ("qsum", "count", "skipped", "capacity"):
            assert torch.equal(getattr(merged, k), getattr(whole, k)), k
    assert whole.check() is whole
    exp, capacity, count = whole.per_model(1)
    assert torch.equal(exp, whole.expected[1]) and torch.equal(capacity, whole.capacity[1])
    assert torch.equal(count, whole.count[1])
    assert whole.expected.dtype == torch.float64 and float(whole.expected.max()) <= 1.0
    path = tmp_path / "interference.pt"
    whole.save(path)
    back = ic.Interference.load(path)
    assert back.n_rows == whole.n_rows
    for k in ("qsum", "count", "skipped", "capacity"):
        x, y = getattr(back, k), getattr(whole, k)
        assert x.dtype == y.dtype and torch.equal(x, y), k
    with pytest.raises(ValueError):
        whole.merge(M.expected_interference(sparse_codes_reference([codes[:, :, :40]]), D[:, :40]))
    with pytest.raises(ValueError):
        ic.check_state("no state", C.G, 48)


def test_skipped_rows_are_counted_and_check_raises():
    D, codes = _result(4)
    full = sparse_codes_reference([codes])
    ref = ic.active_capacity_reference(full, D)
    cap = int(full.row_ptr[0, 40])  # model 0: rows 0 .. 39 fit exactly
    short = sparse_codes_reference([codes], cap=cap)
    got = ic.active_capacity_reference(short, D)
    fits = short.row_ptr[:, 1:] <= cap
    assert torch.equal(got.skipped, (~fits).sum(1)) and int(got.skipped[0]) == 64 - 40
    for g in range(C.G):  # the rows that fit are exact, the others contribute nothing
        k = int(short.row_ptr[g][:-1][~fits[g]].min()) if bool((~fits[g]).any()) else int(short.nnz()[g])
        assert torch.equal(got.entry_cap[g, :k], ref.entry_cap[g, :k]) and not got.entry_cap[g, k:].any()
        assert int(got.count[g].sum()) == k
    res = M.expected_interference(short, D)
    with pytest.raises(ic.InterferenceSkipped):
        res.check()
    # a column outside [0, n), or outside the live atoms, skips that row only
    bad = sparse_codes_reference([codes])
    e = int(bad.row_ptr[1, 7])
    assert int(bad.row_ptr[1, 8]) > e
    bad.col[1, e] = 48
    got = ic.active_capacity_reference(bad, D)
    assert got.skipped.tolist() == [0, 1, 0]
    lo, hi = int(bad.row_ptr[1, 7]), int(bad.row_ptr[1, 8])
    assert not got.entry_cap[1, lo:hi].any()
    assert torch.equal(got.entry_cap[1, :lo], ref.entry_cap[1, :lo])
    assert torch.equal(got.entry_cap[1, hi:], ref.entry_cap[1, hi:])
    masked = ic.active_capacity_reference(full, D, nactive=[48, 20, 48])
    rows_hit = sum(bool((full.row(1, i)[0] >= 20).any()) for i in range(64))
    assert masked.skipped.tolist() == [0, rows_hit, 0] and rows_hit > 0
    # row windows add up
    a = ic.active_capacity_reference(full, D, row0=0, n_rows=20)
    b = ic.active_capacity_reference(full, D, row0=20)
    assert torch.equal(a.qsum + b.qsum, ref.qsum) and torch.equal(a.count + b.count, ref.count)


# ----------------------------------------------------------------------------- the fixtures' own properties
@pytest.mark.parametrize("n,d", C.SHAPES)
def test_planted_fixture_is_exact(n, d):
    D, codes, units = C.planted(n, d)
    assert D.dtype == torch.bfloat16 and tuple(D.shape) == (C.G, n, d) and tuple(codes.shape) == (C.G, C.B, n)
    Dd = D.double()
    norm2 = (Dd * Dd).sum(-1)
    assert _pow2(norm2) and len(set(norm2[0].tolist())) >= 3
    cos2 = (Dd @ Dd.transpose(1, 2)) ** 2 / (norm2.unsqueeze(2) * norm2.unsqueeze(1))
    assert set(cos2.unique().tolist()) == {0.0, 0.25, 1.0}
    assert _pow2(codes[codes > 0])
    sc = sparse_codes_reference([codes])
    ref = ic.active_capacity_reference(sc, D)
    assert not ref.skipped.any()
    lens = sc.row_ptr[:, 1:] - sc.row_ptr[:, :-1]
    for g in range(C.G):
        assert lens[g, :10].tolist() == list(C.PLANTED_L) + [n]
        k = int(sc.nnz()[g])
        assert _pow2(ref.entry_total[g, :k])
        q = ref.entry_cap[g, :k] * 2.0 ** 32
        assert torch.equal(q, q.round()) and float(ref.entry_cap[g, :k].max()) <= 1.0
        assert torch.equal(ref.entry_cap[g, :k].float().double(), ref.entry_cap[g, :k])  # fp32 holds them
        # the capacities seen: 1 (alone), 1/2 (star or pair), smaller powers of two (larger class subsets)
        assert {1.0, 0.5, 0.25} <= set(ref.entry_cap[g, :k].unique().tolist())
        # star A: columns 0 and n - 1, first and last entry; across the tile boundaries in rows 4 and 7
        a = C.star_a(n)
        assert float(cos2[g, 0, n - 1]) == 0.25 and float(cos2[g, n - 2, n - 1]) == 0.25
        for r, at in ((4, 15), (7, 31)):
            cols, _ = sc.row(g, r)
            assert int(cols[0]) == 0 and int(cols[-1]) == n - 1
            assert (int(cols[at]), int(cols[at + 1])) == (n - 2, n - 1) and set(a) <= set(cols.tolist())
        assert set(a) | set(C.STAR_B) <= set(sc.row(g, 2)[0].tolist())  # the 15-entry row holds both stars
    assert int(lens.max()) == n


@pytest.mark.parametrize("n,d", C.SHAPES)
def test_random_fixture_overlaps_everywhere(n, d):
    D, codes = C.random_case(n, d)
    assert C.min_offdiag_cos2(D) >= 0.1
    lens = (codes > 0).sum(-1)
    assert not lens[:, 0].any() and bool((lens[:, 1] == n).all())
    dens = float(lens[:, 2:].double().mean()) / n
    assert 0.07 < dens < 0.13
    # leaving one pair out of a total (for every entry: its partner with the largest cos^2 c_b; a pair with
    # a code of 0.01 weighs next to nothing by itself) moves the capacity by far more than the bound allows
    sc = sparse_codes_reference([codes])
    ref = ic.active_capacity_reference(sc, D)
    bound = C.entry_bound(ref, d)
    Dn = D.double() / D.double().norm(dim=-1, keepdim=True)
    for r in (1, 2, C.B - 1):  # the all-active row and two ordinary ones
        cols, c = sc.row(0, r)
        lo = int(sc.row_ptr[0, r])
        j = cols.long()
        terms = (Dn[0, j] @ Dn[0, j].T) ** 2 * c.double()
        terms.fill_diagonal_(0.0)
        total = ref.entry_total[0, lo:lo + j.numel()]
        moved = c.double() / (total - terms.max(dim=1).values) - c.double() / total
        ratio = float((moved / bound[0, lo:lo + j.numel()]).min())
        print(f"n = {n}, d = {d}, row {r} ({j.numel()} entries): smallest move / bound = {ratio:.3g}")
        assert ratio > 10.0, r


@pytest.mark.parametrize("d", [128, 512])
def test_fp32_emulation_stays_inside_the_bound(d):
    """The kernel's arithmetic emulated on the CPU (fp32 Gram and norms from the bf16 operands, fp32 after
    that) against the fp64 oracle, per entry, in units of ``entry_bound``."""
    n = 128
    D, codes = C.random_case(n, d, seed=1)
    sc = sparse_codes_reference([codes])
    ref = ic.active_capacity_reference(sc, D)
    bound = C.entry_bound(ref, d)
    Df = D.float()
    norm2 = (Df * Df).sum(-1).clamp(min=1e-16)
    worst = 0.0
    for g in range(C.G):
        for r in range(C.B):
            cols, c = sc.row(g, r)
            if not cols.numel():
                continue
            j = cols.long()
            gram = Df[g, j] @ Df[g, j].T
            cos2 = gram * gram / (norm2[g, j].unsqueeze(1) * norm2[g, j].unsqueeze(0))
            cos2.fill_diagonal_(1.0)
            cap = c / (cos2 @ c).clamp(min=1e-8)
            lo, hi = int(sc.row_ptr[g, r]), int(sc.row_ptr[g, r + 1])
            worst = max(worst, float(((cap.double() - ref.entry_cap[g, lo:hi]).abs() / bound[g, lo:hi]).max()))
    print(f"fp32 emulation, d = {d}: largest error / bound = {worst:.3g}")
    assert worst < 1.0
    assert math.isfinite(worst)


# ----------------------------------------------------------------------------- the trainer's torch path
def test_trainer_torch_path_and_refusals():
    from sparse_coding__amd.engine.trainer import EnsembleTrainer
    from sparse_coding__amd.models.signatures import FunctionalReverseSAE, FunctionalSAE, FunctionalTiedSAE

    torch.manual_seed(0)
    rows = torch.randn(48, 16)
    for sig, kind in ((FunctionalSAE, "untied"), (FunctionalTiedSAE, "tied")):
        models = [sig.init(16, 32, l1) for l1 in (1e-4, 1e-3)]
        for engine in ("analytic", "eager"):
            tr = EnsembleTrainer(models, sig, batch_size=16, device="cpu", engine=engine)
            got = tr.interference(rows)
            assert isinstance(got, ic.Interference) and got.n_rows == 48 and not got.skipped.any()
            codes = tr.encode_sparse(rows)
            dicts = torch.stack([ld.get_learned_dict().detach().float() for ld in tr.impl.to_learned_dicts("cpu")])
            for g in range(2):
                want = M.calc_expected_interference(dicts[g].double(), codes.to_dense(g).double())
                assert float((got.expected[g] - want).abs().max()) <= 1e-12 + 2.0 ** -33
                sq = (dicts[g].double() @ dicts[g].double().T) ** 2
                assert float((got.capacity[g] - torch.diagonal(sq) / sq.sum(-1)).abs().max()) <= 1e-10
            # chunk by chunk through state= gives the bits of one call
            part = tr.interference(rows[32:], state=tr.interference(rows[:32]))
            assert part.n_rows == 48 and torch.equal(part.qsum, got.qsum) and torch.equal(part.count, got.count)
            # a budget that is too small: rows are skipped and check() raises
            short = tr.interference(rows, budget=1)
            assert bool(short.skipped.any())
            with pytest.raises(ic.InterferenceSkipped):
                short.check()
    models = [FunctionalSAE.init(16, 32, 1e-3) for _ in range(2)]
    es = EnsembleTrainer(models, FunctionalSAE, batch_size=16, device="cpu", parallel="es")
    try:
        got = es.interference(rows)
    finally:
        es.close()
    want = EnsembleTrainer(models, FunctionalSAE, batch_size=16, device="cpu").interference(rows)
    assert torch.equal(got.qsum, want.qsum) and torch.equal(got.count, want.count)
    for par in ("dp", "zero1"):
        tr = EnsembleTrainer(models, FunctionalSAE, batch_size=16, device="cpu", engine="eager", parallel=par)
        try:
            with pytest.raises(NotImplementedError, match="data-parallel"):
                tr.interference(rows)
        finally:
            tr.close()
    models = [FunctionalReverseSAE.init(16, 32, 1e-3) for _ in range(2)]
    tr = EnsembleTrainer(models, FunctionalReverseSAE, batch_size=16, device="cpu")
    with pytest.raises(NotImplementedError, match="FunctionalReverseSAE"):
        tr.interference(rows)


def test_engine_refusals_need_no_gpu():
    """The fused engine's kind checks, on an object that carries only the fields they read."""
    from sparse_coding__amd.engine.fused import FusedSAEEnsemble

    eng = object.__new__(FusedSAEEnsemble)
    for kind, learned, word in (("threshold", False, "threshold"), ("reverse", False, "reverse"),
                                ("tied", True, "learned centering")):
        eng.kind, eng.learned_center = kind, learned
        with pytest.raises(NotImplementedError, match=word):
            eng.interference(torch.zeros(128, 256))


def test_front_end_validates_before_the_library():
    from sparse_coding__amd.ops import interference as ic_ops

    D = torch.zeros(2, 8, 32, dtype=torch.bfloat16)
    rp = torch.zeros(2, 5, dtype=torch.int64)
    col, val = torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 4)
    n2, q, c, s = torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, 8, dtype=torch.int64), \
        torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="bf16"):
        ic_ops.row_norm2(D.float())
    with pytest.raises(ValueError, match="d % 32"):
        ic_ops.row_norm2(torch.zeros(2, 8, 48, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="row_ptr holds"):
        ic_ops.active_capacity(rp, col, val, D, n2, q, c, s, row0=2, n_rows=4)
    with pytest.raises(ValueError, match="qsum"):
        ic_ops.active_capacity(rp, col, val, D, n2, q.int(), c, s)
    with pytest.raises(ValueError, match="entry_cap"):
        ic_ops.active_capacity(rp, col, val, D, n2, q, c, s, entry_cap=torch.zeros(2, 3))
    with pytest.raises(ValueError, match="nactive"):
        ic_ops.active_capacity(rp, col, val, D, n2, q, c, s, nactive=torch.zeros(2, dtype=torch.int64))
