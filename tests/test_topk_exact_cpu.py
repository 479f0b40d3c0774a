"""CPU checks of the exact top-k cases (``topk_exact_cases.py``): the input bounds that make the
fp32 arithmetic order-free, each fp64 reference against a second plain-torch formulation, complete
instantiation and branch coverage of the select rows, the constants mirrored from ``topk.hip``, and
that each reference catches a deliberately wrong emulation of its kernel."""

import pytest
import torch

import topk_exact_cases as X


# ------------------------------------------------------------------ constants, dispatch, layout
def test_constants_mirror_the_kernel_source():
    got = X.parsed_constants()
    assert got == {"BR_CAP": [X.BR_CAP], "TIE_CAP": [X.TIE_CAP], "S1": [X.S1]}, got


def test_dispatch_table_covers_every_instantiation():
    for (kind, P), ns in X.SELECT_N.items():
        for n in ns:
            assert X.dispatch(kind == "bf16", n) == (kind, P), n
    assert {p for k, p in X.SELECT_N if k == "wave"} == {16, 32, 64}
    assert {p for k, p in X.SELECT_N if k == "block"} == {24, 32, 48, 64}
    assert {p for k, p in X.SELECT_N if k == "radix"} == {4, 8, 16, 24, 32, 48, 64}
    assert {p for k, p in X.SELECT_N if k == "bf16"} == {8, 16, 24, 32, 48, 64}
    for bf, ns in X.REFUSED_N.items():
        assert all(X.dispatch(bf, n) is None for n in ns)
    assert [X.decode_nv(d) for d, *_ in X.DECODE_CASES] == [1, 1, 1, 2, 2, 3, 4, 8, 8, 16, 16]
    assert {X.decode_nv(d) for d, *_ in X.DECODE_CASES} == {1, 2, 3, 4, 8, 16}
    assert all(X.decode_nv(d) is None for d in X.DECODE_REFUSED_D)


@pytest.mark.parametrize("kind,P", [("wave", 16), ("block", 24), ("bf16", 16), ("radix", 8)])
def test_layout_is_the_documented_one(kind, P):
    lay = X.layout(kind, P)
    T, V = {"wave": (64, 4), "block": (256, 4), "bf16": (256, 8), "radix": (256, 1)}[kind]
    assert lay.shape == (T, P) and torch.equal(lay.reshape(-1).sort().values, torch.arange(T * P))
    for t, s in ((0, 0), (3, 5), (T - 1, P - 1)):
        want = t + s * 256 if kind == "radix" else ((s // V) * T + t) * V + s % V
        assert int(lay[t, s]) == want
    rank = X.thread_major_rank(kind, P, T * P)
    assert torch.equal(rank[lay.reshape(-1)], torch.arange(T * P))


def test_order_keys_are_monotone():
    v = torch.tensor([-3e38, -2.0, -1e-30, 0.0, 1e-30, 0.75, 1.0, 3e38])
    for s in (v, v.to(X.BF)):
        assert bool((X.order_keys(s).diff() > 0).all())
        assert torch.equal(X.order_keys(s, absolute=True), X.order_keys(s.abs()))


# ------------------------------------------------------------------ select rows and their branches
def _tags(n, bf):
    c = X.select_case(n, bf)
    kind, P = X.dispatch(bf, n)
    keys = X.order_keys(c["scores"])
    return [X.select_branch(kind, P, keys[g, b], min(c["ks"][g], n, c["kmax"]), have_x=bf)
            for g in range(X.SEL_G) for b in range(X.SEL_B)]


def test_every_instantiation_runs_every_branch():
    for (kind, P), ns in X.SELECT_N.items():
        hit = set().union(*[t for n in ns for t in _tags(n, kind == "bf16")])
        assert X.REQUIRED_BRANCHES[kind] <= hit, (kind, P, sorted(X.REQUIRED_BRANCHES[kind] - hit))


def test_select_rows_are_what_the_recipe_says():
    c = X.select_case(4096, True)
    keys = X.order_keys(c["scores"])
    for g, k in enumerate(c["ks"][:2]):  # k <= 256: the bracket path
        t = int(torch.topk(keys[g, 2], k).values[-1])
        need, nt = k - int((keys[g, 2] > t).sum()), int((keys[g, 2] == t).sum())
        assert need < nt <= X.TIE_CAP and X.select_branch("bf16", 16, keys[g, 2], k, True) == {"resolve"}
        assert X.select_branch("bf16", 16, keys[g, 3], k, True) == {"many_ties"}
    assert bool((c["scores"][0, 3] == 0.75).sum() == 200) and bool((c["scores"][0, 3, 2000:2200] == 0.75).all())
    assert X.select_branch("bf16", 8, X.order_keys(X.select_case(8, True)["scores"])[1, 0], 8, True) == {"overflow"}
    for n in (4, 8, 1, 3):  # k == n on the tiny rows
        c = X.select_case(n, False)
        assert min(c["ks"][-1], n, c["kmax"]) == n
    c = X.select_case(16384, False)  # full bisection with a small bucket needs k > 256
    assert c["ks"][2] > 256 and "full_bucket" in X.select_branch("block", 64, X.order_keys(c["scores"])[2, 0], 300)


@pytest.mark.parametrize("n,bf", [(1024, False), (4100, False), (1023, False), (4096, True)])
def test_select_reference_accepts_the_contract_and_rejects_thread_major_ties(n, bf):
    c = X.select_case(n, bf)
    x, D = X.select_operands(n, 4, False) if bf else (None, None)
    idx, val = X.emulate_select(c["scores"], c["ks"], c["kmax"], x=x, D=D)
    X.check_select(c["scores"], c["ks"], c["kmax"], idx, val, x=x, D=D)
    if X.dispatch(bf, n)[0] == "radix":
        return  # (thread-major is this kernel's contract)
    idx, val = X.emulate_select(c["scores"], c["ks"], c["kmax"], x=x, D=D, ties="thread")
    with pytest.raises(AssertionError, match="picked set differs"):
        X.check_select(c["scores"], c["ks"], c["kmax"], idx, val, x=x, D=D)


def test_select_reference_rejects_other_wrong_results():
    c = X.select_case(1024, False)
    good = X.emulate_select(c["scores"], c["ks"], c["kmax"])

    def broken(fn):
        idx, val = good[0].clone(), good[1].clone()
        fn(idx, val)
        with pytest.raises(AssertionError):
            X.check_select(c["scores"], c["ks"], c["kmax"], idx, val)

    broken(lambda i, v: i[0, 0].__setitem__(1, int(i[0, 0, 0])))  # a duplicate
    broken(lambda i, v: v[0, 0].__setitem__(0, float(v[0, 0, 0]) + 1))  # a value that is not the score
    broken(lambda i, v: i[0, 0].__setitem__(25, 3))  # a padded slot written
    low = int(c["scores"][1, 0].argmin())
    broken(lambda i, v: (i[1, 0].__setitem__(0, low), v[1, 0].__setitem__(0, 0.0)))  # a key outside the top-k


def test_tie_order_pins():
    """bf16, n = 4096: thread 0 owns columns 0..7 and 2048..2055, so thread-major is not column order."""
    c = X.tie_order_case(True)
    keys = X.order_keys(c["scores"])[0, 0]
    assert X.select_branch("bf16", 16, keys, 150) == {"many_ties"}
    want = X.expected_picks(keys, 150, X.tie_rank("bf16", 16, 4096, {"many_ties"}))
    tied = want[(want >= 2000) & (want < 2200)]
    assert torch.equal(tied, torch.arange(2000, 2050) if X.BF16_BRACKET_TIES == "column" else torch.arange(2048, 2098))
    c = X.tie_order_case(False)  # fp32 block kernel: thread-major in the bracket, as documented
    keys = X.order_keys(c["scores"])[0, 0]
    assert X.select_branch("block", 32, keys, 150) == {"bracket"}
    want = X.expected_picks(keys, 150, X.tie_rank("block", 32, 8192, {"bracket"}))
    assert torch.equal(want[(want >= 1000) & (want < 1200)], torch.arange(1024, 1074))


def test_exact_resolve_reference():
    for n, d in [(2048, 4)] + X.RESOLVE_EXTRA:
        for per_model in (False, True):
            x, D = X.select_operands(n, d, per_model)
            e = X.exact_scores(x, D)
            assert e.shape == (X.SEL_G, X.SEL_B, n) and torch.equal(e, e.round())
            c = X.select_case(n, True)
            tags = X.check_select(c["scores"], c["ks"], c["kmax"], *X.emulate_select(c["scores"], c["ks"], c["kmax"], x=x, D=D),
                                  x=x, D=D)
            assert {"resolve"} in tags, (n, d)
            # by column instead of by exact score: caught
            with pytest.raises(AssertionError, match="picked set differs"):
                X.check_select(c["scores"], c["ks"], c["kmax"], *X.emulate_select(c["scores"], c["ks"], c["kmax"]), x=x, D=D)


# ------------------------------------------------------------------ decode and code gradient
def _decode_case(i):
    d, ks, kmax, per_model, dense_from = X.DECODE_CASES[i]
    return X.decode_inputs(3, X.DEC_B, X.DEC_N, d, ks, kmax, per_model), dense_from


def test_decode_cases_cover_the_issue():
    ks = {k for _, kv, *_ in X.DECODE_CASES for k in kv}
    assert {0, 1, 7, 8, 9, 15, 16, 17, 33, 64} <= ks
    assert any(kmax > max(kv) for _, kv, kmax, *_ in X.DECODE_CASES)
    assert {pm for *_, pm, _ in X.DECODE_CASES} == {False, True}
    assert {df for *_, df in X.DECODE_CASES} == {0, 1, 3}
    assert X.DEC_B % 4 != 0


@pytest.mark.parametrize("i", range(len(X.DECODE_CASES)))
def test_decode_reference_and_input_bounds(i):
    t, dense_from = _decode_case(i)
    d, ks, kmax = X.DECODE_CASES[i][:3]
    ref = X.decode_ref(t, dense_from)
    stats = X.check_decode(t, ref, f"d={d}")
    assert stats["max_R"] <= 256 and stats["max_se"] < X.EXACT and stats["max_dot"] < X.EXACT
    two = X.decode_ref_dense(t)
    assert all(torch.equal(ref[k], two[k]) for k in ("R", "row_se", "dot"))
    idx, val = t["idx"], t["val"]
    for g, k in enumerate(ks):
        assert not idx[g, :, k:].any() and not val[g, :, k:].any()
        assert all(idx[g, b, :k].unique().numel() == k for b in range(X.DEC_B))
        if k:
            assert int(idx[g, 0, 0]) == 0 and float(val[g, 0, 0]) > 0  # a real pick of column 0
    live = ref["live"]
    if max(ks) >= 8:
        assert bool((val[live] == 0).any()) and bool((val[live] < 0).any()) and bool((val[live] > 0).any())
        off = live & (val <= 0)
        assert bool((ref["dot"][off] != 0).any())  # the val > 0 gate matters
    assert not ref["code"][:dense_from].any() and not ref["dsc"][:dense_from].any()
    assert not ref["dscv"][~live].any()
    if d >= 1024 and max(ks) >= 33:
        assert ref["dot"].abs().max() > 256  # the bf16 store of the code gradient rounds


@pytest.mark.parametrize("i", [1, 3, 5])  # d = 100, 320 (lanes past d), 768
def test_decode_reference_catches_a_wrong_kernel(i):
    t, _ = _decode_case(i)
    d = X.DECODE_CASES[i][0]
    ref = X.decode_ref(t)
    assert X.decode_matches(X.emulate_decode(t), ref)
    assert not X.decode_matches(X.emulate_decode(t, gate=False), ref)
    assert not X.decode_matches(X.emulate_decode(t, lanes=15), ref)
    if d % 256:
        assert not X.decode_matches(X.emulate_decode(t, zero_tail=False), ref)


def test_prev_idx_steps_overlap():
    d, ks, kmax, per_model, _ = X.DECODE_CASES[3]
    a = X.decode_inputs(3, X.DEC_B, X.DEC_N, d, ks, kmax, per_model, seed=1)
    b = X.decode_inputs(3, X.DEC_B, X.DEC_N, d, ks, kmax, per_model, seed=2)
    ra, rb = X.decode_ref(a), X.decode_ref(b)
    both = (ra["code"] != 0) & (rb["code"] != 0)
    only_a = (ra["code"] != 0) & (rb["code"] == 0)
    assert bool(both.any()) and bool(only_a.any()) and bool((rb["code"][:, 0, 0] != 0)[1:].all())
    assert not torch.equal(ra["code"], rb["code"])


# ------------------------------------------------------------------ sparse weight gradient
@pytest.mark.parametrize("d", X.WGRAD_D)
def test_wgrad_reference_and_lists(d):
    for twin in (False, True):
        t = X.wgrad_inputs(d, dense_twin=twin)
        for alpha in X.WGRAD_ALPHAS:
            ref = X.wgrad_ref(t, alpha)
            assert torch.equal(ref, X.wgrad_ref_slots(t, alpha))
            assert torch.equal(ref.float().double(), ref)  # fp32 holds it exactly
        ref = X.wgrad_ref(t, 1.0)
        if twin:  # what the dense GEMM computes from the scattered bf16 buffers
            dense = t["code"].double().transpose(1, 2) @ t["R"].double() + t["dsc"].double().transpose(1, 2) @ X._x3(t["x"], X.WG_G)
            assert torch.equal(dense, ref) and float(t["val"].min()) == 0
        else:
            assert float(t["val"].min()) < 0
        L = X.list_lengths(t)
        assert int(L[0, X.HOT_ATOM]) == X.WG_B and bool((L == 0).any())
        assert bool(((L % 2 == 1) & (L > 1)).any()) and bool(((L % 2 == 0) & (L > 0)).any())
        assert not ref[L == 0].any()
    assert all(d_ % 256 or d_ > 1024 for d_ in X.WGRAD_REFUSED_D)
