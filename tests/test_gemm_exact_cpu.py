"""The cases of the bit-exact GEMM tests, checked without a GPU: every input recipe satisfies the
conditions that make an fp64 reference the only right answer, the K-tile counts reach every phase
of every K-loop body, and the host-side operand span guard holds its bound."""

import pytest
import torch

import exact_gemm_cases as X

BF = torch.bfloat16
F32 = torch.float32


def _bf(t):
    return t.to(BF)


def test_table_matches_the_launcher_constants():
    from sparse_coding__amd.ops import gemm

    assert len(X.CFG_TABLE) == 12
    for cfg, (bm, bn, bk, nst, loop, full) in X.CFG_TABLE.items():
        assert gemm.SHAPES[cfg & 3] == (bm, bn)
        pipe = (cfg >> 2) & 3
        # (pipe 1 on 128x128 blocks is the BK64 x 3 ring)
        assert (bk, nst) == ((64, 3) if (cfg & 3, pipe) == (1, 1) else gemm.PIPES[pipe])
        assert full == (pipe == 0) and (loop == "p32") == bool(cfg & 16)
    assert (X.EPI_F32, X.EPI_BF16, X.EPI_ENC_ACT, X.EPI_DC_ACT, X.EPI_ROWMAX) == (
        gemm.EPI_F32, gemm.EPI_BF16, gemm.EPI_ENC_ACT, gemm.EPI_DC_ACT, gemm.EPI_ROWMAX)


@pytest.mark.parametrize("cfg", X.ALL_CFGS)
def test_k_tile_counts_reach_every_loop_phase(cfg):
    bk, nst = X.ring(cfg)
    ranges = X.plain_k_ranges(cfg)
    assert X.covered_l(cfg) >= set(range(1, X.max_l(cfg) + 1)), sorted(X.covered_l(cfg))
    assert any(kbeg % nst for kbeg, _ in ranges)  # a range that does not start on the ring's first stage
    whole = {k // bk for k in X.whole_k_values(cfg)}
    assert whole == {t for t in range(1, X.max_l(cfg) + 1) if bk == 64 or t % 2 == 0}
    for k, ks in X.SPLITS:
        r = X.split_ranges(k, bk, ks)
        assert ks <= k // 64 and r[0][0] == 0 and r[-1][1] == k // bk
        assert all(a[1] == b[0] for a, b in zip(r, r[1:])) and all(b > a for a, b in r)
    if bk == 32:  # odd counts come from uneven split ranges and live K ranges only
        assert {3, 5, 7} <= {b - a for k, ks in X.SPLITS for a, b in X.split_ranges(k, bk, ks)}
        assert 1 in {-(-s // bk) for s in X.NACT_K[1]}
    # two segments of different lengths, and a split range across their boundary where one exists
    assert any(k1 != k2 for k1, k2 in X.SEGMENTS)
    for k1, k2 in ((128, 64), (192, 64)):
        assert X.straddling_split(k1, k2, bk) is not None
    # the masked decoder gives the fused epilogue odd counts on the BK32 rings
    if bk == 32:
        assert {1, 3} <= {-(-s // bk) for s in X.MASK_SIZES}


@pytest.mark.parametrize("cfg", X.ALL_CFGS)
def test_every_epilogue_gets_three_k_values(cfg):
    from sparse_coding__amd.ops import gemm

    ks = X.fused_k_values(cfg)
    assert 64 in ks and 128 in ks and 640 in ks and 64 * (X.ring(cfg)[1] + 1) in ks
    # (M, N) of the encoder / code gradient, the decoder and the masked cases
    for name, (M, N) in dict(encoder=(256, 512), decoder=(256, 256), masked=(256, X.MASK_N)).items():
        assert gemm.shape_fits(cfg, M, N) and len(ks) >= 3, name
    bm, bn = X.block(cfg)
    assert 2 * bm <= X.POOL_M and 3 * bn <= X.POOL_N and max(k for k, _ in X.SPLITS) <= X.POOL_K


def test_refusal_table():
    ref = X.refused_launches()
    assert {c for c, _, _ in ref} == set(X.REFUSED_CFGS) | (set(X.ALL_CFGS) - set(X.FULL_CFGS))
    for cfg in X.ALL_CFGS:
        for dt, lay in X.plain_combos(cfg):
            assert (cfg, X.EPI_F32 if dt == F32 else X.EPI_BF16, lay) not in ref


def test_coverage_table_prints():
    rows = X.coverage_table()
    assert len(rows) == 12
    print("\n".join(rows))


@pytest.mark.parametrize("kind", ["int", "ter"])
def test_plain_inputs(kind):
    a, b = (_bf(t) for t in X.plain_pool(kind))
    dtype = F32 if kind == "int" else BF
    spans = {(0, k) for cfg in X.ALL_CFGS for k in X.whole_k_values(cfg)} | {(0, k) for k, _ in X.SPLITS}
    spans |= {(0, 192), (192, 384), (0, X.POOL_K)} | {(0, s) for s in X.NACT_K[1]}
    for cfg in (1, 9):  # one ring of each depth: every split range
        bk = X.ring(cfg)[0]
        spans |= {(t0 * bk, t1 * bk) for k, ks in X.SPLITS for t0, t1 in X.split_ranges(k, bk, ks)}
    for k0, k1 in sorted(spans):
        X.check_plain(a[..., k0:k1], b[..., k0:k1], 2.0, dtype, f"pool {kind} [{k0},{k1})")
    full = X.check_plain(a, b, 1.0, dtype, f"pool {kind}")
    assert full.abs().max().item() > 8  # (not a degenerate product)
    # a shared operand gives another product than per-model operands
    assert not torch.equal(X.ref_plain(a[:1], b)[1], full[1])


@pytest.mark.parametrize("d", [64, 128, 192, 256, 320, 640])
def test_encoder_inputs(d):
    t = X.encoder_inputs(2, 256, 512, d)
    ref = X.check_encode(_bf(t["x"]), _bf(t["w"]), t["bias"])
    X.check_encode(_bf(t["x"][0]), _bf(t["w"]), t["bias"], what="encoder, shared x")
    assert torch.equal(ref["cnt"].sum(1), ref["on"].double().sum(1)) and torch.equal(ref["l0"], ref["cnt"].sum((1, 2)))
    t = X.encoder_inputs(2, 256, 512, d, -3, 3)
    rev = X.check_encode(_bf(t["x"]), _bf(t["w"]), t["bias"], reverse=True, what="reverse encoder")
    assert bool((rev["c"] < 0).any()) and bool((rev["c"] > 0).any())


@pytest.mark.parametrize("n", [64, 128, 192, 256, 320, 640])
def test_decoder_inputs(n):
    t = X.decoder_inputs(2, 256, n, 256)
    ref = X.check_decode(_bf(t["c"]), _bf(t["wd"]), _bf(t["x"]))
    X.check_decode(_bf(t["c"]), _bf(t["wd"]), _bf(t["x"][0]), "decoder, shared x")
    assert ref["rcol"].shape == (2, 2, 256) and torch.equal(ref["rcol"].sum(1), ref["r"].sum(1))


@pytest.mark.parametrize("d", [64, 128, 192, 256, 320, 640])
def test_code_grad_inputs(d):
    enc = X.encoder_inputs(2, 256, 512, 64)
    e = X.ref_encode(_bf(enc["x"]), _bf(enc["w"]), enc["bias"])
    t = X.codegrad_inputs(2, 256, 512, d)
    ref = X.check_code_grad(_bf(t["r"]), _bf(t["w"]), _bf(e["c"].float()), e["on"], t["l1"], t["tied_bias"])
    assert not torch.equal(ref["dot"], ref["dot_tied"])
    assert len(set(t["l1"].tolist())) == 2  # every model its own l1
    enc = X.encoder_inputs(2, 256, 512, d, -3, 3)
    e = X.ref_encode(_bf(enc["x"]), _bf(enc["w"]), enc["bias"], reverse=True)
    rev = X.check_code_grad(_bf(t["r"]), _bf(t["w"]), _bf(e["c"].float()), e["on"], t["l1"], reverse=True)
    assert not rev["colpart"].any()


def test_mask_pair_inputs():
    enc = X.encoder_inputs(2, 256, 256, 64)
    e = X.check_encode(_bf(enc["x"]), _bf(enc["w"]), enc["bias"])
    t = X.codegrad_inputs(2, 256, 256, 64)
    X.check_code_grad(_bf(t["r"]), _bf(t["w"]), _bf(e["c"].float()), e["on"], t["l1"])


@pytest.mark.parametrize("sizes", [X.MASK_SIZES, X.MASK_SIZES_ZERO])
def test_masked_inputs(sizes):
    G, B, n = 4, 256, X.MASK_N
    assert any(s % 128 for s in sizes) and len(sizes) == G and max(sizes) == n
    enc = X.encoder_inputs(G, B, n, 64)
    e = X.check_encode(_bf(enc["x"][0]), _bf(enc["w"]), enc["bias"], live=sizes)
    for g, s in enumerate(sizes):
        assert not e["c"][g, :, s:].any() and not e["cnt"][g, :, s:].any()
    t = X.codegrad_inputs(G, B, n, 128)
    X.check_code_grad(_bf(t["r"]), _bf(t["w"]), _bf(e["c"].float()), e["on"], t["l1"], live=sizes)
    dec = {k: _bf(v) for k, v in X.decoder_inputs(G, B, n, 256).items()}
    for g, s in enumerate(sizes):
        dec["c"][g, :, s:] = 0
    X.check_decode(dec["c"], dec["wd"], dec["x"], "masked decoder", sizes)
    wg = X.wgrad_masked_inputs(G, 256, n, 256, tuple(sizes))
    at, bt = _bf(wg["a"]).transpose(1, 2), _bf(wg["b"]).transpose(1, 2)
    ref = X.ref_plain(at, bt)
    X.assert_accumulators(at, bt, "masked weight gradient")
    X.assert_bf16_out(ref, "masked weight gradient")
    for g, s in enumerate(sizes):
        assert not ref[g, s:].any()
        if s:
            X.assert_k_tiles_contribute(at[g:g + 1], bt[g:g + 1], f"masked weight gradient model {g}")


def test_rowmax_inputs():
    a, b = (_bf(t) for t in X.plain_pool("int"))
    a, b = a[:2, :130, :65], b[:2, :257, :65]
    X.assert_accumulators(a, b, "rowmax")
    X.assert_exact(X.ref_plain(a, b, 0.5), "rowmax", unit=0.5)


# ------------------------------------------------------------------ operand span guard
def test_operand_span_guard():
    from sparse_coding__amd.ops import gemm

    lim = gemm.MAX_OPERAND_SPAN
    assert lim == 2 ** 31 - 1
    # K-major [rows][ld]: the last element ends at ((rows - 1) ld + K) * 2 bytes; [K][ld] likewise
    assert gemm.operand_span_bytes(128, 64, 64, True) == 128 * 64 * 2
    assert gemm.operand_span_bytes(128, 64, 256, True) == (127 * 256 + 64) * 2
    assert gemm.operand_span_bytes(128, 64, 256, False) == (63 * 256 + 128) * 2
    # B = 32768 codes at n = 32768 (one model: exactly 2 GiB) is refused as either operand kind
    big = 32768
    assert gemm.operand_span_bytes(big, big, big, True) == 2 ** 31 == gemm.operand_span_bytes(big, big, big, False)
    for layout in (0, 1, 2, 3):
        gemm.check_operand_spans(layout, 128, 128, 64, 64, [64, 64], [64, 64])
        with pytest.raises(ValueError, match="operand A"):
            gemm.check_operand_spans(layout, big, 128, big, 0, [big, big], [big if layout & 2 else 128] * 2)
        with pytest.raises(ValueError, match="operand B"):
            gemm.check_operand_spans(layout, 128, big, big, 0, [big if layout & 1 else 128] * 2, [big, big])
    # just below and at the bound: rows x K bf16, K-major, ld = K
    K = 1 << 15
    gemm.check_operand_spans(3, K - 1, 128, K, 0, [K, K], [K, K])  # (2^31 - 2^16) bytes
    assert gemm.operand_span_bytes(K, K - 64, K, True) == 2 ** 31 - 128
    gemm.check_operand_spans(3, K, 128, K - 64, 0, [K, K], [K, K])
    ld = (lim // 2 - 64) // 127 + 1  # smallest ld whose 128-row span reaches the bound
    assert gemm.operand_span_bytes(128, 64, ld - 1, True) < lim <= gemm.operand_span_bytes(128, 64, ld, True)
    gemm.check_operand_spans(3, 128, 128, 64, 0, [ld - 1] * 2, [64, 64])
    with pytest.raises(ValueError):
        gemm.check_operand_spans(3, 128, 128, 64, 0, [ld] * 2, [64, 64])
    # the second segment and the second problem are checked too; an unused second segment is not
    gemm.check_operand_spans(0, 128, 128, 64, 0, [128, ld * 4096], [128, 128])
    with pytest.raises(ValueError, match="segment 1"):
        gemm.check_operand_spans(3, 128, 128, 64, 64, [64, ld], [64, 64])
    with pytest.raises(ValueError):
        gemm.check_operand_spans(3, 128, 128, 64, 0, [64, 64, ld, ld], [64] * 4)
