"""Cases, input recipes, fp64 references and branch emulation for the exact top-k tests
(``test_topk_exact_cpu.py`` checks all of this without a GPU, ``test_topk_exact_gpu.py`` compares the
kernels of ``ops/csrc/topk.hip`` against it with ``torch.equal``).

Decode / code gradient / sparse weight gradient: the dictionary is ternary bf16, ``x`` and the picked
values are small integers, so every product and partial sum is an integer below 2^24 and any fp32
summation order gives the same bits (``check_decode`` / ``check_wgrad`` assert the conditions).

Select: the references work on the kernels' orderable integer keys, so they are exact and
order-free; where the tie order is part of the contract the picked *set* is that of
``sort by (-key, rank)`` with the rank of the path the row takes (``select_branch`` mirrors the
dispatch and the branch predicates of the kernels with integer compares on the per-thread column
layout).
"""

from __future__ import annotations

import re
import zlib
from pathlib import Path

import torch

BF, F32, F64, I64 = torch.bfloat16, torch.float32, torch.float64, torch.int64
HIP_SOURCE = Path(__file__).resolve().parent.parent / "sparse_coding__amd" / "ops" / "csrc" / "topk.hip"

# mirrored from topk.hip (test_topk_exact_cpu.py parses the source and compares)
BR_CAP, TIE_CAP, S1 = 1024, 64, 12
LOW = 32 - S1
EXACT = 1 << 24  # integers below this are exact in fp32


def parsed_constants():
    src = HIP_SOURCE.read_text()
    return {name: sorted({int(v) for v in re.findall(rf"constexpr int {name} = (\d+)", src)})
            for name in ("BR_CAP", "TIE_CAP", "S1")}


def _gen(*seed):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(seed).encode()))
    return g


# ===================================================================== select: dispatch and layout
SELECT_N = {  # (kernel, keys per thread) -> row lengths
    ("wave", 16): (4, 8, 1024), ("wave", 32): (1028, 2048), ("wave", 64): (2052, 4096),
    ("block", 24): (4100,), ("block", 32): (6148, 8192), ("block", 48): (8196,), ("block", 64): (16384,),
    ("radix", 4): (1, 3, 1023), ("radix", 8): (2047,), ("radix", 16): (4095,), ("radix", 24): (6143,),
    ("radix", 32): (8191,), ("radix", 48): (12287,), ("radix", 64): (16383,),
    ("bf16", 8): (8, 2048), ("bf16", 16): (2056, 4096), ("bf16", 24): (6144,), ("bf16", 32): (8192,),
    ("bf16", 48): (12288,), ("bf16", 64): (16384,),
}
REFUSED_N = {False: (16385, 16388), True: (12, 16392)}  # bf16? -> row lengths without a kernel
F32_N = [n for (kind, _), ns in SELECT_N.items() if kind != "bf16" for n in ns]
BF16_N = [n for (kind, _), ns in SELECT_N.items() if kind == "bf16" for n in ns]
SEL_G, SEL_B = 3, 5  # 15 rows: not a multiple of the wave kernel's 4 rows per block
REQUIRED_BRANCHES = {
    "wave": {"bucket", "crowded"},
    "block": {"bracket", "overflow", "full_bucket", "full_crowded"},
    "radix": {"tie_pass0", "tie_pass1", "tie_pass2", "k0"},
    "bf16": {"clean", "resolve", "many_ties", "overflow", "full"},
}
# order of the ties the bf16 bracket takes without an exact resolve: "column", or "thread"
BF16_BRACKET_TIES = "column"


def dispatch(bf16: bool, n: int):
    """(kernel, keys per thread) that sc_topk_select / sc_topk_select_bf16 launch, None: refused."""
    if bf16:
        if n % 8 or n < 8:
            return None
        return next((("bf16", p) for p in (8, 16, 24, 32, 48, 64) if n <= 256 * p), None)
    if n % 4 == 0:
        for p in (16, 32, 64):
            if n <= 64 * p:
                return "wave", p
        for p in (24, 32, 48, 64):
            if n <= 256 * p:
                return "block", p
    return next((("radix", p) for p in (4, 8, 16, 24, 32, 48, 64) if (n + 255) // 256 <= p), None)


def layout(kind: str, P: int):
    """[threads, P]: the column thread t holds in register slot s (the kernels' load loops); columns
    past the row are padding.  Flattened, this is the thread-major candidate order."""
    if kind == "radix":
        return torch.arange(256)[:, None] + torch.arange(P)[None] * 256
    T, V = {"wave": (64, 4), "block": (256, 4), "bf16": (256, 8)}[kind]
    t, i, j = torch.arange(T)[:, None, None], torch.arange(P // V)[None, :, None], torch.arange(V)[None, None]
    return ((i * T + t) * V + j).reshape(T, P)


def thread_major_rank(kind: str, P: int, n: int):
    cols = layout(kind, P).reshape(-1)
    rank = torch.empty(cols.numel(), dtype=I64)
    rank[cols] = torch.arange(cols.numel())
    return rank[:n]


def order_keys(scores, absolute=False):
    """int64 orderable key of every score: order_key (fp32) / order16 (bf16) of topk.hip."""
    if scores.dtype == BF:
        h = scores.view(torch.int16).to(I64) & 0xFFFF
        h = h & 0x7FFF if absolute else h
        return torch.where((h & 0x8000) != 0, ~h & 0xFFFF, h | 0x8000)
    u = scores.view(torch.int32).to(I64) & 0xFFFFFFFF
    u = u & 0x7FFFFFFF if absolute else u
    return torch.where((u & 0x80000000) != 0, ~u & 0xFFFFFFFF, u | 0x80000000)


# ===================================================================== select: branch emulation
def _kth(keys, k):
    return int(torch.topk(keys, k).values[-1])


def _bucket(keys, k):
    """The bisection kernels after S1 bits: how many keys share the threshold's top S1 bits."""
    nb = int(((keys >> LOW) == (_kth(keys, k) >> LOW)).sum())
    return "bucket" if nb <= 64 else "crowded"


def _bracket(kind, P, keys, k):
    """bracket_select: lo = k-th largest per-thread maximum (padding keys are 0) and the number of
    keys, padding included, that reach it."""
    cols = layout(kind, P)
    full = torch.zeros(cols.numel(), dtype=I64)
    full[:keys.numel()] = keys
    lo = _kth(full[cols].amax(1), k)
    return lo, int((full >= lo).sum())


def _radix_tags(keys, k):
    tags, prefix, mask, remaining = [], 0, 0, k
    for p, (shift, width) in enumerate(((21, 11), (10, 11), (0, 10))):
        dm = (1 << width) - 1
        cnt = torch.bincount((keys[(keys & mask) == prefix] >> shift) & dm, minlength=2048)
        suffix = cnt.flip(0).cumsum(0).flip(0)  # keys in this bin or a higher one
        sel = int((suffix >= remaining).nonzero().max())
        above = int(suffix[sel] - cnt[sel])
        if int(cnt[sel]) > remaining - above:  # the digit holding the threshold is shared
            tags.append(f"tie_pass{p}")
        prefix, mask, remaining = prefix | (sel << shift), mask | (dm << shift), remaining - above
    assert prefix == _kth(keys, k)
    return tags


def select_branch(kind, P, keys, k, have_x=False):
    """Tags of the code path one row (int64 keys [n], effective k) takes in its kernel."""
    if k == 0:
        return {"k0"}
    if kind == "wave":
        return {_bucket(keys, k)}
    if kind == "radix":
        return set(_radix_tags(keys, k))
    if k > 256:
        return {"full"} if kind == "bf16" else {"full_" + _bucket(keys, k)}
    lo, total = _bracket(kind, P, keys, k)
    if total > BR_CAP:
        return {"overflow"} if kind == "bf16" else {"overflow", "overflow_" + _bucket(keys, k)}
    if kind == "block":
        return {"bracket"}
    t = _kth(keys, k)
    need, nt = k - int((keys > t).sum()), int((keys == t).sum())
    if nt <= need:
        return {"clean"}
    if nt <= TIE_CAP:
        return {"resolve" if have_x else "few_ties"}
    return {"many_ties"}


def tie_rank(kind, P, n, tags, exact_row=None):
    """Rank that orders equal keys on the path ``tags``: the contract of each kernel."""
    col = torch.arange(n)
    if "resolve" in tags:  # the exact fp32 scores, ties to the lower column
        order = torch.argsort(exact_row.to(I64) * 32768 - col, descending=True)
        rank = torch.empty(n, dtype=I64)
        rank[order] = col
        return rank
    thread = (kind == "radix" or (kind == "block" and "bracket" in tags)
              or (kind == "bf16" and BF16_BRACKET_TIES == "thread" and tags & {"few_ties", "many_ties"}))
    return thread_major_rank(kind, P, n) if thread else col


def expected_picks(keys, k, rank):
    """The k columns first in (-key, rank) order, ascending."""
    return torch.topk(keys * 32768 + (32767 - rank), k).indices.sort().values


def exact_scores(x, D):
    """fp64 <x_b, D[g, j]> [G, B, n] of small-integer bf16 operands."""
    xe = x.double() if x.dim() == 3 else x.double().unsqueeze(0).expand(D.shape[0], -1, -1)
    e = torch.einsum("gbd,gnd->gbn", xe, D.double())
    assert e.abs().max() < EXACT and torch.equal(e, e.round())
    return e


def check_select(scores, ks, kmax, idx, val, absolute=False, relu=True, x=None, D=None, what="select"):
    """Every property of one select launch, against the integer keys; returns the tags of each row."""
    scores, idx, val = scores.cpu(), idx.cpu(), val.cpu()
    G, B, n = scores.shape
    kind, P = dispatch(scores.dtype == BF, n)
    keys_all, sf = order_keys(scores, absolute), scores.float()
    have_x = x is not None and not absolute and scores.dtype == BF
    exact = exact_scores(x.cpu(), D.cpu()) if have_x else None
    tags_all = []
    for g in range(G):
        k = min(int(ks[g]), n, kmax)
        for b in range(B):
            row = f"{what} n={n} row ({g}, {b}) k={k}"
            assert torch.equal(idx[g, b, k:], torch.zeros(kmax - k, dtype=torch.int32)), row + ": idx padding"
            assert torch.equal(val[g, b, k:], torch.zeros(kmax - k)), row + ": val padding"
            keys = keys_all[g, b]
            tags = select_branch(kind, P, keys, k, have_x)
            tags_all.append(tags)
            if k == 0:
                continue
            pick = idx[g, b, :k].long()
            assert int(pick.min()) >= 0 and int(pick.max()) < n, row + ": column out of range"
            got = pick.sort().values
            assert bool((got.diff() > 0).all()), row + ": duplicate columns"
            want_val = sf[g, b][pick].clamp(min=0) if relu else sf[g, b][pick]
            assert torch.equal(val[g, b, :k], want_val), row + ": val is not the picked score"
            top = torch.topk(keys, k).values
            assert torch.equal(keys[pick].sort(descending=True).values, top), row + ": not a top-k of the keys"
            assert bool(torch.isin((keys > top[-1]).nonzero().flatten(), pick).all()), row + ": a key above the k-th is missing"
            want = expected_picks(keys, k, tie_rank(kind, P, n, tags, exact[g, b] if have_x else None))
            if not torch.equal(got, want):
                i = int((got != want).nonzero()[0])
                raise AssertionError(f"{row} {sorted(tags)}: picked set differs, first at sorted slot {i}: "
                                     f"column {int(got[i])} vs {int(want[i])}")
    return tags_all


def emulate_select(scores, ks, kmax, absolute=False, relu=True, x=None, D=None, ties="contract"):
    """(idx, val) of a select that follows the contract, or (``ties="thread"``) takes every tie in the
    thread-major order of its kernel's layout."""
    G, B, n = scores.shape
    kind, P = dispatch(scores.dtype == BF, n)
    keys_all, sf = order_keys(scores, absolute), scores.float()
    have_x = x is not None and not absolute and scores.dtype == BF
    exact = exact_scores(x, D) if have_x else None
    idx, val = torch.zeros(G, B, kmax, dtype=torch.int32), torch.zeros(G, B, kmax)
    for g in range(G):
        k = min(int(ks[g]), n, kmax)
        for b in range(B if k else 0):
            keys = keys_all[g, b]
            tags = select_branch(kind, P, keys, k, have_x)
            rank = (tie_rank(kind, P, n, tags, exact[g, b] if have_x else None) if ties == "contract"
                    else thread_major_rank(kind, P, n))
            pick = expected_picks(keys, k, rank)
            idx[g, b, :k] = pick.int()
            val[g, b, :k] = sf[g, b][pick].clamp(min=0) if relu else sf[g, b][pick]
    return idx, val


# ===================================================================== select: input recipes
# bf16 bit patterns of normal values on either side of the tie value 0.75 (0x3F40): rows drawn from
# them without replacement have distinct keys spread over every exponent
_TIE = 0x3F40
_ABOVE = torch.arange(0x3F41, 0x7F00)
_BELOW = torch.cat([torch.arange(0x0080, 0x3F40), torch.arange(0x8080, 0xFF80)])
BOUNDARY = {"wave": 256, "block": 1024, "bf16": 2048, "radix": 256}  # columns per chunk of the layout


def tied_row(n, k, m, need, start, gen):
    """bf16 patterns [n]: k - need distinct values above 0.75, m columns from ``start`` equal to 0.75,
    distinct values below elsewhere; (m, need, start are clipped to the row)."""
    k = max(1, min(k, n))
    need = max(1, min(need, k))
    m = max(need, min(m, n - (k - need)))
    start = max(0, min(start, n - m))
    pat = torch.empty(n, dtype=I64)
    rest = torch.cat([torch.arange(0, start), torch.arange(start + m, n)])
    rest = rest[torch.randperm(rest.numel(), generator=gen)]
    above, below = rest[:k - need], rest[k - need:]
    pat[start:start + m] = _TIE
    pat[above] = _ABOVE[torch.randperm(_ABOVE.numel(), generator=gen)[:above.numel()]]
    pat[below] = _BELOW[torch.randperm(_BELOW.numel(), generator=gen)[:below.numel()]]
    return pat


def patterns_to_scores(pat, bf16, gen):
    """bf16 scores of the patterns, or fp32 scores with random low mantissa bits (equal patterns of
    the tie value stay equal; the order against 0.75 is kept)."""
    if bf16:
        return torch.where(pat >= 0x8000, pat - 0x10000, pat).to(torch.int16).view(BF)
    low = torch.randint(0, 1 << 16, pat.shape, generator=gen)
    bits = (pat << 16) | torch.where(pat == _TIE, torch.full_like(low, 0x1234), low)
    return torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32).view(F32)


def select_ks(kind):
    return ((0, 20, 150), 150) if kind == "radix" else ((20, 150, 300), 300)


def select_case(n, bf16):
    """scores [3, 5, n] whose rows take every branch of their kernel, k [3] and kmax."""
    kind, _ = dispatch(bf16, n)
    ks, kmax = select_ks(kind)
    gen, bd = _gen("select", n, bf16), BOUNDARY[kind]
    rows = []
    for g, k in enumerate(ks):
        k = min(k, n)
        rows += [
            patterns_to_scores(tied_row(n, k, 1, 1, 0, gen), bf16, gen),  # distinct keys
            torch.randn(n, generator=gen).to(BF if bf16 else F32),
            patterns_to_scores(tied_row(n, k, 10, 4, bd - 5, gen), bf16, gen),  # a few ties over a chunk boundary
            patterns_to_scores(tied_row(n, k, 200, 50, bd - 48, gen), bf16, gen),  # more than TIE_CAP of them
            (torch.zeros(n, dtype=BF if bf16 else F32) if g % 2 == 0  # more candidates than BR_CAP
             else patterns_to_scores(tied_row(n, k, 1100, 7, bd - 300, gen), bf16, gen)),
        ]
    return dict(scores=torch.stack(rows).view(SEL_G, SEL_B, n).contiguous(), ks=ks, kmax=kmax)


def select_operands(n, d, per_model, G=SEL_G, B=SEL_B):
    """Small-integer bf16 (x, D) for the exact resolve: the fp32 recompute is exact in any order."""
    gen = _gen("operands", n, d, per_model)
    x = torch.randint(-4, 5, ((G, B, d) if per_model else (B, d)), generator=gen).to(BF)
    return x.contiguous(), torch.randint(-2, 3, (G, n, d), generator=gen).to(BF).contiguous()


RESOLVE_EXTRA = [(1024, 260), (256, 768)]  # (n, d) beyond d = 4: the recompute strides 256 elements a pass


def tie_order_case(bf16):
    """Tie-order pins beyond one chunk of the layout: 200 equal keys just below 100 larger ones,
    k = 150.  bf16: n = 4096, ties in columns 2000..2199; fp32 block kernel: n = 8192, 1000..1199."""
    n, start = (4096, 2000) if bf16 else (8192, 1000)
    gen = _gen("tie order", bf16)
    rows = [patterns_to_scores(tied_row(n, 150, 200, 50, start, gen), bf16, gen) for _ in range(SEL_G * SEL_B)]
    return dict(scores=torch.stack(rows).view(SEL_G, SEL_B, n).contiguous(), ks=(150, 150, 150), kmax=150,
                ties=(start, start + 200))


def over_kmax_case(n, bf16):
    """k[g] = kmax + 5 on the last model (its unclamped rows would run into the guard)."""
    c = select_case(n, bf16)
    return dict(scores=c["scores"], ks=(12, 5, 17), kmax=12)


OVER_KMAX_N = [(1024, False), (4100, False), (1023, False), (2048, True)]  # wave, block, radix, bf16


# ===================================================================== decode and code gradient
DEC_B, DEC_N = 10, 64  # 10 rows a model: not a multiple of the kernel's 4 rows per block
DECODE_CASES = [  # d, k per model, kmax, per-model x, dense_from
    (4, (1, 8, 17), 17, False, 0),
    (100, (7, 16, 33), 33, True, 1),
    (256, (9, 15, 64), 64, False, 3),
    (320, (0, 17, 64), 64, True, 0),
    (512, (1, 7, 9), 20, False, 1),
    (768, (8, 16, 33), 33, True, 0),
    (1024, (15, 17, 64), 64, False, 3),
    (1280, (7, 9, 33), 40, True, 1),
    (2048, (1, 16, 64), 64, False, 0),
    (2052, (8, 15, 17), 17, True, 1),
    (4096, (1, 17, 64), 64, False, 0),
]
DECODE_REFUSED_D = (4100, 6)


def decode_nv(d):
    """Instantiation (64-lane passes of 4 elements over the row) sc_topk_decode_grad launches."""
    if d % 4:
        return None
    return next((v for v in (1, 2, 3, 4, 8, 16) if (d + 255) // 256 <= v), None)


def decode_inputs(G, B, n, d, ks, kmax, per_model, seed=0, min_val=-1):
    """Ternary D (density 1/8), integer x in [-4, 4], distinct picks per row with integer values in
    [min_val, 3]; slots >= k[g] are (0, 0.0) as the select leaves them.  Row 0 of every model picks
    column 0 with a positive value (the padded slots carry index 0 too)."""
    gen = _gen("decode", G, B, n, d, tuple(ks), kmax, per_model, seed)
    D = ((torch.randint(0, 8, (G, n, d), generator=gen) == 0) * (torch.randint(0, 2, (G, n, d), generator=gen) * 2 - 1))
    x = torch.randint(-4, 5, ((G, B, d) if per_model else (B, d)), generator=gen)
    idx = torch.stack([torch.randperm(n, generator=gen)[:kmax] for _ in range(G * B)]).view(G, B, kmax)
    val = torch.randint(min_val, 4, (G, B, kmax), generator=gen).float()
    for g in range(G):
        row = idx[g, 0]
        if (row == 0).any():
            j = int((row == 0).nonzero()[0])
            row[j] = row[0].clone()
        row[0] = 0
        val[g, 0, 0] = 2.0
        idx[g, :, ks[g]:] = 0
        val[g, :, ks[g]:] = 0.0
    return dict(D=D.to(BF).contiguous(), x=x.to(BF).contiguous(), idx=idx.int().contiguous(), val=val.contiguous(),
                ks=tuple(ks), kmax=kmax)


def _live(ks, kmax, B):
    return (torch.arange(kmax)[None, None] < torch.tensor(ks).clamp(max=kmax)[:, None, None]).expand(-1, B, -1)


def _x3(x, G):
    return x.double() if x.dim() == 3 else x.double().unsqueeze(0).expand(G, -1, -1)


def decode_ref(t, dense_from=0):
    """fp64 reference of decode_grad: R [G, B, d], row_se [G, B], dot / dscv [G, B, kmax] and the
    dense bf16 code / code-gradient buffers [G, B, n] (zero wherever nothing is scattered)."""
    D, idx, val = t["D"].double(), t["idx"].long(), t["val"].double()
    G, n, d = D.shape
    B, kmax = idx.shape[1:]
    live = _live(t["ks"], kmax, B)
    rows = torch.gather(D.unsqueeze(1).expand(-1, B, -1, -1), 2, idx.unsqueeze(-1).expand(-1, -1, -1, d))  # D[idx]
    R = torch.einsum("gbk,gbkd->gbd", val * live, rows) - _x3(t["x"], G)
    dot = torch.einsum("gbd,gbkd->gbk", R, rows)
    on = live & (val > 0)
    dscv = torch.where(on, dot, torch.zeros_like(dot))
    dense = on & (torch.arange(G)[:, None, None] >= dense_from)
    code = torch.zeros(G, B, n, dtype=BF)
    dsc = torch.zeros(G, B, n, dtype=BF)
    g, b, s = dense.nonzero(as_tuple=True)
    code[g, b, idx[g, b, s]] = val[g, b, s].float().to(BF)
    dsc[g, b, idx[g, b, s]] = dot[g, b, s].float().to(BF)
    return dict(R=R, row_se=(R * R).sum(-1), dot=dot, dscv=dscv, code=code, dsc=dsc, live=live, on=on)


def decode_ref_dense(t):
    """The same R, row_se and dots through a dense one-hot code matrix (a second formulation)."""
    D, idx, val = t["D"].double(), t["idx"].long(), t["val"].double()
    G, n, _ = D.shape
    B, kmax = idx.shape[1:]
    codes = torch.zeros(G, B, n, dtype=F64).scatter_add_(-1, idx, val * _live(t["ks"], kmax, B))
    R = codes @ D - _x3(t["x"], G)
    return dict(R=R, row_se=(R * R).sum(-1), dot=torch.gather(R @ D.transpose(1, 2), -1, idx))


def check_decode(t, ref, what):
    """The conditions under which every fp32 order of the kernel's sums gives the reference's bits."""
    R = ref["R"]
    assert torch.equal(R, R.round()) and R.abs().max() <= 256, f"{what}: R is not a bf16-exact integer"
    assert ref["row_se"].max() < EXACT, f"{what}: sum R^2 reaches 2^24"
    bound = torch.einsum("gbd,gnd->gbn", R.abs(), t["D"].double().abs()).max()  # every partial sum of every dot
    assert bound < EXACT, f"{what}: a partial dot reaches 2^24"
    assert t["val"].abs().sum(-1).max() + 4 < EXACT, f"{what}: a partial decode sum reaches 2^24"  # |D| <= 1
    return dict(max_R=float(R.abs().max()), max_se=float(ref["row_se"].max()), max_dot=float(ref["dot"].abs().max()))


def emulate_decode(t, gate=True, lanes=16, zero_tail=True):
    """torch emulation of topk_decode_grad_kernel's arithmetic on its lane layout: NV passes of 64
    lanes x 4 elements with clamped loads past d, per-lane partial dots reduced over 16-lane groups.
    The flags break it the way a wrong kernel would: ``gate=False`` drops the val > 0 gate,
    ``lanes=15`` leaves one lane out of every 16-lane butterfly group, ``zero_tail=False`` keeps what
    the clamped loads accumulated in the lanes past d."""
    D, idx, val = t["D"].double(), t["idx"].long(), t["val"].double()
    G, n, d = D.shape
    B, kmax = idx.shape[1:]
    W = decode_nv(d) * 256
    e = torch.arange(W)
    src = torch.minimum(e // 4 * 4, torch.tensor(d - 4)) + e % 4  # clamped 4-element loads
    valid = e // 4 * 4 < d
    live = _live(t["ks"], kmax, B)
    rows = torch.gather(D.unsqueeze(1).expand(-1, B, -1, -1), 2, idx.unsqueeze(-1).expand(-1, -1, -1, d))[..., src]
    acc = torch.einsum("gbk,gbke->gbe", val * live, rows)
    xp = torch.zeros(G, B, W, dtype=F64)
    xp[..., valid] = _x3(t["x"], G)[..., src[valid]]
    acc = torch.where(valid, acc - xp, torch.zeros_like(acc) if zero_tail else acc)
    R = acc[..., valid]
    lane = (e // 4) % 64
    part = torch.zeros(G, B, kmax, 64, dtype=F64).index_add_(-1, lane, acc.unsqueeze(2) * rows)
    dot = part[..., (torch.arange(64) % 16) < lanes].sum(-1)
    on = live & (val > 0) if gate else live
    dscv = torch.where(on, dot, torch.zeros_like(dot))
    code, dsc = torch.zeros(G, B, n, dtype=BF), torch.zeros(G, B, n, dtype=BF)
    g, b, s = on.nonzero(as_tuple=True)
    code[g, b, idx[g, b, s]] = val[g, b, s].float().to(BF)
    dsc[g, b, idx[g, b, s]] = dot[g, b, s].float().to(BF)
    return dict(R=R, row_se=(R * R).sum(-1), dscv=dscv, code=code, dsc=dsc)


def decode_matches(out, ref):
    return all(torch.equal(out[k], ref[k]) for k in ("R", "row_se", "dscv", "code", "dsc"))


# ===================================================================== sparse weight gradient
WG_G, WG_B, WG_N, WG_KS, WG_KMAX = 3, 64, 128, (3, 8, 20), 20  # (n, B: multiples of the dense GEMM's tiles)
WGRAD_D = (256, 512, 768, 1024)
WGRAD_REFUSED_D = (128, 320, 1280)
WGRAD_ALPHAS = (1.0, 0.125)
HOT_ATOM = 5  # picked by every row of model 0


def wgrad_inputs(d, dense_twin=False):
    """Decode inputs whose model 0 picks atom HOT_ATOM in every row, with R and dscv from the decode
    *reference*.  ``dense_twin``: the inputs on which the dense path computes the same sums -- values
    clamped at 0 (the dense code buffer holds only positive codes) and code gradients rounded to
    bf16 (the dense code-gradient buffer's storage)."""
    t = decode_inputs(WG_G, WG_B, WG_N, d, WG_KS, WG_KMAX, per_model=(d // 256) % 2 == 0, seed=7,
                      min_val=0 if dense_twin else -1)
    idx = t["idx"]
    for b in range(WG_B):
        row = idx[0, b, :WG_KS[0]]
        if not (row == HOT_ATOM).any():
            row[1] = HOT_ATOM
    assert all(idx[g, b, :k].unique().numel() == k for g, k in enumerate(WG_KS) for b in range(WG_B))
    ref = decode_ref(t)
    check_decode(t, ref, f"weight-gradient inputs d={d}")
    t["R"] = ref["R"].float().to(BF).contiguous()
    t["dscv"] = (ref["dscv"].float().to(BF).float() if dense_twin else ref["dscv"].float()).contiguous()
    t["code"], t["dsc"] = ref["code"], ref["dsc"]
    return t


def _slot_matrices(t):
    idx = t["idx"].long()
    G, B, kmax = idx.shape
    n = t["D"].shape[1]
    live = _live(t["ks"], kmax, B)
    C = torch.zeros(G, B, n, dtype=F64).scatter_add_(-1, idx, t["val"].double() * live)
    S = torch.zeros(G, B, n, dtype=F64).scatter_add_(-1, idx, t["dscv"].double() * live)
    return C, S


def wgrad_ref(t, alpha):
    """alpha * sum_b (val R + dscv x) per picked atom [G, n, d], fp64; every partial sum below 2^24."""
    C, S = _slot_matrices(t)
    R, x = t["R"].double(), _x3(t["x"], C.shape[0])
    bound = (C.abs().transpose(1, 2) @ R.abs() + S.abs().transpose(1, 2) @ x.abs()).max()
    assert bound < EXACT, f"a weight-gradient partial sum reaches 2^24 ({float(bound)})"
    return alpha * (C.transpose(1, 2) @ R + S.transpose(1, 2) @ x)


def wgrad_ref_slots(t, alpha):
    """The same sums slot by slot (a second formulation)."""
    idx, val, dscv = t["idx"].long(), t["val"].double(), t["dscv"].double()
    G, B, kmax = idx.shape
    R, x = t["R"].double(), _x3(t["x"], G)
    out = torch.zeros(G, t["D"].shape[1], R.shape[-1], dtype=F64)
    for g in range(G):
        for s in range(min(t["ks"][g], kmax)):
            out[g].index_add_(0, idx[g, :, s], val[g, :, s, None] * R[g] + dscv[g, :, s, None] * x[g])
    return alpha * out


def list_lengths(t):
    """Rows that picked each atom [G, n]: the length of its slot list."""
    return (_slot_matrices(dict(t, val=torch.ones_like(t["val"])))[0] != 0).sum(1)
