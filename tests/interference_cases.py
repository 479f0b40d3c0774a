"""Inputs shared by the interference tests (``test_interference_cpu.py`` checks the fixtures' own properties,
``test_interference_gpu.py`` runs the kernel on them).  Everything is built on the CPU from fixed seeds.

**Planted.**  Every atom is a power of two times a sum of *unit blocks* -- one coordinate of value 1 (d = 32)
or four of value 1/2 (larger d), on disjoint coordinates -- so every dot product and squared norm is a small
power of two.  Atoms come in *units* whose members overlap only each other:

- a *class*: m = 2^k copies of one block under different scales: cos^2 = 1 between its members;
- a *star*: five atoms ``hub + spoke_i`` over one hub block and five spoke blocks: cos^2 = 1/4 between them.

A row activates whole stars and power-of-two subsets of classes, one code (a power of two) per unit and at
most one subset per class.  Then ``total`` is ``m c`` in a class subset and ``(1 + 4/4) c = 2 c`` in a star: a
power of two, every capacity is 1/m or 1/2, and ``cap 2^32`` is an integer.  Every intermediate of the
kernel's fp32 arithmetic is exact, whatever the order, so its outputs equal the fp64 oracle's bit for bit.
Star A sits on columns {0, 1, n/2, n-2, n-1}: its 1/4-overlaps join the first and the last entry of a row and,
in the rows with 17 and 33 entries, the entries 15 | 16 and 31 | 32 on either side of a 16-entry tile boundary.

**Random.**  ``normalize(u + 0.7 noise)`` rounded to bf16, the noise of unit length and orthogonal to the
common direction u: every pairwise cos is >= 0.51 / 1.49, so every cos^2 >= 0.1 and dropping or
double-counting one pair moves a capacity by far more than the bound of ``entry_bound``.
"""

import torch

G, B = 3, 128
# (n, d): d = 32 is one MFMA step, 160 no multiple of 64; past d = 512 the kernel reloads the i-tile per k-step
SHAPES = [(128, 32), (640, 32), (128, 128), (640, 160), (128, 544)]
PLANTED_L = (0, 1, 15, 16, 17, 31, 32, 33, 48)            # rows 0 .. 8; row 9 has all n columns active
STAR_B = (7, 8, 9, 10, 11)


def star_a(n):
    return (0, 1, n // 2, n - 2, n - 1)


def _class_sizes(m):
    return [1 << k for k in range(m.bit_length() - 1, -1, -1) if m >> k & 1]


def planted(n, d, seed=0):
    """(D bf16 [G, n, d], dense codes fp32 [G, B, n], units) -- ``units[g]`` lists the column tuples of the
    units of model g (the two stars first)."""
    gen = torch.Generator().manual_seed(1000 * seed + n + d)
    w = 1 if d < 128 else 4
    sizes = _class_sizes(n - 10)
    free = [c for c in range(n) if c not in star_a(n) and c not in STAR_B]
    classes, at = [], 0
    for m in sizes:
        classes.append(tuple(free[at:at + m]))
        at += m
    D = torch.zeros(G, n, d)
    codes = torch.zeros(G, B, n)
    units = []
    for g in range(G):
        perm = torch.randperm(d, generator=gen).tolist()
        blocks = [perm[i * w:(i + 1) * w] for i in range(12 + len(classes))]
        assert len(blocks[-1]) == w, "not enough coordinates for the planted blocks"
        v = 1.0 if w == 1 else 0.5
        for s, cols in enumerate((star_a(n), STAR_B)):
            for i, c in enumerate(cols):
                D[g, c, blocks[6 * s]] = v * (1 << s)
                D[g, c, blocks[6 * s + 1 + i]] = v * (1 << s)
        for k, cols in enumerate(classes):
            for c in cols:
                D[g, c, blocks[12 + k]] = v * 2.0 ** (c % 3 - 1)
        units.append([star_a(n), STAR_B] + classes)

        def code():
            return 2.0 ** int(torch.randint(-2, 3, (1,), generator=gen))

        for r in range(B):
            if r == len(PLANTED_L):                     # all n columns active
                for cols in units[g]:
                    codes[g, r, list(cols)] = code()
                continue
            L = PLANTED_L[r] if r < len(PLANTED_L) else int(torch.randint(0, 49, (1,), generator=gen))
            rest = L
            if L >= 5:
                codes[g, r, list(star_a(n))] = code()
                rest -= 5
            if L >= 10 and L not in (17, 33):
                codes[g, r, list(STAR_B)] = code()
                rest -= 5
            used = set()
            for m in _class_sizes(rest):
                k = min((k for k, cols in enumerate(classes) if len(cols) >= m and k not in used),
                        key=lambda k: len(classes[k]))
                used.add(k)
                pick = torch.randperm(len(classes[k]), generator=gen)[:m].tolist()
                codes[g, r, [classes[k][i] for i in pick]] = code()
    return D.to(torch.bfloat16), codes, units


def random_case(n, d, seed=0, density=0.1):
    """(D bf16 [G, n, d], dense codes fp32 [G, B, n]): atoms ``normalize(u + 0.7 noise)``; codes about
    ``density`` dense with bf16-representable values, row 0 empty and row 1 all active."""
    gen = torch.Generator().manual_seed(2000 * seed + n + d)
    unit = lambda t: t / t.norm(dim=-1, keepdim=True)
    u = unit(torch.randn(d, generator=gen))
    noise = torch.randn(G, n, d, generator=gen)
    noise = unit(noise - (noise @ u).unsqueeze(-1) * u)  # unit and orthogonal to u: cos >= (1 - 0.49) / 1.49
    D = unit(u + 0.7 * noise).to(torch.bfloat16)
    c = (torch.rand(G, B, n, generator=gen) * 4 + 0.01).to(torch.bfloat16).float()
    c = torch.where(torch.rand(G, B, n, generator=gen) < density, c, torch.zeros_like(c))
    c[:, 0] = 0
    c[:, 1] = (torch.rand(G, n, generator=gen) + 0.5).to(torch.bfloat16).float()
    return D, c


def min_offdiag_cos2(D):
    """Smallest cos^2 between two different atoms of the same model, in fp64."""
    Dd = D.double()
    Dd = Dd / Dd.norm(dim=-1, keepdim=True)
    cos2 = (Dd @ Dd.transpose(1, 2)) ** 2
    eye = torch.eye(D.shape[1], dtype=torch.bool)
    return float(cos2.masked_fill(eye, 1.0).min())


def entry_bound(ref, d):
    """Per-entry bound on |cap - cap_ref| for the fp32 kernel against the fp64 oracle ``ref``
    (``ActiveCapacity``): ``cap_ref [(4 eta + 4 eta^2 + 2^-21) S / total + (L + 2) 2^-24] + 2^-33`` with
    eta = d 2^-23 the fp32-accumulation bound of a Gram entry and of a squared norm, S the sum of the row's
    codes and L its length.  (cos^2 carries two Gram and two norm errors: (1 + eta)^4 - 1 <= 4 eta + 4 eta^2 +
    ..., the 2^-21 covers the square, the product, the division and the multiplication by the code; the
    sum of L terms and the final division add (L + 2) 2^-24; 2^-33 is half a quantum of qsum.)"""
    eta = d * 2.0 ** -23
    total = ref.entry_total.clamp(min=1e-300)
    rel = (4 * eta + 4 * eta ** 2 + 2.0 ** -21) * ref.entry_csum / total + (ref.entry_len.double() + 2) * 2.0 ** -24
    return ref.entry_cap * rel + 2.0 ** -33
