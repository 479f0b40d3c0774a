"""Which step outputs are written through the L2 (``sc1`` stores, ``csrc/common.h`` ``st_pol``).

MI355X's eight XCD-private L2s are write-back and not coherent with each other, so the release at the
end of a kernel writes every dirty line back before the dependent kernel may start.  A written-through
store leaves the L2 while the kernel is still computing.  Cache policy only: every value writes the
same bits (``tests/test_store_policy_gpu.py``).

Bits of the knob:

* ``GEMM_OUT`` (1): the GEMM epilogues' output tiles and activity-mask words;
* ``TAIL_PMV`` (2): the step tail's / row Adam's fp32 ``p`` / ``m`` / ``v`` stores (on top of ``nt``);
* ``TAIL_AUX`` (4): the tail's bf16 shadow, row-norm and next-batch gather stores.

``SC_STORE_POLICY=<0..7>`` overrides the default (read once, at import), for same-box A/B runs of whole
steps; ``SC_STORE_POLICY_EPI="epi:0|1,..."`` (e.g. ``1:0,3:1``) overrides bit 0 for single GEMM epilogues
(the ``EPI_*`` numbers of ``ops/gemm.py``).  The default is bits 0 and 1: on the headline step 0.2605 vs
0.2631 ms at 200 / 20 (medians of 7 alternating runs, parent spread 0.0024); bit 0 carries the gain, mostly
through the code gradient's output, bit 1 adds a little, bit 2 nothing
(``profiles/r10/store_policy/README.md``).  Bits 1 and 2 act in the step tails only (``sc_adam_rows`` takes
and ignores them).
"""

from __future__ import annotations

import os

GEMM_OUT, TAIL_PMV, TAIL_AUX = 1, 2, 4
DEFAULT_STORE_POLICY = GEMM_OUT | TAIL_PMV

# A written-through store addresses its array through a buffer resource with 32-bit byte offsets
# (csrc/common.h store_rsrc): an output that spans this much or more keeps plain stores.
MAX_STORE_SPAN = 2 ** 31 - 1


def _parse_policy(spec, what="SC_STORE_POLICY") -> int:
    try:
        pol = int(spec)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be an integer in 0..7 (got {spec!r})") from None
    if not 0 <= pol <= 7:
        raise ValueError(f"{what} must be in 0..7 (got {spec!r})")
    return pol


def _parse_epi(spec: str) -> dict:
    """``"epi:flag,..."`` -> {epi: bool}; flags are 0 or 1."""
    out = {}
    for item in filter(None, (s.strip() for s in spec.split(","))):
        try:
            key, val = item.split(":")
            epi, flag = int(key), int(val)
        except ValueError:
            raise ValueError(f"SC_STORE_POLICY_EPI items are epi:0 or epi:1 (got {item!r})") from None
        if epi < 0 or flag not in (0, 1):
            raise ValueError(f"SC_STORE_POLICY_EPI items are epi:0 or epi:1 (got {item!r})")
        out[epi] = bool(flag)
    return out


def _env():
    spec = os.environ.get("SC_STORE_POLICY", "").strip()
    pol = _parse_policy(spec) if spec else DEFAULT_STORE_POLICY
    return pol, _parse_epi(os.environ.get("SC_STORE_POLICY_EPI", ""))


_POLICY, _EPI = _env()


def store_policy() -> int:
    return _POLICY


def set_store_policy(pol: int):
    """Select the store policy of the following launches (tests / A-B timing)."""
    global _POLICY
    _POLICY = _parse_policy(pol, "store policy")


def set_epilogue_override(epi: int, flag):
    """Write epilogue ``epi``'s outputs through (True) or not (False) whatever bit 0 says; None removes
    the override."""
    if flag is None:
        _EPI.pop(int(epi), None)
    else:
        _EPI[int(epi)] = bool(flag)


def span_ok(span_bytes: int) -> bool:
    """True when an output of ``span_bytes`` can be addressed by the written-through stores."""
    return int(span_bytes) < MAX_STORE_SPAN


def output_span_bytes(M: int, N: int, ldc: int, elem_size: int) -> int:
    """Bytes from a model's output base to the end of its last element ([M][ldc] rows, N used)."""
    return ((M - 1) * ldc + N) * elem_size


def gemm_write_through(epi: int, span_bytes: int) -> bool:
    """Whether the GEMM epilogue ``epi`` writes an output of ``span_bytes`` per model through: bit 0 of
    the knob (or the epilogue's override), and never beyond ``MAX_STORE_SPAN``."""
    want = _EPI.get(int(epi), bool(_POLICY & GEMM_OUT))
    return bool(want) and span_ok(span_bytes)


def tail_bits() -> int:
    """The knob's tail bits as the launchers pass them to the kernels: ORed into the row-Adam policy
    argument above its bits 0 and 1 (``csrc/adam.hip`` ``split_policy``)."""
    return ((_POLICY >> 1) & 3) << 2
