"""The store-policy knob (``ops.store_policy``) without a GPU: parsing, range errors, the environment
override, the per-epilogue override, the span predicate and the bits handed to the row-Adam launchers."""

import pytest

from sparse_coding__amd.ops import adam as adam_ops
from sparse_coding__amd.ops import store_policy as sp


@pytest.fixture(autouse=True)
def _restore():
    before, epi = sp.store_policy(), dict(sp._EPI)
    yield
    sp.set_store_policy(before)
    sp._EPI.clear()
    sp._EPI.update(epi)


def test_set_and_get_every_value():
    for pol in range(8):
        sp.set_store_policy(pol)
        assert sp.store_policy() == pol
        assert sp.tail_bits() == (pol >> 1) << 2
        assert bool(sp.gemm_write_through(0, 1024)) == bool(pol & sp.GEMM_OUT)


@pytest.mark.parametrize("bad", (-1, 8, 99, "x", None, "1.5"))
def test_out_of_range_is_refused(bad):
    sp.set_store_policy(5)
    with pytest.raises(ValueError):
        sp.set_store_policy(bad)
    assert sp.store_policy() == 5


def test_environment_override(monkeypatch):
    monkeypatch.delenv("SC_STORE_POLICY", raising=False)
    monkeypatch.delenv("SC_STORE_POLICY_EPI", raising=False)
    assert sp._env() == (sp.DEFAULT_STORE_POLICY, {})
    monkeypatch.setenv("SC_STORE_POLICY", " 6 ")
    monkeypatch.setenv("SC_STORE_POLICY_EPI", "0:1, 1:0,7:1,")
    assert sp._env() == (6, {0: True, 1: False, 7: True})
    for bad in ("8", "-1", "seven"):
        monkeypatch.setenv("SC_STORE_POLICY", bad)
        with pytest.raises(ValueError, match="SC_STORE_POLICY"):
            sp._env()
    monkeypatch.setenv("SC_STORE_POLICY", "1")
    for bad in ("0", "0:2", "a:1", "0:1:1", "-1:1"):
        monkeypatch.setenv("SC_STORE_POLICY_EPI", bad)
        with pytest.raises(ValueError, match="SC_STORE_POLICY_EPI"):
            sp._env()


def test_epilogue_override_beats_bit_0():
    sp.set_store_policy(sp.GEMM_OUT)
    sp.set_epilogue_override(1, False)
    assert sp.gemm_write_through(0, 1024) and not sp.gemm_write_through(1, 1024)
    sp.set_store_policy(0)
    sp.set_epilogue_override(3, True)
    assert sp.gemm_write_through(3, 1024) and not sp.gemm_write_through(0, 1024)
    sp.set_epilogue_override(3, None)
    assert not sp.gemm_write_through(3, 1024)


def test_span_guard_on_fabricated_sizes():
    sp.set_store_policy(7)
    assert sp.MAX_STORE_SPAN == 2 ** 31 - 1
    assert sp.output_span_bytes(1 << 15, 1 << 14, 1 << 14, 4) == 2 ** 31
    assert sp.output_span_bytes(256, 128, 512, 2) == (255 * 512 + 128) * 2
    assert sp.gemm_write_through(3, 2 ** 31 - 2)
    assert not sp.gemm_write_through(3, 2 ** 31 - 1) and not sp.gemm_write_through(3, 2 ** 31)
    sp.set_epilogue_override(3, True)
    assert not sp.gemm_write_through(3, 2 ** 31)  # an override cannot lift the guard


def test_row_adam_policy_argument_carries_the_tail_bits():
    """Bits 0-1 stay the launch policy of ``ops.adam`` (its range and default untouched); the store
    policy's tail bits sit above them."""
    before = adam_ops.policy()
    try:
        assert adam_ops.DEFAULT_POLICY == 3 and (adam_ops.POLICY_NT_LOAD, adam_ops.POLICY_NT_STORE) == (1, 2)
        for tail in range(4):
            adam_ops.set_policy(tail)
            for pol in range(8):
                sp.set_store_policy(pol)
                arg = adam_ops._launch_policy()
                assert arg & 3 == tail and arg >> 2 == pol >> 1 and 0 <= arg <= 15
        with pytest.raises(ValueError):
            adam_ops.set_policy(4)
    finally:
        adam_ops.set_policy(before)
