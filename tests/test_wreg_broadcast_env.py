"""The FMA_WREG_BROADCAST switch of the k<=64 register LDL (no GPU needed)."""

import pytest

from flink_ms_amd import ops


def test_default_is_readlane(monkeypatch):
    monkeypatch.delenv("FMA_WREG_BROADCAST", raising=False)
    assert ops._wreg_broadcast() == 3


@pytest.mark.parametrize("name,variant", [("shfl", 0), ("panel", 1),
                                          ("subst", 2), ("readlane", 3)])
def test_named_variants(monkeypatch, name, variant):
    monkeypatch.setenv("FMA_WREG_BROADCAST", name)
    assert ops._wreg_broadcast() == variant


def test_unknown_variant_is_an_error(monkeypatch):
    monkeypatch.setenv("FMA_WREG_BROADCAST", "bpermute")
    with pytest.raises(ValueError, match="FMA_WREG_BROADCAST"):
        ops._wreg_broadcast()
