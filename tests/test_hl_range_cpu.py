"""The f16hl range monitor's ABI (infur_hl_monitor_enable / infur_hl_range, ABI 7) without a GPU: declared, exported, bound in ctypes
and in the Rust -sys crate; the Python surface fails loudly where no device exists."""
import os
import re

import pytest

from infur_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("infur_hl_monitor_enable", "infur_hl_range")


def test_abi_version_is_7(lib):
    assert _lib.ABI_VERSION == 7 and lib.infur_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    assert re.search(r"#define INFUR_ABI_VERSION 7\b", header)
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    assert "pub const INFUR_ABI_VERSION: u32 = 7;" in rust


def test_monitor_exports_everywhere(lib):
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    assert "int32_t infur_hl_monitor_enable(infur_ctx* ctx, uint32_t on);" in header
    assert "int32_t infur_hl_range(infur_ctx* ctx, float* act_amax, float* wino_amax, uint32_t* saturated, uint32_t* nan_seen);" in header
    for s in EXPORTS:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
        assert re.search(rf"pub fn {s}\s*\(", rust), s
    assert len(_lib.SIGNATURES["infur_hl_range"][1]) == 5


def test_null_context_is_rejected(lib):
    assert lib.infur_hl_monitor_enable(None, 1) == _lib.E_INVALID_ARG
    assert lib.infur_hl_range(None, None, None, None, None) == _lib.E_INVALID_ARG


def test_monitored_context_without_gpu_fails_loudly(lib):
    if lib.infur_device_count() > 0:
        pytest.skip("a GPU is visible: the loud-failure path is covered on CPU-only hosts")
    from infur_amd.processors import Context, InfurError

    with pytest.raises(InfurError) as e:
        Context(device=0, dtype="f16hl", hl_monitor=True)
    assert e.value.code == _lib.E_HIP and "no CPU fallback" in str(e.value)
