"""CPU: the plan of the sampled-threshold deep search (rfx_deep_sampled_plan, csrc/deep_sampled_plan.h; DESIGN
§4.20), its argument errors (rfx_search_deep's) and the export of its three symbols."""
import ctypes
import os
import subprocess

import pytest

from rfx import _lib
from rfx.index import deep_plan, deep_sampled_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rfx_deep_sampled_plan", "rfx_search_deep_sampled_workspace_bytes", "rfx_search_deep_sampled")


@pytest.mark.parametrize("nq", [1, 16, 17, 65, 130, 1024])
@pytest.mark.parametrize("k", [65, 128, 129, 1000, 1024])
@pytest.mark.parametrize("rows", [1, 70, 1000, 8 * 128, 8 * 128 + 1, 4113, 8 * 1024, 8 * 1024 + 1, 40001, 10_000_000])
def test_plan(rows, k, nq):
    dense, S, stride, cap, q_per_wg, ranges = deep_sampled_plan(rows, 768, "bf16", nq, k)
    kb = deep_plan(rows, 768, "bf16", nq, k)[2]
    assert dense == (rows <= 8 * kb)
    assert cap % 2 == 0
    if dense:
        assert S == 0 and rows <= cap <= rows + 1
    else:
        assert S >= 4 * kb and S % 16 == 0 and stride >= 1 and (S - 1) * stride < rows
        assert S * S >= 2 * kb * rows and cap == 2 * kb * -(-rows // S) + 64
    slab = max(S, cap)
    assert slab % 2 == 0
    assert q_per_wg == 16 if nq <= 16 else q_per_wg in (64, 128, 256)
    assert 1 <= ranges <= 512
    # (the workspace takes an index handle: tests/test_gpu_deep_sampled.py holds it to slabs + the parent's)
    assert deep_sampled_plan(rows, 1024, "f16", nq, k)[:4] == (dense, S, stride, cap), "the slab does not depend on dim"


@pytest.mark.parametrize("k", [64, 1025])
def test_argument_errors(k):
    with pytest.raises(ValueError, match=r"out of range \[65, 1024\]"):  # RFX_EINVAL, as rfx_deep_plan
        deep_sampled_plan(1000, 768, "bf16", 1, k)
    with pytest.raises(_lib.RfxError, match="bf16 and f16 stores only"):  # RFX_EUNSUPPORTED
        deep_sampled_plan(1000, 768, "f32", 1, 100)
    with pytest.raises(_lib.RfxError, match="dim % 64 == 0 up to 1024"):
        deep_sampled_plan(1000, 1088, "bf16", 1, 100)
    b = ctypes.c_size_t()
    rcs = [(_lib.lib.rfx_search_deep_workspace_bytes(0, 1, 100, ctypes.byref(b)),
            _lib.lib.rfx_search_deep_sampled_workspace_bytes(0, 1, 100, ctypes.byref(b))),
           (_lib.lib.rfx_search_deep(0, None, 1, 100, None, None, None, None, 0, None),
            _lib.lib.rfx_search_deep_sampled(0, None, 1, 100, None, None, None, None, 0, None))]
    assert all(a == b_ != 0 for a, b_ in rcs), rcs  # an unknown handle: the parent's code


def test_exports():
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    with open(os.path.join(ROOT, "include", "rfx.h"), encoding="utf-8") as f:
        header = f.read()
    for s in SYMBOLS:
        assert f" T {s}\n" in exported and f"int {s}(" in header and s in _lib.SIGNATURES, s
