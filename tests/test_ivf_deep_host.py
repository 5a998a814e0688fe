"""CPU: the host side of the IVF deep search: argument errors of the C ABI that need no device,
the slab stride (rfx_ivf_deep_qcap) and the RFX_IVF_DEEP switch."""
import ctypes

import numpy as np
import pytest

from rfx import _lib
from rfx.ivf import deep_qcap
from rfx.store import ivf_deep_mode


@pytest.mark.parametrize("k", [64, 1025])
def test_k_out_of_range(k):
    b = ctypes.c_size_t()
    for rc in (_lib.lib.rfx_ivf_search_deep_workspace_bytes(0, 1, k, 4, ctypes.byref(b)),
               _lib.lib.rfx_ivf_deep_rerank_workspace_bytes(0, 1, k, 4, 1024, ctypes.byref(b)),
               _lib.lib.rfx_ivf_search_deep(0, None, 1, 1, k, 4, None, 0, None, None, None, 0, None)):
        with pytest.raises(ValueError, match=r"out of range \[65, 1024\]"):
            _lib.check(rc)


def test_handle_and_rerank_k():
    b = ctypes.c_size_t()
    with pytest.raises(ValueError, match="unknown IVF handle"):
        _lib.check(_lib.lib.rfx_ivf_search_deep_workspace_bytes(0, 1, 100, 4, ctypes.byref(b)))
    for rk in (99, 1025):
        with pytest.raises(ValueError, match=r"rerank_k=\d+ must be in \[k=100, 1024\]"):
            _lib.check(_lib.lib.rfx_ivf_deep_rerank_workspace_bytes(0, 1, 100, 4, rk, ctypes.byref(b)))


@pytest.mark.parametrize("nlist,nprobe", [(1, 1), (5, 3), (200, 64), (4096, 32)])
def test_qcap(nlist, nprobe):
    lens = np.random.default_rng(nlist).integers(0, 500, nlist)
    off = np.concatenate([[0], np.cumsum(lens)])
    want = int(np.sort(lens)[::-1][:nprobe].sum())
    assert deep_qcap(off, nprobe) == max(want + want % 2, 2)
    with pytest.raises(ValueError):
        deep_qcap(off, nlist + 1)


@pytest.mark.parametrize("value,on", [(None, False), ("0", False), ("1", True), (" 1 ", True), ("auto", False)])
def test_switch(monkeypatch, value, on):
    monkeypatch.delenv("RFX_IVF_DEEP", raising=False)
    if value is not None:
        monkeypatch.setenv("RFX_IVF_DEEP", value)
    assert ivf_deep_mode() is on
