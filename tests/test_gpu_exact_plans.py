"""The plans of the exact scans, cell by cell, against a table recorded before the kernels were put behind one
descriptor table (tests/golden/exact_scan_plans.json): for every (dtype, dim, int8 copy, rows) store and every
(nq, k) the kernel rfx_search runs, the kernel and candidate count rfx_scan_topk plans, the list length and the
workspace size.  No scan is launched: the test builds the stores and asks.

Rows: plan_scan_screen's 2-wave wide form (k 11..64, up to 64 questions, and every d-1024 batch) cuts a store of
T 32-row tiles into min(512, max(T / 12, 8)) ranges, rounded down to a multiple of 8, with two lists a range, and
plans only with 64 lists or more: 32 ranges, T >= 384.  12,256 rows are 383 tiles (24 ranges, 48 lists: the exact
plans stay), 12,257 rows are 384 tiles (32 ranges, 64 lists: plan 12).
"""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = ("bf16", "f16", "f32")
DIMS = (768, 1024, 256)  # 256: served by kernels 1 and 2 (and the VALU scan) only
NQS = (9, 16, 17, 64, 65, 128, 129, 257)
KS = (4, 10, 11, 16, 17, 64)
ROWS = (12_256, 12_257)
KERNELS = {1, 2, 3, 6, 8, 9, 10, 12}


def _ask(fn, *a):
    """The value, or ["error", code] where the library refuses the cell."""
    from rfx import _lib
    try:
        v = fn(*a)
    except _lib.RfxError as e:
        return ["error", e.code]
    return list(v) if isinstance(v, tuple) else v


def collect():
    """{store key: {"screen": None or ["error", code], "cells": [[nq, k, search_plan, plan, list_len, ws], ...]}}"""
    import rfx.index as rindex
    out = {}
    for dtype in DTYPES:
        for dim in DIMS:
            for rows in ROWS:
                for copy in (0, 1):
                    ix = rindex.DeviceIndex(dim, dtype)
                    ix.add_synthetic(7, rows)
                    screen = _ask(ix.enable_screen, 1) if copy else None
                    cells = [[nq, k, _ask(ix.search_plan, nq, k), _ask(ix.plan, nq, k), _ask(ix.list_len, nq, k),
                              _ask(ix.workspace_bytes, nq, k)] for nq in NQS for k in KS]
                    out[f"{dtype}/{dim}/{rows}/int8={copy}"] = {"screen": screen, "cells": cells}
                    ix.close()
    return out


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "exact_scan_plans.json")) as f:
        return json.load(f)


def test_golden_holds_every_kernel(golden):
    assert len(golden) == len(DTYPES) * len(DIMS) * len(ROWS) * 2
    seen = set()
    for store in golden.values():
        assert [c[:2] for c in store["cells"]] == [[nq, k] for nq in NQS for k in KS]
        for _, _, search_plan, plan, _, _ in store["cells"]:
            if isinstance(search_plan, int):
                seen.add(search_plan)
            if plan[0] != "error":
                seen.add(plan[0])
    assert KERNELS <= seen, sorted(KERNELS - seen)


def test_plans_match_golden(golden):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    got = collect()
    assert sorted(got) == sorted(golden)
    for key, store in golden.items():
        assert got[key]["screen"] == store["screen"], key
        for want, have in zip(store["cells"], got[key]["cells"]):
            assert have == want, (key, "nq, k, search_plan, plan, list_len, workspace_bytes", want, have)
