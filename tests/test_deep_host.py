"""CPU: the work split of the deep search (rfx_deep_plan, csrc/deep_plan.h) and its argument errors."""
import pytest

from rfx import _lib
from rfx.index import deep_plan

LDS_BUDGET = 160 * 1024  # kDeepLdsBudget


@pytest.mark.parametrize("nq", [1, 17, 1024])
@pytest.mark.parametrize("k", [65, 128, 129, 1024])
@pytest.mark.parametrize("rows", [1, 70, 4 * 128, 4 * 128 + 1, 1 << 20])
def test_plan(rows, k, nq):
    ranges, rpr, kb, q_per_wg = deep_plan(rows, 768, "bf16", nq, k)
    assert kb >= k and kb in (128, 256, 512, 1024) and (kb == 128 or kb // 2 < k)
    # range i = [i * rpr, (i + 1) * rpr), the last one to the end of the store: every row exactly once
    bounds = [i * rpr for i in range(ranges)] + [rows]
    sizes = [b - a for a, b in zip(bounds, bounds[1:])]
    assert ranges >= 1 and sum(sizes) == rows and all(s > 0 for s in sizes)
    assert rpr % 64 == 0, "a range starts on a round of 4 waves x 16 rows (and on a mask word's half)"
    if ranges > 1:
        assert min(sizes) >= 4 * kb
    assert q_per_wg >= 1 and q_per_wg * 2 * kb * 8 <= LDS_BUDGET
    if rows == 1 << 20 and nq == 1:
        assert ranges > 1


@pytest.mark.parametrize("k", [64, 1025])
def test_k_out_of_range(k):
    with pytest.raises(ValueError, match=r"out of range \[65, 1024\]"):  # RFX_EINVAL
        deep_plan(1000, 768, "bf16", 1, k)
    with pytest.raises(_lib.RfxError, match="bf16 and f16 stores only"):  # RFX_EUNSUPPORTED
        deep_plan(1000, 768, "f32", 1, 100)
