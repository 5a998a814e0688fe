"""CPU: the deep MMR selection's host side — the exports, the plan's slice and workspace
arithmetic (rfx_mmr_deep_plan, csrc/mmr_deep_plan.h), parse_diversity_deep, and the two properties of the rule's
reference (tests/mmr_ref.py) at 1,024 candidates."""
import numpy as np
import pytest

import mmr_ref
from test_host_lib import declared_symbols


def test_exports_declared_and_bound():
    from rfx import _lib
    for name in ("rfx_mmr_deep_workspace_bytes", "rfx_mmr_select_deep", "rfx_mmr_deep_plan"):
        assert name in declared_symbols() and name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.SIGNATURES["rfx_mmr_select_deep"] == _lib.SIGNATURES["rfx_mmr_select"]  # the same argument list


@pytest.mark.parametrize("nq,n_max,n_pad,slice_q", [(1, 65, 128, 1), (1024, 128, 128, 1024), (1024, 256, 256, 1024),
                                                    (1024, 257, 320, 1024), (1024, 1000, 1024, 128),
                                                    (129, 1024, 1024, 128), (128, 1024, 1024, 128), (300, 700, 704, 270)])
def test_plan(nq, n_max, n_pad, slice_q):
    from rfx.index import mmr_deep_plan
    got_pad, pairs, got_slice, slices, total = mmr_deep_plan(nq, n_max)
    tiles = n_pad // 64
    assert (got_pad, pairs, got_slice) == (n_pad, tiles * (tiles + 1) // 2, slice_q)
    assert slices == -(-nq // slice_q)
    mats = slice_q * n_pad * n_pad * 4
    assert mats <= 512 << 20 and (slice_q == nq or (slice_q + 1) * n_pad * n_pad * 4 > 512 << 20)
    # the matrices, the bit matrix, the norms and flags of a slice, the call's tables and stats; 256-byte pieces
    rest = slice_q * (n_pad * n_pad // 8 + n_pad * 5) + nq * 16
    assert mats + rest <= total <= mats + rest + 6 * 256


@pytest.mark.parametrize("nq,n_max", [(0, 128), (1025, 128), (4, 64), (4, 1025)])
def test_plan_refuses(nq, n_max):
    from rfx.index import mmr_deep_plan
    with pytest.raises(ValueError):
        mmr_deep_plan(nq, n_max)


def test_parse_diversity_deep():
    from rfx.retriever import parse_diversity, parse_diversity_deep
    assert parse_diversity_deep(None, 100) is None
    assert parse_diversity_deep(0.5, 10) == (0.5, 65) and parse_diversity_deep(0.5, 100) == (0.5, 400)
    assert parse_diversity_deep(1, 300) == (1.0, 1024) and parse_diversity_deep(0.0, 1024) == (0.0, 1024)
    assert parse_diversity_deep({"lambda": 0.25, "fetch_k": 200}, 10) == (0.25, 200)
    assert parse_diversity_deep({"lambda": 0.25, "fetch_k": 65}, 65) == (0.25, 65)
    for bad, k in ((1.5, 100), (float("nan"), 100), (True, 100), ("0.5", 100), ({"fetch_k": 200}, 100),
                   ({"lambda": 0.5, "fetch_k": 64}, 10), ({"lambda": 0.5, "fetch_k": 1025}, 100),
                   ({"lambda": 0.5, "fetch_k": 100}, 101), ({"lambda": 0.5, "fetch_k": 128.0}, 100),
                   ({"lambda": 0.5, "depth": 3}, 100)):
        with pytest.raises(ValueError):
            parse_diversity_deep(bad, k)
    with pytest.raises(ValueError):  # the shallow form keeps its cap
        parse_diversity({"lambda": 0.5, "fetch_k": 65}, 10)


def test_reference_properties_at_1024():
    rng = np.random.default_rng(2)
    centres = rng.standard_normal((40, 64))
    rows64 = centres[rng.integers(0, 40, 1500)] + 0.3 * rng.standard_normal((1500, 64))
    rows64 = rows64.astype(np.float32).astype(np.float64)
    qv = rng.standard_normal(64)
    order = np.argsort(-(rows64 @ qv), kind="stable")[:1024]
    cs, cr = (rows64[order] @ qv).astype(np.float32), order.astype(np.int64)
    s1, r1, _, _ = mmr_ref.select(cs, cr, rows64, 200, 1.0)
    assert np.array_equal(r1, cr[:200]) and s1.tobytes() == cs[:200].tobytes()  # lambda 1: the identity
    s200, r200, o200, _ = mmr_ref.select(cs, cr, rows64, 200, 0.4)
    s64, r64, o64, _ = mmr_ref.select(cs, cr, rows64, 64, 0.4)
    assert np.array_equal(r200[:64], r64) and np.array_equal(s200[:64], s64) and np.array_equal(o200[:64], o64)
    assert not np.array_equal(r200, cr[:200])
    mmr_ref.check_valid(s200, r200, cs, cr)
