"""CPU: the host half of diversified retrieval (rfx_mmr_select).  The library exports and
declares the two entry points; the reference of the rule (tests/mmr_ref.py) has the two properties the
contract promises — lambda = 1 is the identity on the valid candidates, selections are prefix-stable — and
does not pick an exact duplicate second; the retriever's diversity argument is validated on the host."""
import os
import re
import subprocess

import numpy as np
import pytest

import mmr_ref
from oracle import synth as osynth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rfx.h")
NEW = ("rfx_mmr_workspace_bytes", "rfx_mmr_select")


def test_symbols_exported_and_declared():
    from rfx import _lib, index
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rfx_\w+)", out))
    declared = set(re.findall(r"^\s*(?:const char\*|int)\s+(rfx_\w+)\s*\(", open(HEADER).read(), re.M))
    for s in NEW:
        assert s in exported and s in declared and s in _lib.SIGNATURES, s
    assert hasattr(index.DeviceIndex, "mmr_select") and hasattr(index.DeviceIndex, "search_mmr")


def candidates(rows64, q64, n):
    """The search's answer at k = n: fl32 of the f64 dot, score desc then row asc."""
    s = (rows64 @ q64).astype(np.float32)
    s[np.isnan(s)] = -np.inf
    order = np.lexsort((np.arange(len(s)), -s.astype(np.float64)))[:n]
    return s[order], order.astype(np.int64)


@pytest.fixture(scope="module")
def corpus():
    rows = osynth.to_f64(osynth.synth_rows(7, 0, 96, 64, "f32"), "f32")
    q = osynth.to_f64(osynth.synth_rows(11, 0, 4, 64, "f32"), "f32")
    return rows, q


def test_lambda_one_is_the_first_k_valid(corpus):
    rows, q = corpus
    rows = rows.copy()
    for qi in range(len(q)):
        cs, cr = candidates(rows, q[qi], 24)
        s, r, _, _ = mmr_ref.select(cs, cr, rows, 10, 1.0)
        assert np.array_equal(r, cr[:10]) and s.tobytes() == cs[:10].tobytes()
    # padding (row -1, a tombstoned row) never takes part: the first k VALID candidates
    cs, cr = candidates(rows, q[0], 24)
    cr = cr.copy()
    dead = int(cr[2])
    cr[4] = -1
    rows[dead] = np.nan
    s, r, _, _ = mmr_ref.select(cs, cr, rows, 10, 1.0)
    keep = [i for i in range(24) if i not in (2, 4)][:10]
    assert np.array_equal(r, cr[keep]) and s.tobytes() == cs[keep].tobytes()
    # fewer valid candidates than k: (-inf, -1) at the tail
    s, r, o, _ = mmr_ref.select(cs[:5], cr[:5], rows, 6, 0.5)
    assert (r[:3] >= 0).all() and (r[3:] == -1).all() and np.isneginf(s[3:]).all() and np.isneginf(o[3:]).all()


@pytest.mark.parametrize("lam", [0.0, 0.3, 0.5, 0.7])
def test_prefix_stable(corpus, lam):
    rows, q = corpus
    for qi in range(len(q)):
        cs, cr = candidates(rows, q[qi], 48)
        s32, r32, o32, _ = mmr_ref.select(cs, cr, rows, 32, lam)
        for k in (1, 10, 31):
            s, r, o, _ = mmr_ref.select(cs, cr, rows, k, lam)
            assert np.array_equal(r, r32[:k]) and s.tobytes() == s32[:k].tobytes() and np.array_equal(o, o32[:k])
        assert len(set(r32.tolist())) == 32
        mmr_ref.check_valid(s32, r32, cs, cr)


def test_exact_duplicate_is_not_picked_second(corpus):
    rows, _ = corpus
    rows = rows.copy()
    rows[20] = rows[3]  # a re-uploaded chunk
    q = 0.8 * rows[3] + 0.6 * rows[7]
    cs, cr = candidates(rows, q, 16)
    assert cr[:2].tolist() == [3, 20] and cs[0] == cs[1]  # the plain top 2 are the two copies
    s, r, o, _ = mmr_ref.select(cs, cr, rows, 4, 0.5)
    assert r[0] == 3 and r[1] != 20
    assert r[1] == 7  # relevance 0.6, nearly orthogonal to the pick: 0.5 * 0.6 - 0.5 * ~0 beats 0.5 * 0.8 - 0.5 * 1
    # at lambda 1 the copy is second
    assert mmr_ref.select(cs, cr, rows, 4, 1.0)[1][:2].tolist() == [3, 20]


def test_batch_form_and_per_query_arguments(corpus):
    rows, q = corpus
    cands = [candidates(rows, q[qi], 32) for qi in range(len(q))]
    cs, cr = np.stack([c[0] for c in cands]), np.stack([c[1] for c in cands])
    lam, nc = [0.2, 1.0, 0.5, 0.9], [32, 7, 16, 8]
    s, r, o, m = mmr_ref.select_batch(cs, cr, rows, 7, lam, nc)
    for qi in range(len(q)):
        s1, r1, o1, m1 = mmr_ref.select(cs[qi], cr[qi], rows, 7, lam[qi], nc[qi])
        assert np.array_equal(r[qi], r1) and s[qi].tobytes() == s1.tobytes() and m[qi] == m1
        assert set(r1.tolist()) <= set(cr[qi, :nc[qi]].tolist())
    assert np.array_equal(r[1], cr[1, :7])  # lambda 1


def test_diversity_argument():
    from rfx.retriever import default_fetch_k, parse_diversity
    assert [default_fetch_k(k) for k in (1, 4, 5, 10, 16, 64)] == [16, 16, 20, 40, 64, 64]
    assert parse_diversity(None, 5) is None
    assert parse_diversity(0.5, 5) == (0.5, 20)
    assert parse_diversity({"lambda": 1, "fetch_k": 5}, 5) == (1.0, 5)
    for bad in (-0.1, 1.5, float("nan"), "0.5", True, {"fetch_k": 20}, {"lambda": 0.5, "fetch_k": 4},
                {"lambda": 0.5, "fetch_k": 65}, {"lambda": 0.5, "k": 3}):
        with pytest.raises(ValueError):
            parse_diversity(bad, 5)
