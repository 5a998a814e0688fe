"""CPU: the host half of the segmented search (rfx_search_segmented: one launch for questions under
different metadata filters).  The library exports and declares the new entry points; rfx_segmented_plan,
a pure host function, cuts every group's selected rows into work items that tile them exactly once and
refuses every malformed input; rfx.filters.group_by_filter groups batch items by filter."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rfx.h")
NEW = ("rfx_search_segmented_workspace_bytes", "rfx_search_segmented", "rfx_segmented_plan")
L = 64  # chunks per group at most (rfx.index.SEGMENT_LISTS)


def test_symbols_exported_and_declared():
    from rfx import _lib, index
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rfx_\w+)", out))
    declared = set(re.findall(r"^\s*(?:const char\*|int)\s+(rfx_\w+)\s*\(", open(HEADER).read(), re.M))
    for s in NEW:
        assert s in exported and s in declared and s in _lib.SIGNATURES, s
    assert index.SEGMENT_LISTS == L


def arrays(groups):
    """[(n queries, [(first, count), ...])] -> (nq, group_q, group_r, ranges)"""
    gq, gr, flat = [0], [0], []
    for n, rngs in groups:
        gq.append(gq[-1] + n)
        flat += [v for fc in rngs for v in fc]
        gr.append(len(flat) // 2)
    return gq[-1], gq, gr, flat


def plan(rows, groups, k=10, dim=768, dtype="bf16"):
    from rfx.index import segmented_plan
    nq, gq, gr, flat = arrays(groups)
    return segmented_plan(rows, dim, dtype, nq, k, gq, gr, flat)


def check_tiling(rows, groups, **kw):
    """The properties every plan has; returns (items, lists)."""
    items, lists = plan(rows, groups, **kw)
    nq, gq, gr, flat = arrays(groups)
    assert 1 <= lists <= L
    sizes = items[:, 3]
    assert (np.diff(sizes) <= 0).all(), "heaviest items first"
    for g, (n, rngs) in enumerate(groups):
        mine = items[items[:, 0] == g]
        total = sum(c for _, c in rngs)
        if n == 0 or total == 0:
            assert len(mine) == 0
            continue
        # slices: first queries gq[g], gq[g] + 8, ...; each holds at most 8 queries of this group only
        firsts = sorted(set(mine[:, 1].tolist()))
        assert firsts == list(range(gq[g], gq[g + 1], 8))
        for q0 in firsts:
            assert min(8, gq[g + 1] - q0) >= 1
            chunks = mine[mine[:, 1] == q0]
            chunks = chunks[np.argsort(chunks[:, 2])]
            assert len(chunks) <= lists <= L
            # the chunks tile positions [0, total) exactly once: no gap, no overlap
            assert chunks[0, 2] == 0
            assert (chunks[1:, 2] == chunks[:-1, 2] + chunks[:-1, 3]).all()
            assert chunks[-1, 2] + chunks[-1, 3] == total
            assert (chunks[:, 3] > 0).all()
    return items, lists


def spans(rngs, pos0, n):
    """How many of the group's ranges the chunk of positions [pos0, pos0 + n) touches."""
    ends = np.cumsum([c for _, c in rngs])
    starts = ends - np.array([c for _, c in rngs])
    return int(((starts < pos0 + n) & (ends > pos0)).sum())


FILE_RANGES = [(0, 7), (31, 2), (1000, 337)]


def test_plan_tiles_each_group_once():
    groups = [(1, [(0, 20_011)]), (8, FILE_RANGES), (9, [(5, 1)]), (40, [(0, 7), (31, 2), (1000, 337), (15_000, 5011)]),
              (3, []), (0, [(0, 100)])]
    items, lists = check_tiling(20_011, groups)
    # a group with no range, and a group with no query, yield no item
    assert not (items[:, 0] == 4).any() and not (items[:, 0] == 5).any()
    # 9 queries: two slices; 40 queries: five
    assert len(set(items[items[:, 0] == 2][:, 1].tolist())) == 2
    assert len(set(items[items[:, 0] == 3][:, 1].tolist())) == 5
    # the whole-store group is cut into several chunks, never more than L
    assert 2 <= len(items[items[:, 0] == 0]) <= L
    assert lists == len(items[items[:, 0] == 0])


def test_chunk_spans_two_ranges():
    items, _ = check_tiling(2000, [(1, FILE_RANGES)])
    assert max(spans(FILE_RANGES, int(p), int(n)) for _, _, p, n in items) >= 2
    # 346 selected rows in chunks of at least 128 rows: the first chunk covers (0,7), (31,2) and part of (1000,337)
    first = items[items[:, 2] == 0][0]
    assert spans(FILE_RANGES, 0, int(first[3])) == 3


@pytest.mark.parametrize("rows_g", [1, 127, 128, 129, 8192, 8193, 1_000_000, 9_999_999])
def test_chunk_counts(rows_g):
    items, lists = check_tiling(10_000_000, [(1, [(0, rows_g)])])
    chunk = max(128, -(-rows_g // L))
    chunk = -(-chunk // 64) * 64
    assert len(items) == -(-rows_g // chunk) == lists
    assert (items[:, 3] <= chunk).all()


def test_many_small_ranges():
    rngs = [(10 * i, 3) for i in range(500)]
    items, _ = check_tiling(5000, [(2, rngs), (1, rngs[:1])])
    assert max(spans(rngs, int(p), int(n)) for g, _, p, n in items if g == 0) > 40


def test_empty_calls():
    items, lists = plan(100, [])
    assert len(items) == 0 and lists == 1
    items, lists = plan(100, [(4, [])])
    assert len(items) == 0 and lists == 1


BAD = {
    "unsorted": (100, 1, [0, 1], [0, 2], [50, 5, 10, 5]),
    "overlapping": (100, 1, [0, 1], [0, 2], [10, 5, 14, 5]),
    "past the end": (100, 1, [0, 1], [0, 1], [96, 5]),
    "negative first": (100, 1, [0, 1], [0, 1], [-1, 5]),
    "first at rows": (100, 1, [0, 1], [0, 1], [100, 1]),
    "count zero": (100, 1, [0, 1], [0, 1], [10, 0]),
    "count negative": (100, 1, [0, 1], [0, 1], [10, -3]),
    "huge count": (100, 1, [0, 1], [0, 1], [10, 2 ** 62]),
    "group_q not monotone": (100, 4, [0, 3, 2, 4], [0, 1, 2, 3], [0, 1, 2, 1, 4, 1]),
    "group_r not monotone": (100, 3, [0, 1, 2, 3], [0, 2, 1, 3], [0, 1, 2, 1, 4, 1]),
    "group_q[0] != 0": (100, 2, [1, 2], [0, 1], [0, 1]),
    "group_r[0] != 0": (100, 2, [0, 2], [1, 1], [0, 1]),
    "group_q[n] != nq": (100, 5, [0, 2, 4], [0, 1, 2], [0, 1, 2, 1]),
    "group_q beyond nq": (100, 3, [0, 4, 3], [0, 1, 2], [0, 1, 2, 1]),
    "queries without a group": (100, 2, [0], [0], []),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_plan_rejects(name):
    from rfx.index import segmented_plan
    rows, nq, gq, gr, flat = BAD[name]
    with pytest.raises(ValueError):
        segmented_plan(rows, 768, "bf16", nq, 10, gq, gr, flat)


@pytest.mark.parametrize("k,nq", [(0, 1), (65, 1), (-1, 1), (10, 1025), (10, -1)])
def test_plan_rejects_k_and_nq(k, nq):
    from rfx.index import segmented_plan
    with pytest.raises(ValueError):
        segmented_plan(100, 768, "bf16", nq, k, [0, nq], [0, 1], [0, 10])


def test_plan_accepts_the_batchers_max_batch():
    items, _ = check_tiling(1000, [(256, [(0, 1000)])], k=64)
    assert len(set(items[:, 1].tolist())) == 32
    check_tiling(1000, [(1, [(i, 1)]) for i in range(256)], k=1)
    for dim, dt in ((256, "f32"), (1024, "f16"), (1024, "f32"), (64, "bf16")):
        check_tiling(1000, [(3, [(0, 1000)])], dim=dim, dtype=dt)


def test_plan_rejects_bad_dim():
    from rfx.index import segmented_plan
    with pytest.raises(ValueError):
        segmented_plan(100, 100, "bf16", 1, 10, [0, 1], [0, 1], [0, 10])


def test_pack_groups():
    from rfx.index import pack_groups
    perm, gq, gr, flat = pack_groups(5, [([3, 0], [(0, 7), (31, 2)]), ([], [(4, 1)]), ([1, 2, 4], [])])
    assert perm == [3, 0, 1, 2, 4]
    assert gq.tolist() == [0, 2, 2, 5] and gr.tolist() == [0, 2, 3, 3] and flat.tolist() == [0, 7, 31, 2, 4, 1]
    for bad in ([([0, 1], [])], [([0, 1, 1], [])], [([0, 1, 3], [])]):
        with pytest.raises(ValueError):
            pack_groups(3, bad)


def test_group_by_filter():
    from rfx import filters
    fs = [{"tenant": "a", "year": 2020}, {"tenant": "b"}, {"year": 2020, "tenant": "a"}, {"tenant": ["a", "b"]},
          {"tenant": "b"}, {"tenant": ["b", "a"]}]
    groups = filters.group_by_filter(fs)
    # equal filters written with another key order share a group; a list's order is part of the filter
    assert [idxs for _, idxs in groups] == [[0, 2], [1, 4], [3], [5]]
    assert [f for f, _ in groups] == [fs[0], fs[1], fs[3], fs[5]]
    assert filters.group_by_filter([]) == []
