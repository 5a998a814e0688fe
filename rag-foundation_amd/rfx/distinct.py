"""Distinct-document search: top-k DOCUMENTS, one best chunk each.

The rule.  Take the project's full ranking of the live rows the filter selects (fl32 of the f64 dot; score
desc, row asc).  Keep a row if no earlier row of the ranking belongs to the same file.  The answer is the
first k kept rows, in that order, then padding (-inf, -1).

This module is the host side, free of any device call: the `distinct` argument, and the rounds that turn
searches of at most 64 rows into that exact answer (`run_rounds`).  DeviceIndex.search_distinct supplies the
device operations (the searches the project already has, and the collapse kernel rfx_distinct_collapse);
the host tests supply numpy ones.
"""
import os

import numpy as np

from . import filters

DISTINCT_ERROR = "distinct needs a flat single-device store and neither diversity nor hybrid"
COMPLETION_K = 64  # a completion round fetches the longest list a search answers with


def default_fetch_k(k: int) -> int:
    """Rows round 1 fetches when the caller names no fetch_k: min(64, max(4k, 16)), as diversity does."""
    return min(64, max(4 * int(k), 16))


def env_default():
    """RFX_DISTINCT=0|1: what a question gets that passes no `distinct` (default 0: nothing changes)."""
    return True if os.environ.get("RFX_DISTINCT", "0").strip() == "1" else None


def parse_distinct(distinct, k: int):
    """distinct (None | False | True | {"fetch_k": n}) -> None or the fetch_k of round 1, k <= fetch_k <= 64."""
    if distinct is None or distinct is False:
        return None
    if distinct is True:
        fetch_k = None
    elif isinstance(distinct, dict):
        unknown = set(distinct) - {"fetch_k"}
        if unknown:
            raise ValueError(f"distinct takes 'fetch_k' only, got {sorted(distinct)}")
        fetch_k = distinct.get("fetch_k")
        if fetch_k is not None and (isinstance(fetch_k, bool) or not isinstance(fetch_k, int)):
            raise ValueError(f"distinct fetch_k={fetch_k!r} must be an integer")
    else:
        raise ValueError(f"distinct={distinct!r} must be None, True or {{'fetch_k': n}}")
    fetch_k = default_fetch_k(k) if fetch_k is None else int(fetch_k)
    if not int(k) <= fetch_k <= 64:
        raise ValueError(f"distinct fetch_k={fetch_k} must satisfy k={k} <= fetch_k <= 64")
    return fetch_k


class SegmentedUnsupported(Exception):
    """ops.segmented: the segmented search refuses this index's shape (RFX_EUNSUPPORTED)."""


def run_rounds(ops, nq: int, k: int, rows: int, doc_ranges, select_ranges=None) -> int:
    """The exact distinct-document search as a first round and completion rounds; returns the rounds run.

    ops (device or numpy):
      first()                     -> candidates: the plain search of all nq questions at fetch_k
      collapse(cand, have)        -> None: the collapse of `cand` into the picks; have False = round 1
                                     (nothing held yet), True = append to the counts of the round before
      read()                      -> (n [nq], done [nq], docs [nq][k]) on the host, numpy
      segmented(open_q, ranges)   -> candidates for all nq questions: question open_q[i] searched at
                                     COMPLETION_K over ranges[i], every other question padding; ONE search.
                                     Raises SegmentedUnsupported when the index refuses the shape
      masked(open_q, ranges)      -> the same answer from one masked search per open question
    doc_ranges [n_docs][2] = (first row, rows) of every document ordinal; select_ranges = the ascending
    disjoint (first, count) ranges the filter selects (None: all `rows`).

    Round 1 finds, for every question, the documents of its fetch_k best rows.  A question is done when it
    holds k documents or its list was not full (the search ran out of rows).  A completion round searches,
    for every open question, the selected rows WITHOUT the rows of the documents it has found: each of its
    candidates belongs to a document not seen before and ranks after every row of the rounds before, so the
    round either adds a document or exhausts the question — at most k rounds in all, which is asserted."""
    sel = filters.subtract_ranges(select_ranges if select_ranges is not None else [(0, int(rows))], [])
    doc_ranges = np.asarray(doc_ranges, dtype=np.int64).reshape(-1, 2)
    ops.collapse(ops.first(), False)
    rounds = 1
    n, done, docs = ops.read()
    done = np.asarray(done).astype(bool).copy()
    while not done.all():
        open_q, ranges = [], []
        for q in np.flatnonzero(~done):
            found = sorted((int(doc_ranges[d, 0]), int(doc_ranges[d, 1])) for d in docs[q, :n[q]])
            rest = filters.subtract_ranges(sel, found)
            if rest:
                open_q.append(int(q))
                ranges.append(rest)
            else:
                done[q] = True  # nothing left to search: exhausted
        if not open_q:
            break
        if rounds >= k:
            raise RuntimeError(f"distinct search: {len(open_q)} questions still open after {rounds} rounds at k={k}")
        try:
            cand = ops.segmented(open_q, ranges)
        except SegmentedUnsupported:
            cand = ops.masked(open_q, ranges)
        ops.collapse(cand, True)
        rounds += 1
        n2, done2, docs = ops.read()
        done2 = np.asarray(done2).astype(bool)
        stuck = [q for q in open_q if not (n2[q] > n[q] or done2[q])]
        if stuck:
            raise RuntimeError(f"distinct search: round {rounds} neither added a document nor exhausted "
                               f"questions {stuck[:8]}")
        done, n = done | done2, n2
    return rounds
