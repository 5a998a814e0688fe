"""Reference and cases of the IVF search of a batch under different filters (rfx_ivf_search_multi).
TEST INFRASTRUCTURE ONLY (tests/test_ivf_multi_ref.py on the CPU, tests/test_gpu_ivf_multi.py on the GPU); numpy,
tests/ivf_mask_ref.py, oracle/ivf.py and the corpora of tests/hostile_ivf.py, all unchanged.

The reference is the rule itself: question q's answer is what the one-mask search returns for question q ALONE at
nprobes[q] under its own mask — ivf_mask_ref.search called once per question, the results stacked.  The three
mutants are what a wrong kernel would compute: every question under question 0's mask (one mask for the staged
batch), every question at the batch's largest probe count (the stride taken for the count, or stale candidates of
a wider call), and the mask applied to a finished unmasked top-k.  CASES is the GPU file's grid; the CPU file shows
that each mutant differs from the reference on every case where it can (more than one distinct mask in use, mixed
probe counts, a mask that is not all ones).
"""
import numpy as np

import ivf_mask_ref as mr

FULL = mr.FULL


# ---- the reference and its mutants ---------------------------------------------------------------------------
def _each(fn, qq, qinv, codes, inv, labels, qc, fc, nprobes, k, sels):
    out = [fn(qq[i:i + 1], qinv[i:i + 1], codes, inv, labels, qc, fc, int(nprobes[i]), k, sels[i])
           for i in range(len(qq))]
    return np.concatenate([s for s, _ in out]), np.concatenate([r for _, r in out])


def search(qq, qinv, codes, inv, labels, qc, fc, nprobes, k, sels):
    """sels: one selection (bool [n]) per question (all ones = no mask); nprobes: one probe count per question."""
    return _each(mr.search, qq, qinv, codes, inv, labels, qc, fc, nprobes, k, sels)


def brute_force(qq, qinv, codes, inv, labels, qc, fc, nprobes, k, sels):
    return _each(mr.brute_force, qq, qinv, codes, inv, labels, qc, fc, nprobes, k, sels)


def mutant_first_mask(qq, qinv, codes, inv, labels, qc, fc, nprobes, k, sels):
    return search(qq, qinv, codes, inv, labels, qc, fc, nprobes, k, [sels[0]] * len(sels))


def mutant_max_nprobe(qq, qinv, codes, inv, labels, qc, fc, nprobes, k, sels):
    return search(qq, qinv, codes, inv, labels, qc, fc, [max(nprobes)] * len(sels), k, sels)


def mutant_after_topk(qq, qinv, codes, inv, labels, qc, fc, nprobes, k, sels):
    return _each(mr.mutant_after_topk, qq, qinv, codes, inv, labels, qc, fc, nprobes, k, sels)


# ---- mask tables ---------------------------------------------------------------------------------------------
def selection(name, labels, splits=1, nq=1):
    """ivf_mask_ref.selection, plus "~name" (the complement) and "rot<i>" (one of nq distinct masks: the rows r
    with ((r + i) mod nq') even, nq' = nq made odd, so no two shifts agree)."""
    if name.startswith("~"):
        return ~selection(name[1:], labels, splits, nq)
    if name.startswith("rot"):
        m = nq | 1
        return ((np.arange(len(labels)) + int(name[3:])) % m) % 2 == 0
    return mr.selection(name, labels, splits)


TABLES = {
    "one": ["alt"],
    "comp": ["alt", "~alt"],            # complementary: a clear and a set bit of the same row in one staged batch
    "same": ["ranges", "ranges"],       # identical masks under two table indices
    "eight": ["ones", "zeros", "alt", "wordedge", "first", "last", "ranges", "~alt"],
    "nine": ["ones", "zeros", "alt", "wordedge", "first", "last", "ranges", "~alt", "few"],
    "nine_seedless": ["seedless", "zeros", "alt", "wordedge", "first", "last", "ranges", "~alt", "few"],
    "perq": None,                       # nq distinct masks rot0 .. rot<nq-1>
    "none": [],                         # no table: every mask_of entry is -1
}


def table_names(table, nq):
    return [f"rot{i}" for i in range(nq)] if table == "perq" else TABLES[table]


def mask_of(n_masks, nq, holes, order):
    """Each question's table index.  "group": the questions in filter-group order (blocks of equal indices);
    "shuffle": the same counts, interleaved by a fixed permutation.  holes: every fourth question (1, 5, 9 ..)
    takes no mask (-1); an empty table gives -1 throughout."""
    if n_masks == 0:
        return np.full(nq, -1, dtype=np.int32)
    mo = (np.arange(nq) * n_masks // nq).astype(np.int32) if nq >= n_masks else np.arange(nq, dtype=np.int32)
    if order == "shuffle":
        mo = mo[np.random.default_rng(5).permutation(nq)]
    if holes:
        mo[1::4] = -1
    return mo


def probe_counts(plan, nq, nlist):
    """"mix": 1 / 3 / every list in turn; "most1": 1 for all but every fifth question, which probes every list;
    an integer: all equal (FULL = every list, capped at 64)."""
    full = min(nlist, 64)
    if plan == "mix":
        return np.array([(1, 3, full)[i % 3] for i in range(nq)], dtype=np.int32)
    if plan == "most1":
        return np.array([full if i % 5 == 0 else 1 for i in range(nq)], dtype=np.int32)
    return np.full(nq, plan or full, dtype=np.int32)


# ---- the GPU file's grid: (corpus, table, holes, order, splits, k, nq, probes) -------------------------------
CASES = [
    ("edges", "one", False, "group", 1, 1, 1, 1),
    ("edges", "comp", False, "shuffle", 2, 4, 9, 3),
    ("edges", "eight", False, "group", 4, 5, 33, FULL),
    ("edges", "nine", True, "shuffle", 1, 16, 33, "mix"),
    ("edges", "perq", False, "shuffle", 2, 17, 33, 3),
    ("edges", "same", False, "shuffle", 4, 64, 33, "mix"),
    ("edges", "none", True, "group", 1, 64, 33, "mix"),
    ("edges", "comp", True, "group", 2, 16, 33, "most1"),
    ("skew", "same", False, "group", 1, 4, 1, FULL),
    ("skew", "comp", False, "shuffle", 4, 64, 33, FULL),
    ("skew", "nine_seedless", False, "shuffle", 2, 64, 33, "mix"),
    ("skew", "eight", True, "group", 1, 5, 9, "mix"),
    ("skew", "one", False, "group", 4, 17, 9, 3),
    ("skew", "perq", True, "shuffle", 2, 16, 33, "mix"),
    ("skew", "nine_seedless", False, "group", 4, 1, 33, 1),
    ("skew", "none", True, "group", 1, 64, 9, "most1"),
    ("dups", "one", True, "group", 2, 64, 33, 3),
    ("dups", "comp", False, "shuffle", 1, 17, 33, "mix"),
    ("dups", "eight", False, "shuffle", 4, 16, 33, "mix"),
    ("dups", "nine", False, "group", 2, 5, 9, FULL),
    ("dups", "perq", True, "shuffle", 1, 4, 33, 1),
    ("dups", "same", False, "group", 4, 1, 1, 1),
    ("dups", "perq", False, "shuffle", 4, 64, 9, "most1"),
]


def build(c, table, holes, order, splits, nq, probes):
    """-> (names of the table's masks, mask_of int32 [nq], nprobes int32 [nq]) of one case over corpus c."""
    names = table_names(table, nq)
    return names, mask_of(len(names), nq, holes, order), probe_counts(probes, nq, c.nlist)


def selections(c, names, mo, splits, nq):
    """One bool [n] per question from the table's names and mask_of (-1: all ones)."""
    lab = c.quantized()[2]
    memo = {n: selection(n, lab, splits, nq) for n in set(names)}
    ones = np.ones(len(lab), dtype=bool)
    return [ones if m < 0 else memo[names[m]] for m in mo]
