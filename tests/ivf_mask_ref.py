"""Reference and cases of the metadata-filtered IVF search (rfx_ivf_search_masked).  TEST
INFRASTRUCTURE ONLY (tests/test_ivf_masked_ref.py on the CPU, tests/test_gpu_ivf_masked.py on the GPU); numpy,
oracle/ivf.py unchanged and the corpora of tests/hostile_ivf.py.

The reference: oracle.ivf.search called with the labels of the unselected rows replaced by -1.  No probe id is
-1, so those rows fall out BEFORE the ranking and the probes are the unfiltered search's (the oracle computes
them from the centroids alone).  The two mutants are what a wrong kernel would compute: the mask ignored, and
the mask applied to a finished top-k (too few rows come back).  CASES is the GPU file's grid; the CPU file
shows that both mutants differ from the reference on every one of them but the all-ones and all-zero masks.
"""
import numpy as np

from oracle import ivf as oivf

FULL = 0  # nprobe: every list (capped at 64), as tests/test_gpu_ivf_hostile.py


# ---- the reference and its mutants ---------------------------------------------------------------------------
def search(qq, qinv, codes, inv, labels, qc, fc, nprobe, k, sel):
    """oracle.ivf.search over the rows sel (bool [n]) selects: (scores f32 [nq][k], rows i64 [nq][k])."""
    lab = np.where(sel, labels, -1)
    return oivf.search(qq, qinv, codes, inv, lab, qc, fc, nprobe, k)


def mutant_ignored(qq, qinv, codes, inv, labels, qc, fc, nprobe, k, sel):
    return oivf.search(qq, qinv, codes, inv, labels, qc, fc, nprobe, k)


def mutant_after_topk(qq, qinv, codes, inv, labels, qc, fc, nprobe, k, sel):
    """The unmasked top-k with its unselected rows struck out, the survivors moved up, padding behind."""
    s, r = oivf.search(qq, qinv, codes, inv, labels, qc, fc, nprobe, k)
    out_s = np.full_like(s, -np.inf)
    out_r = np.full_like(r, -1)
    for i in range(len(r)):
        keep = (r[i] >= 0) & sel[np.maximum(r[i], 0)]
        out_s[i, :keep.sum()] = s[i][keep]
        out_r[i, :keep.sum()] = r[i][keep]
    return out_s, out_r


def brute_force(qq, qinv, codes, inv, labels, qc, fc, nprobe, k, sel):
    """The definition, written out: score every row of the probed lists, drop the unselected, then rank."""
    pr = oivf.probes(qq, qc, fc, nprobe)
    nq = qq.shape[0]
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    out_r = np.full((nq, k), -1, dtype=np.int64)
    for i in range(nq):
        rows = [r for r in range(len(labels)) if labels[r] in pr[i]]
        dots = codes[rows].astype(np.int64) @ qq[i].astype(np.int64)  # exact
        scored = [(np.float32(d) * (inv[r] * qinv[i]), r) for d, r in zip(dots, rows)]  # f32 * (f32 * f32)
        kept = [(s, r) for s, r in scored if sel[r]]
        kept.sort(key=lambda t: (-float(t[0]), t[1]))  # (-0.0 and +0.0 compare equal: the row decides)
        for j, (s, r) in enumerate(kept[:k]):
            out_s[i, j], out_r[i, j] = s, r
    return out_s, out_r


# ---- mask builders: bool [n] over insertion-order row ids -----------------------------------------------------
def list_positions(labels):
    """Position of every row inside its posting list (lists hold their rows by ascending row id)."""
    pos = np.empty(len(labels), dtype=np.int64)
    for c in np.unique(labels):
        m = np.flatnonzero(labels == c)
        pos[m] = np.arange(len(m))
    return pos


def file_ranges(n):
    """Contiguous (first, count) ranges as a file filter makes them: files of uneven length, every other one
    selected, none starting on a word edge but the first."""
    bounds = [0]
    step = 37
    while bounds[-1] + step < n:
        bounds.append(bounds[-1] + step)
        step = step * 2 + 5 if step < n // 6 else 211
    bounds.append(n)
    return [(bounds[i], bounds[i + 1] - bounds[i]) for i in range(0, len(bounds) - 1, 2)]


def selection(name, labels, splits=1):
    """The named mask over a corpus with these list labels."""
    n = len(labels)
    r = np.arange(n)
    if name == "ones":
        return np.ones(n, dtype=bool)
    if name == "zeros":
        return np.zeros(n, dtype=bool)
    if name == "alt":
        return r % 2 == 1
    if name == "wordedge":  # only the first and the last bit of every mask word
        return (r % 32 == 31) | (r % 32 == 0)
    pos = list_positions(labels)
    if name == "first":
        return pos == 0
    if name == "last":
        return pos == np.bincount(labels)[labels] - 1
    if name == "ranges":
        from rfx import filters
        words = filters.row_mask_words(n, file_ranges(n))
        return from_words(words, n)
    if name == "seedless":
        # list_scan_kernel: wave w of block (L, split) scores the 64-row chunks (split * 4 + w) + 4 * splits * j
        # of list L and keeps its first two (j = 0, 1) for seed_lists.  Clearing list positions below
        # 2 * 256 * splits of the longest list clears exactly those chunks of every wave: seed_lists sees
        # nothing but NaN and the list is filled by offer() alone.
        long_list = np.argmax(np.bincount(labels))
        return ~((labels == long_list) & (pos < 512 * splits))
    if name == "few":  # three rows in all: fewer than k eligible whatever the probes, for every k > 3
        sel = np.zeros(n, dtype=bool)
        big = np.argsort(-np.bincount(labels), kind="stable")[:3]
        for c in big:
            m = np.flatnonzero(labels == c)
            sel[m[len(m) // 2]] = True
        return sel
    raise ValueError(name)


def to_words(sel, spare=True):
    """bool [n] -> int32 mask words (bit r & 31 of word r >> 5); spare: the bits past row n - 1 of the last
    word SET — the kernel never consults them (every row id it holds is below n)."""
    n = len(sel)
    bits = np.zeros((n + 31) // 32 * 32, dtype=np.uint8)
    bits[:n] = sel
    if spare:
        bits[n:] = 1
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)


def from_words(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


# ---- the GPU file's grid: (corpus, mask, splits, k, nq, nprobe) ----------------------------------------------
# Every corpus sees every value of splits {1, 2, 4}, k {1, 4, 5, 16, 17, 64}, nq {1, 9, 33} and nprobe {1, 3,
# FULL} at least once (test_search_cases_cover_every_value), thinned as tests/test_gpu_ivf_hostile.py thins its
# grid; which mask takes which point is chosen so that both mutants differ on it (tests/test_ivf_masked_ref.py).
G = {"a": (1, 1, 1, 1), "b": (2, 4, 9, 3), "c": (4, 5, 33, FULL), "d": (1, 16, 33, 3), "e": (2, 17, 1, FULL),
     "f": (4, 64, 9, 1), "g": (1, 64, 33, 3), "h": (4, 64, 33, 3), "i": (2, 16, 33, FULL), "j": (4, 17, 33, 1),
     "k": (1, 64, 33, FULL), "l": (2, 64, 33, 1)}
PLAN = {
    "edges": {"ones": "ac", "zeros": "bf", "alt": "cd", "wordedge": "be", "first": "fk", "last": "gd",
              "ranges": "ce", "few": "ab"},
    "skew": {"ones": "ae", "zeros": "cf", "alt": "bd", "wordedge": "ce", "first": "fg", "last": "dk",
             "ranges": "bc", "few": "af", "seedless": "ghil"},
    "dups": {"ones": "af", "zeros": "de", "alt": "hg", "wordedge": "ci", "first": "bf", "last": "ek",
             "ranges": "hd", "few": "ac"},
}
CASES = [(corpus, mask) + G[g] for corpus, masks in PLAN.items() for mask, gs in masks.items() for g in gs]
