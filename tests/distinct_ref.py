"""CPU reference of the distinct-document rule, the corpora built to break an implementation
of it, and numpy stand-ins for the device operations of its rounds.

The rule: take the full ranking of the live rows the filter selects (score = fl32 of the f64 dot; score desc,
row asc); keep a row if no earlier row of the ranking belongs to the same file; the answer is the first k kept
rows, then padding (-inf, -1).

Every corpus value is a multiple of 1/64 in [-1, 1]: exact in f32, bf16 and f16, and every dot of up to 1024
of them is exact in f32 as well, so equal rows tie exactly and no answer hangs on a rounding."""
import numpy as np

from oracle import search as osearch

NQ = 5


# ---- the rule -------------------------------------------------------------------------------------------
def ranking(q64, x64, allowed=None):
    """Per query the full ranking of the live (non-NaN), allowed rows: [(scores f32, rows int64)], from the
    oracle's exact top-n at n = all rows, ordered by the rule (fl32 score desc, row asc)."""
    x = np.array(x64, dtype=np.float64)
    if allowed is not None:
        x[~np.asarray(allowed, dtype=bool)] = np.nan
    s, r = osearch.topk(q64, x, len(x))
    out = []
    for i in range(len(s)):
        live = r[i] >= 0
        s32, rr = s[i][live].astype(np.float32), r[i][live]
        o = np.lexsort((rr, -s32))
        out.append((s32[o], rr[o]))
    return out


def reference(q64, x64, row_doc, k, allowed=None):
    """(scores f32 [nq][k], rows int64 [nq][k], docs int32 [nq][k]) of the rule."""
    nq = len(q64)
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    out_r = np.full((nq, k), -1, dtype=np.int64)
    out_d = np.full((nq, k), -1, dtype=np.int32)
    for i, (s, r) in enumerate(ranking(q64, x64, allowed)):
        seen, n = set(), 0
        for sc, row in zip(s, r):
            d = int(row_doc[row])
            if d < 0 or d in seen:
                continue
            seen.add(d)
            out_s[i, n], out_r[i, n], out_d[i, n] = sc, row, d
            n += 1
            if n == k:
                break
    return out_s, out_r, out_d


def collapse(cand_s, cand_r, row_doc, rows, k, have=None, out=None):
    """rfx_distinct_collapse in numpy: (scores, rows, docs [nq][k], n [nq], done [nq]); `out` (the 5-tuple of
    the round before) is appended to in place when given, its slots below have[q] left as they are."""
    cand_s, cand_r = np.asarray(cand_s, dtype=np.float32), np.asarray(cand_r, dtype=np.int64)
    nq, n_cand = cand_s.shape
    if out is None:
        out = (np.zeros((nq, k), np.float32), np.zeros((nq, k), np.int64), np.zeros((nq, k), np.int32),
               np.zeros(nq, np.int32), np.zeros(nq, np.int32))
    o_s, o_r, o_d, o_n, o_done = out
    have = np.zeros(nq, np.int32) if have is None else np.array(have, dtype=np.int32)
    for q in range(nq):
        h = int(min(max(have[q], 0), k))
        seen = set(int(d) for d in o_d[q, :h])
        n, valid = h, 0
        for s, r in zip(cand_s[q], cand_r[q]):
            if not 0 <= r < rows:
                continue
            valid += 1
            d = int(row_doc[r])
            if d < 0 or d in seen:
                continue
            seen.add(d)
            if n < k:
                o_s[q, n], o_r[q, n], o_d[q, n] = s, r, d
                n += 1
        o_s[q, n:], o_r[q, n:], o_d[q, n:] = -np.inf, -1, -1
        o_n[q] = n
        o_done[q] = int(n >= k or valid < n_cand)
    return out


# ---- corpora ----------------------------------------------------------------------------------------------
def _grid(rng, n, d):
    return rng.integers(-64, 65, size=(n, d)).astype(np.float32) / 64.0


def _near(rng, base, n, changed):
    """n copies of `base`, each with `changed` coordinates redrawn from the grid."""
    x = np.repeat(base[None, :], n, axis=0).copy()
    for row in x:
        at = rng.choice(len(base), size=changed, replace=False)
        row[at] = rng.integers(-64, 65, size=changed).astype(np.float32) / 64.0
    return x


class Corpus:
    """rows f32 [n][d]; files [(first, n, deleted)] in ordinal order; queries f32 [nq][d]; k; fetch_k; the
    rounds an exact implementation takes on it (`rounds`)."""

    def __init__(self, name, d, pieces, queries, k, rounds, deleted=(), fetch_k=None):
        self.name, self.d, self.k, self.rounds, self.fetch_k = name, d, k, rounds, fetch_k
        self.rows = np.concatenate(pieces).astype(np.float32)
        self.files, first = [], 0
        for i, p in enumerate(pieces):
            self.files.append((first, len(p), i in deleted))
            first += len(p)
        self.queries = np.asarray(queries, dtype=np.float32)
        self.row_doc = np.full(len(self.rows), -1, dtype=np.int32)
        for o, (f0, n, dead) in enumerate(self.files):
            if not dead:
                self.row_doc[f0:f0 + n] = o
        self.doc_ranges = np.array([(f0, n) for f0, n, _ in self.files], dtype=np.int64)
        self.dead_rows = np.flatnonzero(np.concatenate([np.full(n, dead) for _, n, dead in self.files]))

    @property
    def x64(self):
        x = self.rows.astype(np.float64)
        x[self.dead_rows] = np.nan  # a deleted file's rows are tombstoned
        return x

    @property
    def q64(self):
        return self.queries.astype(np.float64)

    def files_in_best(self, n, allowed=None):
        """Per query: how many files the best n rows of the ranking hold."""
        return [len(set(self.row_doc[r[:n]].tolist())) for _, r in ranking(self.q64, self.x64, allowed)]


def build(name, d, seed=0):
    rng = np.random.default_rng(1000 + seed)
    base = np.where(rng.integers(0, 2, d) > 0, 1.0, -1.0).astype(np.float32)  # base . base = d
    queries = _near(rng, base, NQ, 2)
    small = lambda n_files, lo, hi: [_grid(rng, int(rng.integers(lo, hi + 1)), d) for _ in range(n_files)]
    if name == "plain":  # 60 files of 1-40 chunks; the first search suffices
        return Corpus(name, d, small(60, 1, 40), _grid(rng, NQ, d), 10, 1)
    if name == "dominant":  # one file owns the best 200 rows of every question: one completion round
        return Corpus(name, d, small(3, 1, 5) + [_near(rng, base, 200, 2)] + small(3, 1, 5), queries, 5, 2)
    if name == "dominant2":  # two such files in a row: two completion rounds
        second = _near(rng, base, 200, 2)
        second[:, :d // 4] = 0.0  # every row of it scores below every row of the first
        return Corpus(name, d, small(3, 1, 5) + [_near(rng, base, 200, 2), second] + small(3, 1, 5), queries, 5, 3)
    if name == "dups":
        # identical rows in different files: Z holds one copy of `base` BEFORE the 64 copies of file A, so the best
        # 64 rows are Z's copy and 63 of A's; C (two copies: the lower row is its hit) and D (one) follow
        # across the rank-64 edge, equal in score to everything before them
        z, c = _grid(rng, 3, d), _grid(rng, 3, d)
        z[1], c[0], c[2] = base, base, base
        return Corpus(name, d, [z, np.repeat(base[None, :], 64, axis=0), c, base[None, :].copy()] + small(5, 1, 4),
                      queries, 5, 2, fetch_k=64)
    if name == "few":  # 3 files at k 10, fewer rows than fetch_k: padding after one round
        return Corpus(name, d, small(3, 4, 7), _grid(rng, NQ, d), 10, 1)
    if name == "few_big":  # 3 files at k 10 with more rows than fetch_k: nothing is left after round 1
        return Corpus(name, d, small(3, 30, 40), _grid(rng, NQ, d), 10, 1)
    if name == "holes":  # deleted files in the middle and at both ends; the deleted ones hold the best rows
        pieces = small(20, 1, 30)
        deleted = (0, 7, 8, 19)
        for i in deleted:
            pieces[i] = _near(rng, base, len(pieces[i]), 2)
        return Corpus(name, d, pieces, queries, 10, 1, deleted=deleted)
    raise ValueError(name)


CORPORA = ("plain", "dominant", "dominant2", "dups", "few", "few_big", "holes")


# ---- numpy stand-ins for the device operations of rfx.distinct.run_rounds --------------------------------------
def np_search(q64, x64, n, allowed=None):
    """The plain search at k = n in numpy: (scores f32 [nq][n], rows int64 [nq][n]), padded (-inf, -1)."""
    s = np.full((len(q64), n), -np.inf, dtype=np.float32)
    r = np.full((len(q64), n), -1, dtype=np.int64)
    for i, (rs, rr) in enumerate(ranking(q64, x64, allowed)):
        m = min(n, len(rr))
        s[i, :m], r[i, :m] = rs[:m], rr[:m]
    return s, r


def _allowed(n_rows, ranges):
    a = np.zeros(n_rows, dtype=bool)
    for first, count in ranges:
        a[first:first + count] = True
    return a


class NumpyOps:
    """run_rounds' operations over a Corpus; `refuse_segmented` makes segmented() refuse the shape."""

    def __init__(self, c, k, fetch_k, allowed=None, refuse_segmented=False):
        self.c, self.k, self.fetch_k, self.allowed, self.refuse = c, k, fetch_k, allowed, refuse_segmented
        self.out = None
        self.calls = []

    def first(self):
        self.calls.append("first")
        return np_search(self.c.q64, self.c.x64, self.fetch_k, self.allowed)

    def collapse(self, cand, have):
        self.out = collapse(cand[0], cand[1], self.c.row_doc, len(self.c.rows), self.k,
                            self.out[3] if have else None, self.out if have else None)

    def read(self):
        return self.out[3].copy(), self.out[4].copy(), self.out[2].copy()

    def _complete(self, open_q, ranges):
        nq = len(self.c.queries)
        s = np.full((nq, 64), -np.inf, dtype=np.float32)
        r = np.full((nq, 64), -1, dtype=np.int64)
        for q, rg in zip(open_q, ranges):
            s[q], r[q] = (a[0] for a in np_search(self.c.q64[q:q + 1], self.c.x64, 64, _allowed(len(self.c.rows), rg)))
        return s, r

    def segmented(self, open_q, ranges):
        from rfx import distinct
        if self.refuse:
            raise distinct.SegmentedUnsupported("refused")
        self.calls.append(("segmented", tuple(open_q)))
        return self._complete(open_q, ranges)

    def masked(self, open_q, ranges):
        self.calls.append(("masked", tuple(open_q)))
        return self._complete(open_q, ranges)


# ---- mutants ------------------------------------------------------------------------------------------------
def mutant_first64(c, k):
    """The collapse of the first 64 rows only, no completion."""
    s, r = np_search(c.q64, c.x64, 64)
    return collapse(s, r, c.row_doc, len(c.rows), k)[:3]


def mutant_ignores_ties(c, k):
    """Every file's best chunk by score alone: among equal scores it takes whichever comes last."""
    nq = len(c.queries)
    out_r = np.full((nq, k), -1, dtype=np.int64)
    for i, (s, r) in enumerate(ranking(c.q64, c.x64)):
        best = {}
        for sc, row in zip(s, r):
            d = int(c.row_doc[row])
            if d >= 0 and (d not in best or sc >= best[d][0]):
                best[d] = (sc, row)
        picks = sorted(best.values(), key=lambda p: (-p[0], -p[1]))[:k]
        out_r[i, :len(picks)] = [p[1] for p in picks]
    return out_r
