"""numpy float64 reference of the lexical index's rules: the statistics over live rows, the BM25
score and its top-k with the tie order, reciprocal-rank fusion; and the counter-based CSR generator of the GPU
tests.  Plain Python / numpy on purpose: every operation is an IEEE f64 operation rounded on its own."""
import math

import numpy as np

M64 = (1 << 64) - 1


def splitmix64(x):
    """splitmix64 of a uint64 array (oracle/synth.py's generator step)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _unit(h):
    """(0, 1) from the top 24 bits"""
    return ((h >> np.uint64(40)).astype(np.float64) + 0.5) / float(1 << 24)


def gen_csr(seed, n, V=4096, row0=0, max_len=400, skew=2.5, lengths=None):
    """Counter-based Zipf-like CSR of rows row0 .. row0 + n - 1: a row draws 0 .. max_len - 1 buckets (short rows
    likelier; `lengths` fixes the draws per row), bucket = floor(V * u ** skew), repeated buckets merged, tf 1..9,
    a hash sign on the count.  Returns (indptr int32, bucket int32, count int16), buckets sorted within a row."""
    r = np.arange(row0, row0 + n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        base = splitmix64(np.uint64(seed) * np.uint64(0x100000001B3) + r)
    if lengths is None:
        draws = np.floor(max_len * _unit(splitmix64(base)) ** 2).astype(np.int64)
    else:
        draws = np.broadcast_to(np.asarray(lengths, dtype=np.int64), (n,)).copy()
    rows = np.repeat(np.arange(n, dtype=np.int64), draws)
    j = np.arange(rows.size, dtype=np.int64) - np.repeat(np.cumsum(draws) - draws, draws)
    with np.errstate(over="ignore"):
        key = splitmix64(base[rows] + (j.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15))
    bucket = np.minimum(np.floor(V * _unit(key) ** skew).astype(np.int64), V - 1)
    tf = 1 + ((key & np.uint64(0xFFFF)) % np.uint64(9)).astype(np.int64)
    sign = np.where((key >> np.uint64(16)) & np.uint64(1), -1, 1)
    order = np.lexsort((j, bucket, rows))
    rows, bucket, cnt = rows[order], bucket[order], (tf * sign)[order]
    first = np.ones(rows.size, dtype=bool)
    first[1:] = (rows[1:] != rows[:-1]) | (bucket[1:] != bucket[:-1])
    rows, bucket, cnt = rows[first], bucket[first], cnt[first]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, rows + 1, 1)
    return np.cumsum(indptr).astype(np.int32), bucket.astype(np.int32), cnt.astype(np.int16)


def exact_rows(seed, sizes, V=4096):
    """Rows with exactly sizes[i] distinct buckets each (tf 1..9)."""
    ip, bk, ct = [0], [], []
    for i, sz in enumerate(sizes):
        h = splitmix64(np.uint64(seed + 7919 * i) + np.arange(4 * sz + 8, dtype=np.uint64))
        b = np.unique((h % np.uint64(V)).astype(np.int64))[:sz]
        assert b.size == sz
        bk.append(b)
        ct.append(1 + (np.arange(sz) * 5 + i) % 9)
        ip.append(ip[-1] + sz)
    return (np.asarray(ip, np.int32), np.concatenate(bk).astype(np.int32) if bk else np.zeros(0, np.int32),
            np.concatenate(ct).astype(np.int16) if ct else np.zeros(0, np.int16))


def concat_csr(parts):
    ip, bk, ct = [np.zeros(1, np.int64)], [], []
    base = 0
    for p_ip, p_bk, p_ct in parts:
        p_ip = np.asarray(p_ip, np.int64)
        ip.append(p_ip[1:] - p_ip[0] + base)
        bk.append(np.asarray(p_bk)[p_ip[0]:p_ip[-1]])
        ct.append(np.asarray(p_ct)[p_ip[0]:p_ip[-1]])
        base += int(p_ip[-1] - p_ip[0])
    return np.concatenate(ip).astype(np.int32), np.concatenate(bk).astype(np.int32), np.concatenate(ct).astype(np.int16)


def drop_buckets(csr, buckets):
    """the CSR without the entries of the given buckets"""
    ip, bk, ct = csr
    ip = np.asarray(ip, np.int64)
    keep = ~np.isin(bk, buckets)
    rows = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    nip = np.zeros(ip.size, np.int64)
    np.add.at(nip, rows[keep] + 1, 1)
    return np.cumsum(nip).astype(np.int32), np.asarray(bk)[keep], np.asarray(ct)[keep]


def slice_csr(csr, lo, hi):
    ip, bk, ct = csr
    return concat_csr([(ip[lo:hi + 1], bk, ct)])


# ---- the corpus and the question sets of tests/test_gpu_lex.py (shared with the CPU pre-check of the near-tie
# allowance in tests/test_lex_host.py, so both see exactly the same data) ---------------------------------------
GPU_ROWS = 20000  # no multiple of a workgroup's 512 rows, nor of a wave's 32-row tile
GPU_V = 4096
GPU_ABSENT = (4090, 4091)  # buckets no row of the corpus holds
GPU_SPECIAL_AT = (0, 29, 509, GPU_ROWS - 6)


def gpu_corpus():
    """20,000 rows: the generator's, with rows of 0, 1, 63, 64, 65 and 300 entries at the start, around a tile
    boundary (rows 29..34), around a workgroup's boundary (rows 509..514) and at the end"""
    sp = exact_rows(5, [0, 1, 63, 64, 65, 300], GPU_V)
    assert not np.isin(sp[1], GPU_ABSENT).any()
    gen = drop_buckets(gen_csr(101, GPU_ROWS), GPU_ABSENT)
    parts, at = [], 0
    for pos in GPU_SPECIAL_AT:
        parts.append(slice_csr(gen, at, pos))
        parts.append(sp)
        at = pos + 6
    parts.append(slice_csr(gen, at, GPU_ROWS))
    csr = concat_csr(parts)
    assert csr[0].size - 1 == GPU_ROWS
    return csr


def gpu_special_questions(csr):
    """questions aimed at the special rows: one made of each special row's own buckets"""
    ip, bk, _ = csr
    qs = []
    for row in (1, 2, 3, 4, 5, 30, 33, 34, 510, 514, GPU_ROWS - 5, GPU_ROWS - 1):
        b = bk[ip[row]:ip[row + 1]][:12]
        qs.append((b, np.ones(b.size, np.int64)))
    return qs


def gpu_mask_words():
    """a row mask with sparse, empty and full words; (words uint32, allowed bool [rows])"""
    words = (GPU_ROWS + 31) // 32
    h = splitmix64(np.arange(words, dtype=np.uint64) + np.uint64(77))
    m = (h & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    m &= (splitmix64(h) & np.uint64(0xFFFFFFFF)).astype(np.uint32)  # sparse words
    m[::3] = 0
    m[1::7] = 0xFFFFFFFF
    m[0], m[words - 1] = 0x80000001, 0xFFFFFFFF
    r = np.arange(GPU_ROWS)
    return m, ((m[r >> 5] >> (r & 31).astype(np.uint32)) & 1).astype(bool)


def gpu_question_sets(csr):
    """name -> (questions, k values, (k1, b) pairs, masked): every set tests/test_gpu_lex.py compares on the
    20,000-row corpus"""
    special = gpu_special_questions(csr)
    return {"scan": (special + gen_questions(7, 21), (1, 10, 64), ((1.2, 0.75),), False),
            "batch": (gen_questions(7, 33), (64,), ((1.2, 0.75),), False),
            "parameters": (gen_questions(9, 9), (10,), ((0.0, 0.75), (2.0, 0.0), (0.9, 1.0)), False),
            "mask": (gen_questions(7, 9) + special[:3], (10,), ((1.2, 0.75),), True)}


class RefIndex:
    """The rules' state: entries (row, bucket, tf) with tf = |count|, zero counts dropped; len_r = sum of tf; the
    statistics over live rows."""

    def __init__(self, V=4096):
        self.V = V
        self.rows = 0
        self.e_row = np.zeros(0, np.int64)
        self.e_bucket = np.zeros(0, np.int64)
        self.e_tf = np.zeros(0, np.int64)
        self.len = np.zeros(0, np.int64)
        self.dead = np.zeros(0, bool)

    def add(self, indptr, bucket, count):
        indptr = np.asarray(indptr, np.int64)
        n = indptr.size - 1
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr)) + self.rows
        tf = np.minimum(np.abs(np.asarray(count, np.int64)[indptr[0]:indptr[-1]]), 65535)
        bk = np.asarray(bucket, np.int64)[indptr[0]:indptr[-1]]
        keep = tf > 0
        self.e_row = np.concatenate([self.e_row, rows[keep]])
        self.e_bucket = np.concatenate([self.e_bucket, bk[keep]])
        self.e_tf = np.concatenate([self.e_tf, tf[keep]])
        ln = np.zeros(n, np.int64)
        np.add.at(ln, rows[keep] - self.rows, tf[keep])
        self.len = np.concatenate([self.len, ln])
        self.dead = np.concatenate([self.dead, np.zeros(n, bool)])
        self.rows += n

    def tombstone(self, rows):
        self.dead[np.asarray(rows, np.int64)] = True

    def stats(self):
        """(N, df [V], total_len) over live rows, exact integers"""
        live_e = ~self.dead[self.e_row]
        df = np.bincount(self.e_bucket[live_e], minlength=self.V).astype(np.int64)
        return int((~self.dead).sum()), df, int(self.len[~self.dead].sum())

    def fresh(self):
        """a new RefIndex over the live rows only (renumbered), and the old row of each new row"""
        old = np.nonzero(~self.dead)[0]
        new_of = -np.ones(self.rows, np.int64)
        new_of[old] = np.arange(old.size)
        keep = ~self.dead[self.e_row]
        f = RefIndex(self.V)
        f.rows = old.size
        f.e_row, f.e_bucket, f.e_tf = new_of[self.e_row[keep]], self.e_bucket[keep], self.e_tf[keep]
        f.len = self.len[old]
        f.dead = np.zeros(old.size, bool)
        return f, old

    def weights(self, q_bucket, q_count):
        """w [V] f32: fl32(idf_t * qtf_t), qtf = |count| summed over a repeated bucket"""
        N, df, _ = self.stats()
        qtf = np.zeros(self.V, np.int64)
        np.add.at(qtf, np.asarray(q_bucket, np.int64), np.abs(np.asarray(q_count, np.int64)))
        w = np.zeros(self.V, np.float32)
        for t in np.nonzero(qtf)[0]:
            idf = math.log(1.0 + (float(N - int(df[t])) + 0.5) / (float(int(df[t])) + 0.5))
            w[t] = np.float32(idf * float(int(qtf[t])))
        return w

    def scores(self, q_bucket, q_count, k1=1.2, b=0.75, allowed=None):
        """(score f32 [rows], ranks bool [rows]): the BM25 score of every row that may rank"""
        k1, b = float(np.float32(k1)), float(np.float32(b))
        N, _, total = self.stats()
        w = self.weights(q_bucket, q_count).astype(np.float64)
        ok = ~self.dead if allowed is None else (~self.dead & np.asarray(allowed, bool)[:self.rows])
        sel = (w[self.e_bucket] != 0.0) & ok[self.e_row]
        er, eb, et = self.e_row[sel], self.e_bucket[sel], self.e_tf[sel].astype(np.float64)
        acc = np.zeros(self.rows, np.float64)
        if er.size:
            avgdl = float(total) / float(N)
            B = k1 * ((1.0 - b) + b * (self.len.astype(np.float64) / avgdl))
            term = (w[eb] * (et * (k1 + 1.0))) / (et + B[er])
            np.add.at(acc, er, term)
        ranks = np.zeros(self.rows, bool)
        ranks[er] = True
        return acc.astype(np.float32), ranks

    def topk(self, q_bucket, q_count, k, k1=1.2, b=0.75, allowed=None):
        """(scores f32 [k], rows int64 [k], close): score desc, row asc, padded (-inf, -1).  close: two of the
        positions 1..k+1 hold different scores within one f32 ulp of each other (their order may legitimately
        differ on the device)."""
        s, ranks = self.scores(q_bucket, q_count, k1, b, allowed)
        cand = np.nonzero(ranks)[0]
        order = cand[np.lexsort((cand, -s[cand].astype(np.float64)))][:k + 1]
        top = s[order]
        close = bool(np.any((top[:-1] != top[1:]) & (np.nextafter(top[1:], np.float32(np.inf)) >= top[:-1])))
        out_s = np.full(k, -np.inf, np.float32)
        out_r = np.full(k, -1, np.int64)
        n = min(k, order.size)
        out_s[:n], out_r[:n] = top[:n], order[:n]
        return out_s, out_r, close


def question_csr(questions):
    """[(buckets, counts), ...] -> CSR"""
    ip = np.zeros(len(questions) + 1, np.int32)
    ip[1:] = np.cumsum([len(q[0]) for q in questions])
    bk = np.concatenate([np.asarray(q[0], np.int32) for q in questions]) if questions else np.zeros(0, np.int32)
    ct = np.concatenate([np.asarray(q[1], np.int16) for q in questions]) if questions else np.zeros(0, np.int16)
    return ip, bk, ct


def gen_questions(seed, nq, V=4096, terms=(1, 12)):
    """nq questions of terms[0]..terms[1] Zipf-like buckets, counts in +-1..3"""
    qs = []
    for q in range(nq):
        h = splitmix64(np.uint64(seed * 1000003 + q) + np.arange(64, dtype=np.uint64))
        n = terms[0] + int(h[0] % np.uint64(terms[1] - terms[0] + 1))
        b = np.unique(np.minimum(np.floor(V * _unit(h[1:1 + n]) ** 2.5).astype(np.int64), V - 1))
        c = 1 + (h[32:32 + b.size] % np.uint64(3)).astype(np.int64)
        c = np.where((h[32:32 + b.size] >> np.uint64(8)) & np.uint64(1), -c, c)
        qs.append((b, c))
    return qs


def compare_topk(got_s, got_r, ref: RefIndex, questions, k, k1=1.2, b=0.75, allowed=None):
    """The comparison rule of the GPU tests.  Scores: equal to the reference's or an adjacent f32.  Rows:
    identical, except that a question whose reference scores hold two near neighbours (RefIndex.topk's `close`)
    is left out of the row comparison.  Returns the number of questions left out."""
    skipped = 0
    for qi, (qb, qc) in enumerate(questions):
        rs, rr, close = ref.topk(qb, qc, k, k1, b, allowed)
        gs, gr = np.asarray(got_s[qi]), np.asarray(got_r[qi])
        n = int((rr >= 0).sum())
        assert int((gr >= 0).sum()) == n, (qi, gr, rr)
        assert np.all(gr[n:] == -1) and np.all(np.isneginf(gs[n:])), (qi, gs, gr)
        if close:
            skipped += 1
            # the scores still match position by position
            lo, hi = np.nextafter(rs[:n], np.float32(-np.inf)), np.nextafter(rs[:n], np.float32(np.inf))
            assert np.all((gs[:n] >= lo) & (gs[:n] <= hi)), (qi, gs, rs)
            continue
        assert np.array_equal(gr, rr), (qi, gr, rr, gs, rs)
        lo, hi = np.nextafter(rs[:n], np.float32(-np.inf)), np.nextafter(rs[:n], np.float32(np.inf))
        assert np.all((gs[:n] >= lo) & (gs[:n] <= hi)), (qi, gs, rs)
        assert np.all(gs[:n] > 0)
    return skipped


# ---- reciprocal-rank fusion ------------------------------------------------------------------------------
def rrf(dense, lex, k, alpha, rrf_c=60):
    """One question: dense / lex = row lists in search order (row < 0 = padding).  Returns (scores f32 [k], rows
    int64 [k], ranks int32 [k][2]); f = A / (c + rank_d) + (1 - A) / (c + rank_l) in f64, absent = 0.0; order
    f desc, row asc; padding (-inf, -1, 0, 0)."""
    A = float(np.float32(alpha))
    c = float(int(rrf_c))

    def ranks(lst):
        out, n = {}, 0
        for r in lst:
            r = int(r)
            if r < 0:
                continue
            n += 1
            out.setdefault(r, n)
        return out

    rd, rl = ranks(dense), ranks(lex)
    items = []
    for row in set(rd) | set(rl):
        d, l = rd.get(row, 0), rl.get(row, 0)
        fd = A / (c + float(d)) if d else 0.0
        fl = (1.0 - A) / (c + float(l)) if l else 0.0
        items.append((-(fd + fl), row, d, l))
    items.sort()
    out_s = np.full(k, -np.inf, np.float32)
    out_r = np.full(k, -1, np.int64)
    out_k = np.zeros((k, 2), np.int32)
    for i, (nf, row, d, l) in enumerate(items[:k]):
        out_s[i], out_r[i], out_k[i] = np.float32(-nf), row, (d, l)
    return out_s, out_r, out_k


def rrf_batch(dense, lex, k, alpha, n_dense=None, n_lex=None, rrf_c=60):
    dense, lex = np.asarray(dense), np.asarray(lex)
    nq = dense.shape[0]
    alpha = np.broadcast_to(np.asarray(alpha, np.float32), (nq,))
    nd = np.broadcast_to(dense.shape[1] if n_dense is None else np.asarray(n_dense), (nq,))
    nl = np.broadcast_to(lex.shape[1] if n_lex is None else np.asarray(n_lex), (nq,))
    res = [rrf(dense[q, :nd[q]], lex[q, :nl[q]], k, alpha[q], rrf_c) for q in range(nq)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res])
