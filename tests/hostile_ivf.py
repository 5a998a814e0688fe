"""Hostile corpora for the IVF-Flat int8 path: what synth_clustered's unit-norm, repeat-free rows
never show it — equal scores, both zeros, row scales 2^200 apart, planted list lengths.  TEST INFRASTRUCTURE
ONLY (tests/test_ivf_hostile_oracle.py on the CPU, tests/test_gpu_ivf_hostile.py on the GPU); numpy and a
seeded default_rng, nothing else.  Every builder returns stored values (exactly representable in `dtype`,
hostile.stored) and asserts what it plants against oracle/ivf.py alone.

  planted        exact list sizes without k-means: centroid c is the int8 one-hot 127 e_c (set_centroids), a row
                 of list c is e_c + 0.05 g (g a unit gaussian vector; + common e_{d-1} where asked), rows shuffled.
  edges          d 256, 24 lists of 0, 1, 63 .. 65, 127 .. 129, 255 .. 257, 511 .. 513, 1023 .. 1025 rows.
  skew           d 768, 16 lists: one of 12,000 rows, the others 0 .. 40.
  dups           edges with blocks of rows whose scores tie exactly: A 300 copies in the 1025-row list (list
                 positions 200 .. 499: past the first 128, in every wave), B 70 copies in the 257-row list, C five
                 rows in two lists (3 + 2).  Exact copies always share a list, so C's rows are e_21 + h and
                 e_22 + h (h zero at 21 and 22) and its query e_21 + e_22 + h: equal int8 dots, equal scales, the
                 two lists tied on top of its probes.
  dup_centroids  d 256, nlist 260: identical centroids at (c, c + 4), (c, c + 32), (c, c + 64), (c, c + 128) — the
                 lane halves, MFMA tiles, waves and 128-centroid tiles of the assignment kernel — and one all-zero.
  dup_sample     2,048 training rows whose rows 0, step, 2 step are identical: three equal initial centroids.
  scales         planted rows times 2^e_r, e over -100 .. 100 (f16: -8 .. 8), lists 0 .. 3 small rows only; four
                 zero rows, a row that is zero but for one -1.0, a rint-tie row.  Queries "unit", "tiny" (times
                 2^-80: inv_r inv_q denormal or 0, scores +0.0 and -0.0), "zero" (all-zero).
  neg            planted rows with a common component, queries their negation: every fine score < 0.
  subscale       rows whose amax is below 127 / FLT_MAX (127 / amax = inf): zero rows by the oracle's rule.
"""
from dataclasses import dataclass, field

import numpy as np

from hostile import _unit, stored
from oracle import ivf as oivf

EDGE_SIZES = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 0, 1023, 1024, 1025, 3, 0, 511, 512, 513, 2, 64, 64, 700]
NOISE = 0.05
COMMON = 0.5      # neg: the shared component at e_{d-1}
COPY_NOISE = 0.3  # dups: a block's row is e_c + 0.3 g, so its self-dot stands clear of the list's other rows
SUB_AMAX = [2.0 ** -126, 2.0 ** -122, 1e-37, 2.0 ** -130]   # 127 / amax overflows: zero rows
NEAR_AMAX = [2.0 ** -121, 2.0 ** -120, 2.0 ** -100]         # just above 127 / FLT_MAX = 2^-121.0003: ordinary rows


@dataclass
class IvfCorpus:
    name: str
    dtype: str
    rows: np.ndarray            # [n][d] f32, stored values
    qc: np.ndarray              # [nlist][d] int8 centroid table (set_centroids); None: the test trains
    queries: dict               # name -> [nq][d] f32, stored values
    notes: dict = field(default_factory=dict)

    @property
    def nlist(self):
        return self.qc.shape[0]

    def quantized(self):
        """(codes, inv, labels, fc) of the rows under qc, by the oracle (computed once)."""
        if "_q" not in self.notes:
            codes, inv = oivf.quantize(self.rows)
            fc = oivf.centroid_factor(self.qc)
            self.notes["_q"] = (codes, inv, oivf.assign(codes, self.qc, fc), fc)
        return self.notes["_q"]


def onehot_centroids(nlist, d):
    qc = np.zeros((nlist, d), dtype=np.int8)
    qc[np.arange(nlist), np.arange(nlist)] = 127
    return qc


def _law(rng, lists, d, noise=NOISE, common=0.0):
    """One row per entry of `lists`: e_c + noise g (+ common e_{d-1}), f32."""
    x = noise * _unit(rng.standard_normal((len(lists), d)))
    x[np.arange(len(lists)), lists] += 1.0
    if common:
        x[:, d - 1] += common
    return x.astype(np.float32)


def planted(d, sizes, dtype, seed=11, common=0.0):
    """-> (rows f32 stored [n][d], labels [n], qc int8 [nlist][d], rng).  Asserts the oracle's assignment."""
    nlist = len(sizes)
    assert nlist < d
    rng = np.random.default_rng(seed)
    lab = rng.permutation(np.repeat(np.arange(nlist), sizes))
    rows = stored(_law(rng, lab, d, common=common), dtype)
    qc = onehot_centroids(nlist, d)
    got = oivf.assign(oivf.quantize(rows)[0], qc, oivf.centroid_factor(qc))
    assert np.array_equal(got, lab), "planted: the oracle assigns a row elsewhere"
    return rows, lab.astype(np.int32), qc, rng


def _queries(rng, nlist, d, nq, dtype, sizes, noise=NOISE, common=0.0, sign=1.0):
    """nq rows of the law aimed at the non-empty lists in turn (largest first)."""
    live = [c for c in np.argsort(-np.asarray(sizes), kind="stable") if sizes[c] > 0]
    lists = np.array([live[i % len(live)] for i in range(nq)])
    return stored(sign * _law(rng, lists, d, noise, common), dtype)


queries = _queries  # (for corpora built outside this module)


def edges(dtype="bf16", nq=33):
    rows, lab, qc, rng = planted(256, EDGE_SIZES, dtype, seed=11)
    q = _queries(rng, len(EDGE_SIZES), 256, nq, dtype, EDGE_SIZES)
    return IvfCorpus("edges", dtype, rows, qc, {"law": q}, {"labels": lab, "sizes": EDGE_SIZES})


def skew(dtype="bf16", nq=33):
    rng0 = np.random.default_rng(12)
    sizes = rng0.integers(0, 41, 16)
    sizes[[2, 9]] = 0
    sizes[5] = 12000
    sizes = sizes.tolist()
    rows, lab, qc, rng = planted(768, sizes, dtype, seed=13)
    q = _queries(rng, 16, 768, nq, dtype, sizes)
    return IvfCorpus("skew", dtype, rows, qc, {"law": q}, {"labels": lab, "sizes": sizes})


def dups(dtype="bf16", nq=33):
    d = 256
    rows, lab, qc, rng = planted(d, EDGE_SIZES, dtype, seed=11)
    members = lambda c: np.flatnonzero(lab == c)  # ascending row ids = list order
    la, lb, lc1, lc2 = EDGE_SIZES.index(1025), EDGE_SIZES.index(257), 21, 22
    va = stored(_law(rng, [la], d, COPY_NOISE), dtype)[0]
    vb = stored(_law(rng, [lb], d, COPY_NOISE), dtype)[0]
    block_a = members(la)[200:500]
    block_b = members(lb)[100:170]
    rows[block_a] = va
    rows[block_b] = vb
    h = COPY_NOISE * _unit(rng.standard_normal(d))
    h[[lc1, lc2]] = 0.0
    block_c = np.sort(np.concatenate([members(lc1)[[5, 30, 63]], members(lc2)[[0, 40]]]))
    for r in block_c:
        rows[r] = h
        rows[r, lab[r]] = 1.0
    qcv = h.copy()
    qcv[[lc1, lc2]] = 1.0
    rows = stored(rows, dtype)
    special = stored(np.stack([va, vb, qcv]).astype(np.float32), dtype)
    q = _queries(rng, len(EDGE_SIZES), d, nq, dtype, EDGE_SIZES)
    for i in range(0, nq, 3):  # queries 0, 3, 6, 9 .. = A, B, C, A ..
        q[i] = special[(i // 3) % 3]
    c = IvfCorpus("dups", dtype, rows, qc, {"law": q},
                  {"labels": lab, "sizes": EDGE_SIZES, "block_a": block_a, "block_b": block_b, "block_c": block_c,
                   "query_of": {"a": 0, "b": 3, "c": 6}, "lists_c": (lc1, lc2)})
    assert np.array_equal(c.quantized()[2], lab), "dups: a planted block left its list"
    return c


def dup_centroids(dtype="bf16", n=3000, nq=33):
    d, nlist = 256, 260
    rng = np.random.default_rng(14)
    dirs = _unit(rng.standard_normal((nlist, d)))
    qc = oivf.quantize(dirs.astype(np.float32))[0]
    # (c, c + 4): the two lane halves; + 32: the two MFMA tiles of a wave; + 64: the two centroid waves; + 128: two
    # 128-centroid tiles, (130, 258) into the ragged last tile of 4
    pairs = [(1, 5), (10, 42), (20, 84), (30, 158), (130, 258), (137, 141), (150, 182), (160, 224)]
    zero_c = 200
    for a, b in pairs:
        qc[b] = qc[a]
        dirs[b] = dirs[a]
    qc[zero_c] = 0
    near = np.array([a for a, _ in pairs] + [3, 77, 199, 259])  # rows gather near the paired centroids and a few others
    rl = near[rng.integers(0, near.size, n)]
    rows = stored(_unit(dirs[rl] + 0.3 * _unit(rng.standard_normal((n, d)))), dtype)
    # queries: one near each pair's direction (the tie on top: straddles nprobe 1), one mixing two other
    # directions above it (the tie at places 3 and 4: straddles nprobe 3), then rows of the law
    qs = []
    for a, _ in pairs:
        qs.append(dirs[a] + 0.1 * _unit(rng.standard_normal(d)))
        qs.append(1.0 * dirs[3] + 0.8 * dirs[77] + 0.6 * dirs[a])
    while len(qs) < nq:
        qs.append(dirs[near[len(qs) % near.size]] + 0.3 * _unit(rng.standard_normal(d)))
    q = stored(_unit(np.stack(qs[:nq])), dtype)
    return IvfCorpus("dup_centroids", dtype, rows, qc, {"law": q}, {"pairs": pairs, "zero_centroid": zero_c})


def dup_sample(dtype="bf16"):
    d, nlist, n = 256, 16, 2048
    rng = np.random.default_rng(15)
    dirs = _unit(rng.standard_normal((nlist, d)))
    x = _unit(dirs[rng.integers(0, nlist, n)] + 0.5 * _unit(rng.standard_normal((n, d))))
    step = n // nlist
    x[step] = x[0]
    x[2 * step] = x[0]
    return IvfCorpus("dup_sample", dtype, stored(x, dtype), None, {}, {"nlist": nlist, "step": step})


SCALE_SIZES = [300, 200, 150, 100, 130, 65, 64, 63, 1, 0, 257, 129, 40, 300, 128, 17]
SMALL_LISTS = 4  # lists 0 .. 3 hold small rows only: a tiny query that probes them sees nothing but zeros


def scales(dtype="bf16", nq=33):
    d = 256
    rows, lab, qc, rng = planted(d, SCALE_SIZES, dtype, seed=16)
    n = rows.shape[0]
    lo, hi = (-8, 8) if dtype == "f16" else (-100, 100)
    small_hi = -4 if dtype == "f16" else -60
    e = rng.integers(lo, hi + 1, n)
    big = np.flatnonzero(lab >= SMALL_LISTS)
    e[rng.permutation(big)[:hi - lo + 1]] = np.arange(lo, hi + 1)  # every exponent occurs, the extremes included
    small = lab < SMALL_LISTS
    e[small] = rng.integers(lo, small_hi + 1, int(small.sum()))
    rows = stored(rows * np.exp2(e).astype(np.float32)[:, None], dtype)
    assert np.isfinite(rows).all() and (np.abs(rows).max(axis=1) > 0).all()
    assert np.array_equal(oivf.assign(oivf.quantize(rows)[0], qc, oivf.centroid_factor(qc)), lab), "scales: a row moved"
    # planted rows (they leave their lists: the oracle says where to)
    spots = rng.permutation(np.flatnonzero(lab >= SMALL_LISTS))[:6]
    zero_rows, onehot_row, tie_row = np.sort(spots[:4]), int(spots[4]), int(spots[5])
    rows[zero_rows] = 0.0
    rows[onehot_row] = 0.0
    rows[onehot_row, d // 3] = -1.0
    j = np.arange(d)
    tie = ((j % 127) + 0.5) * 2.0 ** -7 * np.where((j // 127) % 2 == 0, 1.0, -1.0)
    tie[2 * d // 3] = 127 * 2.0 ** -7
    rows[tie_row] = tie
    assert np.array_equal(stored(rows, dtype), rows)
    unit = _queries(rng, len(SCALE_SIZES), d, nq, dtype, SCALE_SIZES)
    qdt = "f32" if dtype == "f16" else dtype  # (2^-80 is below f16: the tiny queries of an f16 store are f32)
    # tiny: louder noise.  The first 12 aim at a small list a, are exactly 0 at the other small lists and -0.05 at
    # the large ones: their probes are a, then the other small lists tied at coarse score 0 (lowest id first),
    # where a row's dot is 127 code_a + noise — either sign, so the list holds +0.0 and -0.0 side by side —
    # and every large list scores below 0.
    tl = np.array([i % SMALL_LISTS if i < 12 else 4 + i % 8 for i in range(nq)])
    tiny = _law(rng, tl, d, 0.3)
    for i in range(min(12, nq)):
        tiny[i, :SMALL_LISTS] = 0.0
        tiny[i, tl[i]] = 1.0
        tiny[i, SMALL_LISTS:len(SCALE_SIZES)] = -0.05
    tiny = stored(tiny * np.float32(2.0 ** -80), qdt)
    zero = np.zeros((nq, d), dtype=np.float32)
    return IvfCorpus("scales", dtype, rows, qc, {"unit": unit, "tiny": tiny, "zero": zero},
                     {"exponents": e, "zero_rows": zero_rows, "onehot_row": onehot_row, "tie_row": tie_row,
                      "sizes": SCALE_SIZES, "tiny_dtype": qdt})


NEG_SIZES = [40, 0, 129, 64, 300, 1, 65, 200]


def neg(dtype="bf16", nq=33):
    d = 256
    rows, lab, qc, rng = planted(d, NEG_SIZES, dtype, seed=17, common=COMMON)
    q = _queries(rng, len(NEG_SIZES), d, nq, dtype, NEG_SIZES, common=COMMON, sign=-1.0)
    return IvfCorpus("neg", dtype, rows, qc, {"neg": q}, {"labels": lab, "sizes": NEG_SIZES})


def subscale(dtype="f32", d=256):
    """One row per amax of SUB_AMAX + NEAR_AMAX: elements amax * {0, +-1, +-1/2, +-1/4}, most of them zero.
    notes["sub"]: the rows whose 127 / amax is not finite (the oracle's zero rows)."""
    assert dtype in ("f32", "bf16")
    rng = np.random.default_rng(18)
    am = stored(np.array(SUB_AMAX + NEAR_AMAX, dtype=np.float32), dtype)
    pat = rng.choice(np.array([0, 0, 0, 0, 1, -1, 0.5, -0.5, 0.25, -0.25], dtype=np.float32), (am.size, d))
    pat[:, 7] = -1.0  # the amax itself, negative
    rows = stored(pat * am[:, None], dtype)
    assert np.array_equal(np.abs(rows).max(axis=1), am)
    with np.errstate(over="ignore"):
        sub = ~np.isfinite(np.float32(127) / am)
    return IvfCorpus("subscale", dtype, rows, None, {}, {"sub": sub, "amax": am})


def ord_f32(s):
    """The kernels' orderable u32 of a float (rfx_device.h ord_f32): -0.0 strictly below +0.0."""
    u = np.asarray(s, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def search_by(rule, qq, qinv, codes, inv, labels, qc, fc, nprobe, k):
    """oracle.ivf.search with its ranking swapped out — the mutants that show which corpora discriminate:
    "oracle"   (score desc by float comparison, row asc): oracle.ivf.search itself, restated;
    "ord"      (ord_f32 key desc, row asc): +0.0 ranks above -0.0 whatever the rows;
    "row_desc" (score desc, row DESC): the tie rule reversed."""
    nq = qq.shape[0]
    pr = oivf.probes(qq, qc, fc, nprobe)
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    out_r = np.full((nq, k), -1, dtype=np.int64)
    for i in range(nq):
        rows = np.flatnonzero(np.isin(labels, pr[i]))
        if len(rows) == 0:
            continue
        d = oivf.int_dot(qq[i:i + 1], codes[rows])[0].astype(np.float32)
        s = d * (inv[rows] * qinv[i]).astype(np.float32)
        if rule == "oracle":
            o = np.lexsort((rows, -s))[:k]
        elif rule == "ord":
            o = np.lexsort((rows, -ord_f32(s).astype(np.int64)))[:k]
        elif rule == "row_desc":
            o = np.lexsort((-rows, -s))[:k]
        else:
            raise ValueError(rule)
        out_s[i, :len(o)] = s[o]
        out_r[i, :len(o)] = rows[o]
    return out_s, out_r


def same_bits(s, r, ref_s, ref_r):
    """The GPU tests' bar: rows equal, scores equal as uint32 (the sign of zero included)."""
    return np.array_equal(np.asarray(r), ref_r) and np.array_equal(
        np.ascontiguousarray(s, dtype=np.float32).view(np.uint32), ref_s.view(np.uint32))
