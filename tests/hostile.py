"""Hostile corpora for the exact two-pass scan: what oracle.synth's isotropic unit rows
never show it.  TEST INFRASTRUCTURE ONLY (tests/test_screen_hostile_oracle.py on the CPU,
tests/test_gpu_screen_hostile.py on the GPU); numpy and a seeded default_rng, nothing else.

Every builder returns a Corpus: rows and query sets as f32 arrays that hold STORED values (each is
exactly representable in `dtype`: an upload through stored() and the oracle see the same bits).

  aniso    normalize(0.6 m + 0.8 g): m a fixed unit direction, g gaussian with per-dimension spread
           exp(N(0, 0.7)), normalised — a shared-mean corpus (thousands of survivors per query).  Query sets:
           "same" (the rows' law) and "neg" (negated rows of the law, and -m itself): every exact score < 0.
  shifted  isotropic rows (with a small low-dimensional "topic" part, see SHIFT below) moved by -SHIFT u (u a
           dense unit direction) and normalised; queries lean to +u: every exact score < 0 (-0.42 +- 0.08), so
           the k-th screen score and the bound thr - e2 are negative, with few survivors.
  mixed    isotropic rows, tile t (32 rows) multiplied by 2^e_t, e_t uniform in -20..10 (f16: -8..8, nothing
           flushes or overflows); planted tiles: two live all-zero tiles, a tile that is zero but for one
           negative element (code -127), a "tie" tile of scale 2^-7 exactly whose elements (j + 0.5) 2^-7
           all land on rint ties (codes up to +-126, +127 for the amax).
  zeros    the shifted corpus with (a) one whole tile of zero rows, or (b) four zero rows: two in a tile
           whose other rows the caller tombstones (Corpus.dead), two elsewhere.  Every other score is
           negative, so the top-k is known outright: the zero rows in row order with score 0.0, then the
           best negatives.  (c): as (b) with the four rows scaled by 2^-20 instead of zeroed.  (d): 16 rows all over
           the store shrunk by 2^-3 .. 2^-18, the only rows near the k-th score: few enough survivors for a
           search cut into 8 workgroups to answer itself.
"""
from dataclasses import dataclass, field

import numpy as np

from oracle import synth as osynth

TM = 32
# shifted: rows normalize(g + TOPIC h - SHIFT u), queries normalize(g' + TOPIC h' + Q_LEAN u); g, h, u unit vectors, h in
# a fixed TOPIC_DIM-dimensional subspace (dense orthonormal basis).  Scores: -1.44 / 3.44 = -0.42 from the shift, at
# most +1 / 3.44 = +0.29 from the topics (h . h' <= 1), 0.018 sigma from g: negative whatever the draw (best -0.10).
# Why the topic part: plain isotropic rows spread their scores by 1 / sqrt(d) only, the width of the band
# 2 E_q ~ 0.04 itself, and 700 of 24,000 rows survive a query: the 8-wave kernel 10 answers that from its 512 lists,
# the 2-wave kernel's 112 lists of 10 overflow inside the band and the batch goes to the gated exact pass (first GPU
# run).  Sixteen topic dimensions widen the spread to 0.077: 66 .. 183 survivors, which every form answers itself
# (fewer dimensions crowd the scores against their upper edge: 8 gave 186 on average, 4 gave 275).
SHIFT = 1.2
Q_LEAN = 1.2
TOPIC = 1.0
TOPIC_DIM = 16


@dataclass
class Corpus:
    name: str
    dtype: str
    rows: np.ndarray                      # [n][d] f32, stored values
    queries: dict                         # name -> [nq][d] f32, stored values
    dead: list = field(default_factory=list)   # rows the caller tombstones after the upload
    notes: dict = field(default_factory=dict)  # planted tiles / rows by name


def stored(x, dtype):
    """f32 values rounded to `dtype` (round to nearest even) and widened back: exact stored values."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "f32":
        return x
    if dtype == "bf16":
        return osynth.bf16_bits_to_f32(osynth.f32_to_bf16_bits(x)).reshape(x.shape)
    if dtype == "f16":
        return x.astype(np.float16).astype(np.float32)
    raise ValueError(dtype)


def live_rows(c: Corpus):
    """The rows as the index holds them after the caller's tombstones: dead rows NaN."""
    x = c.rows.copy()
    if c.dead:
        x[c.dead] = np.nan
    return x


def scale_bound(rows32, q32):
    """S = max(1, max ||x|| max ||q||): what the unit-norm tolerances of check_topk scale by."""
    x = np.asarray(rows32, dtype=np.float64)
    ok = ~np.isnan(x).any(axis=1)
    xn = np.sqrt((x[ok] ** 2).sum(axis=1)).max() if ok.any() else 0.0
    qn = np.sqrt((np.asarray(q32, dtype=np.float64) ** 2).sum(axis=1)).max()
    return max(1.0, float(xn * qn))


def _unit(v):
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def _best_scores(rows32, q32):
    x = np.asarray(rows32, dtype=np.float64)
    ok = ~np.isnan(x).any(axis=1)
    return (np.asarray(q32, dtype=np.float64) @ x[ok].T).max(axis=1)


def _aniso_law(rng, n, m, spread):
    g = _unit(rng.standard_normal((n, m.size)) * spread)
    return _unit(0.6 * m + 0.8 * g)


def aniso(n, d, dtype, nq, seed=101):
    rng = np.random.default_rng(seed)
    m = _unit(rng.standard_normal(d))
    spread = np.exp(rng.normal(0.0, 0.7, d))
    rows = stored(_aniso_law(rng, n, m, spread), dtype)
    same = stored(_aniso_law(rng, nq, m, spread), dtype)
    neg = -_aniso_law(rng, nq, m, spread)
    neg[0] = -m
    neg = stored(neg, dtype)
    best = _best_scores(rows, neg)
    assert (best < 0).all(), f"aniso/neg: a best score is not negative ({best.max():.4f})"
    return Corpus("aniso", dtype, rows, {"same": same, "neg": neg})


def shifted(n, d, dtype, nq, seed=202):
    rng = np.random.default_rng(seed)
    u = _unit(rng.standard_normal(d))
    basis = np.linalg.qr(rng.standard_normal((d, TOPIC_DIM)))[0].T  # [TOPIC_DIM][d], orthonormal rows

    def law(m, sign):
        h = _unit(rng.standard_normal((m, TOPIC_DIM))) @ basis
        return _unit(_unit(rng.standard_normal((m, d))) + TOPIC * h + sign * u)

    rows = stored(law(n, -SHIFT), dtype)
    q = stored(law(nq, Q_LEAN), dtype)
    best = _best_scores(rows, q)
    assert (best < 0).all(), f"shifted: a best score is not negative ({best.max():.4f})"
    return Corpus("shifted", dtype, rows, {"lean": q})


def mixed(n, d, dtype, nq, seed=303):
    rng = np.random.default_rng(seed)
    nt = -(-n // TM)
    assert nt >= 16, "mixed needs room for its planted tiles"
    lo, hi = (-8, 8) if dtype == "f16" else (-20, 10)
    e = rng.integers(lo, hi + 1, nt)
    e[rng.permutation(nt)[:hi - lo + 1]] = np.arange(lo, hi + 1)  # every exponent occurs, the extremes included
    rows = _unit(rng.standard_normal((n, d))).astype(np.float32)
    rows = stored(rows * np.repeat(np.exp2(e), TM)[:n, None].astype(np.float32), dtype)
    zero_tiles = [3, nt // 2]
    onehot_tile, tie_tile = 7, nt - 3
    for t in zero_tiles:
        rows[t * TM:(t + 1) * TM] = 0.0
    rows[onehot_tile * TM:(onehot_tile + 1) * TM] = 0.0
    onehot_row, onehot_col = onehot_tile * TM + 13, d // 3
    rows[onehot_row, onehot_col] = -1.0
    # the tie tile: s_t = 2^-7 exactly (amax 127 2^-7), every other element (j + 0.5) 2^-7, j < 127, in both
    # signs: x / s_t = +-(j + 0.5) exactly, a rint tie (to even); 2 j + 1 <= 253 fits bf16's 8 significant bits
    i = np.arange(TM * d)
    tie = ((i % 127) + 0.5) * 2.0 ** -7 * np.where((i // 127) % 2 == 0, 1.0, -1.0)
    tie = tie.reshape(TM, d).astype(np.float32)
    tie_row, tie_col = tie_tile * TM + 5, 2 * d // 3
    tie[5, 2 * d // 3] = 127 * 2.0 ** -7
    rows[tie_tile * TM:(tie_tile + 1) * TM] = tie
    assert np.array_equal(stored(rows, dtype), rows)
    assert np.isfinite(rows).all() and (dtype != "f16" or np.abs(rows).max() < 65504)
    q = stored(_unit(rng.standard_normal((nq, d))), dtype)
    notes = {"zero_tiles": zero_tiles, "onehot_tile": onehot_tile, "onehot_row": onehot_row, "tie_tile": tie_tile,
             "tie_row": tie_row, "exponents": e}
    return Corpus("mixed", dtype, rows, {"iso": q}, notes=notes)


def zeros(n, d, dtype, nq, variant, seed=202):
    """variant "a": tile ZT is 32 zero rows.  variant "b": rows ZT*32 + 4 and + 21 are zero and the tile's other
    30 rows are to be tombstoned (Corpus.dead); two more zero rows stand in other tiles.  variant "c": as "b", the
    four rows multiplied by 2^-20 instead of zeroed (bf16 / f32): scores of -4e-7, the best of the store, in a tile
    of scale 2^-30 — a negative bound divided by a tiny scale, the -2^30 clamp of the integer pass mask."""
    c = shifted(n, d, dtype, nq, seed)
    nt = n // TM
    zt = nt // 3
    rows = c.rows
    if variant == "a":
        zr = list(range(zt * TM, (zt + 1) * TM))
        dead = []
    elif variant == "d":
        zr, dead = [], []
    elif variant in ("b", "c"):
        zr = sorted([zt * TM + 4, zt * TM + 21, 9, (nt - 2) * TM + 31])
        dead = [r for r in range(zt * TM, (zt + 1) * TM) if r not in zr]
    else:
        raise ValueError(variant)
    if variant == "d":
        # 16 rows all over the store shrunk by 2^-3 .. 2^-18: scores -0.05 .. -1.6e-6, above every other row's (the
        # best of those is about -0.10) and, from 2^-4 on, the only ones inside the band of 0.04 below the k-th
        zr = sorted(np.random.default_rng(seed + 1).choice(n, 16, replace=False).tolist())
        assert dtype != "f16"
        for j, r in enumerate(np.random.default_rng(seed + 2).permutation(zr)):
            rows[r] = stored(rows[r] * np.float32(2.0 ** -(j + 3)), dtype)
        return Corpus("zeros_d", dtype, rows, c.queries, notes={"zero_rows": zr})
    if variant == "c":
        rows[zr] = stored(rows[zr] * np.float32(2.0 ** -20), dtype)
        assert dtype != "f16" and (np.abs(rows[zr]).max(axis=1) > 0).all()
    else:
        rows[zr] = 0.0
    return Corpus("zeros_" + variant, dtype, rows, c.queries, dead=dead, notes={"zero_rows": zr, "zero_tile": zt})


def known_zero_answer(c: Corpus, k, f32_rule=False):
    """(rows [nq][k], zero count) of a zeros corpus: the zero rows in row order, then the best negatives
    (f64 scores, row ascending; f32_rule: the scores rounded to f32 first, the score rule of every GPU plan) —
    exact because every other score is < 0."""
    zr = np.asarray(c.notes["zero_rows"], dtype=np.int64)
    x = live_rows(c).astype(np.float64)
    q = next(iter(c.queries.values())).astype(np.float64)
    s = q @ np.where(np.isnan(x), 0.0, x).T
    s[:, np.isnan(x).any(axis=1)] = -np.inf
    nz = min(k, zr.size)
    out = np.empty((q.shape[0], k), dtype=np.int64)
    out[:, :nz] = zr[:nz]
    rest = s.astype(np.float32).astype(np.float64) if f32_rule else s.copy()
    rest[:, zr] = -np.inf
    assert (rest.max(axis=1) < 0).all()
    for i in range(q.shape[0]):
        out[i, nz:] = np.lexsort((np.arange(s.shape[1]), -rest[i]))[:k - nz]
    return out, nz
