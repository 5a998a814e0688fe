"""CPU reference of the MMR selection rule (rfx_mmr_select), numpy float64.

Per query: candidates (score f32, row int64) in search order; a candidate whose row is outside [0, rows) or
whose stored row holds a NaN is padding.  sim(i, j) = fl32 of the f64 dot of stored rows i and j.  Step 0
picks the first valid candidate; step t >= 1 the unpicked valid candidate that maximises
L * f64(s_i) - (1 - L) * f64(max over picked j of sim(i, j)), every operation rounded on its own (numpy
scalars never fuse), L = f64(f32(lambda)); ties go to the lower position.  Padded with (-inf, -1)."""
import numpy as np

MARGIN = 1e-6  # a query whose best and second-best objective lie closer than this at some step may differ


def select(cand_s, cand_r, rows64, k, lam, n_cand=None):
    """One query.  cand_s f32 [n_max], cand_r int64 [n_max], rows64 f64 [rows][dim] (the stored rows widened
    exactly; tombstoned rows NaN).  Returns (scores f32 [k], rows int64 [k], objectives f64 [k], margin):
    margin = the smallest gap between the best and the second-best objective over the steps t >= 1 that had
    a choice (inf when none had)."""
    cand_s = np.asarray(cand_s, dtype=np.float32)
    cand_r = np.asarray(cand_r, dtype=np.int64)
    n = len(cand_s) if n_cand is None else int(n_cand)
    L = np.float64(np.float32(lam))
    valid = [bool(0 <= cand_r[i] < len(rows64)) and not np.isnan(rows64[cand_r[i]]).any() for i in range(n)]
    avail = [i for i in range(n) if valid[i]]
    m = np.full(n, -np.inf, dtype=np.float32)
    out_s = np.full(k, -np.inf, dtype=np.float32)
    out_r = np.full(k, -1, dtype=np.int64)
    out_o = np.full(k, -np.inf, dtype=np.float64)
    margin = np.inf
    for t in range(k):
        if not avail:
            break
        if t == 0:
            pick, obj = avail[0], L * np.float64(cand_s[avail[0]])
        else:
            objs = [L * np.float64(cand_s[i]) - (np.float64(1.0) - L) * np.float64(m[i]) for i in avail]
            best = max(objs)
            at = objs.index(best)  # the lowest position among the equals
            pick, obj = avail[at], best
            if len(objs) > 1:
                margin = min(margin, best - max(o for j, o in enumerate(objs) if j != at))
        out_s[t], out_r[t], out_o[t] = cand_s[pick], cand_r[pick], obj
        avail.remove(pick)
        if avail:
            sims = (rows64[cand_r[avail]] @ rows64[cand_r[pick]]).astype(np.float32)
            m[avail] = np.maximum(m[avail], sims)
    return out_s, out_r, out_o, margin


def select_batch(cand_s, cand_r, rows64, k, lam=0.5, n_cand=None):
    """[nq][n_max] candidates -> (scores [nq][k], rows [nq][k], objectives [nq][k], margins [nq]); lam and
    n_cand are scalars or [nq]."""
    nq = len(cand_s)
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float32), (nq,))
    nc = [None] * nq if n_cand is None else np.broadcast_to(np.asarray(n_cand), (nq,))
    res = [select(cand_s[q], cand_r[q], rows64, k, lam[q], nc[q]) for q in range(nq)]
    return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res]),
            np.array([r[3] for r in res]))


def check_valid(sel_s, sel_r, cand_s, cand_r):
    """What every selection satisfies whatever the arithmetic: a subset of the candidates with their own
    scores, no repeats, candidate 0 first."""
    pairs = {(int(r), np.float32(s).tobytes()) for s, r in zip(cand_s, cand_r)}
    got = [(int(r), np.float32(s).tobytes()) for s, r in zip(sel_s, sel_r) if r >= 0]
    assert all(p in pairs for p in got), "a pick is no candidate"
    assert len(set(r for r, _ in got)) == len(got), "a row picked twice"
    assert got and got[0][0] == int(cand_r[0]), "the first pick is not candidate 0"
