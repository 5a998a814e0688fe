"""GPU: reciprocal-rank fusion (rfx_lex_fuse) against the numpy reference (tests/lex_ref.py), bit for bit on
scores, rows and ranks: only correctly rounded f64 adds, one subtract and divisions are involved."""
import numpy as np
import pytest
import torch

import lex_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ix():
    from rfx.lexical import LexIndex
    x = LexIndex(64)
    yield x
    x.close()


def _lists(seed, nq, n_d, n_l, universe=150, pad=0.0):
    """per question two lists of distinct rows drawn from a small universe (so they overlap), some padding"""
    rng = np.random.default_rng(seed)
    d = np.stack([rng.permutation(universe)[:n_d] for _ in range(nq)]).astype(np.int64)
    l = np.stack([rng.permutation(universe)[:n_l] for _ in range(nq)]).astype(np.int64)
    if pad:
        d[rng.random(d.shape) < pad] = -1
        l[rng.random(l.shape) < pad] = -1
    return d, l


def _fuse(ix, d, l, k, alpha, **kw):
    s, r, rk = ix.fuse(torch.from_numpy(d).cuda(), torch.from_numpy(l).cuda(), k, alpha, ranks=True, **kw)
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy(), rk.cpu().numpy()


def _check(ix, d, l, k, alpha, **kw):
    gs, gr, gk = _fuse(ix, d, l, k, alpha, **kw)
    rs, rr, rk = lex_ref.rrf_batch(d, l, k, alpha, kw.get("n_dense"), kw.get("n_lex"), kw.get("rrf_c", 60))
    assert np.array_equal(gr, rr), (gr, rr)
    assert np.array_equal(gs.view(np.uint32), rs.view(np.uint32))
    assert np.array_equal(gk, rk)
    return gs, gr, gk


@pytest.mark.parametrize("nq", [1, 7, 256])
@pytest.mark.parametrize("n_d,n_l", [(1, 1), (10, 10), (64, 64), (40, 17)])
def test_fuse_matches_the_reference(ix, nq, n_d, n_l):
    d, l = _lists(nq * 100 + n_d, nq, n_d, n_l, pad=0.1 if n_d > 1 else 0.0)
    rng = np.random.default_rng(nq + n_l)
    alpha = rng.random(nq).astype(np.float32)
    for k in (1, 10, 64):
        if k > n_d + n_l:
            continue
        for c in (1, 60):
            _check(ix, d, l, k, alpha, rrf_c=c)
    # mixed list lengths per question
    nd = rng.integers(1, n_d + 1, nq).astype(np.int32)
    nl = rng.integers(1, n_l + 1, nq).astype(np.int32)
    _check(ix, d, l, min(10, n_d + n_l), alpha, n_dense=nd, n_lex=nl)


def test_list_shapes(ix):
    d = np.arange(10, dtype=np.int64)[None]
    # disjoint, identical, one list all padding, padding in the middle of a hand-assembled list
    _check(ix, d, d + 100, 20, 0.5)
    gs, gr, gk = _check(ix, d, d.copy(), 20, 0.3)
    assert (gr[0, 10:] == -1).all() and np.isneginf(gs[0, 10:]).all() and (gk[0, 10:] == 0).all()  # k > n_d + n_l - overlap
    _check(ix, d, np.full((1, 10), -1, np.int64), 12, 0.5)
    _check(ix, np.full((1, 10), -1, np.int64), d, 12, 0.5)
    _check(ix, np.full((1, 3), -1, np.int64), np.full((1, 3), -5, np.int64), 4, 0.5)
    hand_d = np.array([[5, -1, 9, -1, -1, 2]], np.int64)
    hand_l = np.array([[-1, 9, 40, -1, 5, 41]], np.int64)
    gs, gr, gk = _check(ix, hand_d, hand_l, 6, 0.5)
    assert gk[0, list(gr[0]).index(9)].tolist() == [2, 1] and gk[0, list(gr[0]).index(2)].tolist() == [3, 0]


def test_alpha_extremes_ties_and_prefix_stability(ix):
    d, l = _lists(5, 7, 40, 40)
    for k in (1, 10, 40):
        assert np.array_equal(_check(ix, d, l, k, 1.0)[1], d[:, :k])
        assert np.array_equal(_check(ix, d, l, k, 0.0)[1], l[:, :k])
    _check(ix, d, l, 64, 0.5)
    # exact f64 ties: alpha 0.5, ranks (1, 2) and (2, 1) -> the lower row first
    gs, gr, gk = _check(ix, np.array([[8, 3]], np.int64), np.array([[3, 8]], np.int64), 2, 0.5)
    assert gr.tolist() == [[3, 8]] and gs[0, 0] == gs[0, 1]
    # prefix stability 64 -> 10
    d, l = _lists(6, 7, 64, 64)
    a = np.linspace(0.05, 0.95, 7).astype(np.float32)
    s64, r64, k64 = _check(ix, d, l, 64, a)
    s10, r10, k10 = _check(ix, d, l, 10, a)
    assert np.array_equal(r64[:, :10], r10) and np.array_equal(s64[:, :10], s10) and np.array_equal(k64[:, :10], k10)


def test_per_question_alphas_equal_the_questions_alone(ix):
    d, l = _lists(8, 7, 30, 25, pad=0.1)
    a = np.array([0.0, 1.0, 0.5, 0.25, 0.75, 0.1, 0.9], np.float32)
    nd = np.array([30, 1, 17, 30, 5, 29, 12], np.int32)
    nl = np.array([25, 25, 1, 9, 25, 3, 20], np.int32)
    gs, gr, gk = _check(ix, d, l, 10, a, n_dense=nd, n_lex=nl)
    for q in range(7):
        s1, r1, k1 = _fuse(ix, d[q:q + 1], l[q:q + 1], 10, a[q:q + 1], n_dense=nd[q:q + 1], n_lex=nl[q:q + 1])
        assert np.array_equal(s1[0], gs[q]) and np.array_equal(r1[0], gr[q]) and np.array_equal(k1[0], gk[q])


def test_refused_arguments_leave_the_outputs_untouched(ix):
    d, l = _lists(9, 2, 10, 10)
    dt, lt = torch.from_numpy(d).cuda(), torch.from_numpy(l).cuda()
    out = (torch.full((2, 10), 7.0, dtype=torch.float32, device="cuda"),
           torch.full((2, 10), 7, dtype=torch.int64, device="cuda"),
           torch.full((2, 10, 2), 7, dtype=torch.int32, device="cuda"))
    nan = float("nan")
    bad = [dict(k=0), dict(k=65), dict(k=21), dict(k=10, alpha=[0.5, 1.5]), dict(k=10, alpha=[-0.1, 0.5]),
           dict(k=10, alpha=[nan, 0.5]), dict(k=10, rrf_c=0), dict(k=10, n_dense=[0, 10]), dict(k=10, n_dense=[1, 11]),
           dict(k=10, n_lex=[11, 1]), dict(k=10, n_lex=0)]
    for kw in bad:
        kw.setdefault("alpha", 0.5)
        with pytest.raises(ValueError):
            ix.fuse(dt, lt, ranks=True, out=out, **kw)
    wide = torch.zeros((2, 65), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        ix.fuse(wide, lt, 10, 0.5, ranks=True, out=out)
    many = torch.zeros((1025, 4), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        ix.fuse(many, many, 4, 0.5)
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == 7)) for t in out)
