"""GPU: reciprocal-rank fusion at depth (rfx_lex_fuse_deep) against the numpy reference (tests/lex_ref.py), bit for
bit on scores, rows and ranks: only correctly rounded f64 adds, one subtract and divisions are involved."""
import numpy as np
import pytest
import torch

import lex_ref

pytestmark = pytest.mark.gpu

ALPHA = np.array([0.0, 1.0, 0.5, 0.3, 0.9], np.float32)


@pytest.fixture(scope="module")
def ix():
    from rfx.lexical import LexIndex
    x = LexIndex(64)
    yield x
    x.close()


def _lists(seed, n_d, n_l, overlap):
    """five questions, distinct rows per list (large row ids among them); the lexical rows share none, about half
    or all of their universe with the dense ones; padding inside the lists; one row repeated in a dense list"""
    rng = np.random.default_rng(seed)
    n = max(n_d, n_l)
    universe = np.arange({"none": 2 * n, "half": 3 * n // 2, "all": n}[overlap], dtype=np.int64) * 2_000_003 + 5
    d = np.stack([rng.permutation(universe[:n])[:n_d] for _ in ALPHA])
    l = np.stack([rng.permutation(universe[-n:])[:n_l] for _ in ALPHA])
    d[rng.random(d.shape) < 0.1] = -1
    l[rng.random(l.shape) < 0.1] = -1
    d[0, 40], d[0, 3] = 11, 11
    return d, l


def _check(ix, d, l, k, **kw):
    s, r, rk = ix.fuse_deep(torch.from_numpy(d).cuda(), torch.from_numpy(l).cuda(), k, ALPHA, ranks=True, **kw)
    torch.cuda.synchronize()
    rs, rr, rrk = lex_ref.rrf_batch(d, l, k, ALPHA, kw.get("n_dense"), kw.get("n_lex"), kw.get("rrf_c", 60))
    assert np.array_equal(r.cpu().numpy(), rr)
    assert np.array_equal(s.cpu().numpy().view(np.uint32), rs.view(np.uint32))
    assert np.array_equal(rk.cpu().numpy(), rrk)


@pytest.mark.parametrize("overlap", ["none", "half", "all"])
@pytest.mark.parametrize("n_d,n_l,k", [(65, 65, 65), (1024, 1024, 1024), (1024, 1, 100), (700, 1000, 1024)])
def test_fuse_deep_matches_the_reference(ix, n_d, n_l, k, overlap):
    d, l = _lists(n_d + n_l, n_d, n_l, overlap)
    _check(ix, d, l, k)
    rng = np.random.default_rng(k)
    _check(ix, d, l, k, rrf_c=1, n_dense=rng.integers(1, n_d + 1, 5).astype(np.int32),
           n_lex=rng.integers(1, n_l + 1, 5).astype(np.int32))


def test_refused_arguments_leave_the_outputs_untouched(ix):
    d, l = _lists(9, 100, 100, "half")
    dt, lt = torch.from_numpy(d).cuda(), torch.from_numpy(l).cuda()
    out = (torch.full((5, 100), 7.0, dtype=torch.float32, device="cuda"),
           torch.full((5, 100), 7, dtype=torch.int64, device="cuda"),
           torch.full((5, 100, 2), 7, dtype=torch.int32, device="cuda"))
    for kw in (dict(k=0), dict(k=1025), dict(k=201), dict(k=100, alpha=1.5), dict(k=100, alpha=float("nan")),
               dict(k=100, rrf_c=0), dict(k=100, n_dense=101), dict(k=100, n_lex=0)):
        kw.setdefault("alpha", 0.5)
        with pytest.raises(ValueError):
            ix.fuse_deep(dt, lt, ranks=True, out=out, **kw)
    wide = torch.zeros((5, 1025), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        ix.fuse_deep(wide, lt, 100, 0.5, ranks=True, out=out)
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == 7)) for t in out)
