"""GPU: the BM25 lexical scan (rfx_lex_search) against the numpy reference (tests/lex_ref.py) on the
generator's CSR.  Comparison rule (lex_ref.compare_topk): scores equal to the reference's or an adjacent f32
(the f64 evaluation errs by a few 1e-16 relative, far under half an f32 ulp, so the two roundings differ by at
most one ulp); rows identical, except that a question whose reference scores hold two neighbours within one
f32 ulp is left out of the row comparison: at most 2 % of a test's questions."""
import numpy as np
import pytest
import torch

import lex_ref

pytestmark = pytest.mark.gpu

ROWS, V, ABSENT = lex_ref.GPU_ROWS, lex_ref.GPU_V, lex_ref.GPU_ABSENT


@pytest.fixture(scope="module")
def corpus():
    """lex_ref.gpu_corpus: 20,000 rows with the special rows at the first, last, tile- and workgroup-boundary
    positions; tests/test_lex_host.py checks the near-tie allowance on the same corpus and question sets"""
    from rfx.lexical import LexIndex
    csr = lex_ref.gpu_corpus()
    ref = lex_ref.RefIndex(V)
    ref.add(*csr)
    ix = LexIndex(V)
    # growth: 4096 -> 8192 -> 16384 -> 32768 rows, three reallocations after the first allocation
    for lo in range(0, ROWS, 2500):
        ix.add_csr(*lex_ref.slice_csr(csr, lo, min(lo + 2500, ROWS)))
    assert ix.rows == ROWS and ix.live_rows == ROWS
    yield ix, ref, csr
    ix.close()


def _search(ix, questions, k, **kw):
    s, r = ix.search(lex_ref.question_csr(questions), k, **kw)
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy()


def test_statistics_match_the_reference(corpus):
    ix, ref, _ = corpus
    N, df, total = ref.stats()
    rows, live, nnz, total_len = ix.info()
    assert (rows, live, total_len) == (ROWS, N, total) and nnz == ref.e_row.size
    assert np.array_equal(ix.df(), df)


@pytest.mark.parametrize("nq", [1, 8, 9, 33])
@pytest.mark.parametrize("k", [1, 10, 64])
def test_scan_matches_the_reference(corpus, nq, k):
    ix, ref, csr = corpus
    qs = lex_ref.gpu_question_sets(csr)["scan"][0][:nq]
    assert len(qs) == nq
    gs, gr = _search(ix, qs, k)
    skipped = lex_ref.compare_topk(gs, gr, ref, qs, k)
    print(f"nq {nq} k {k}: {skipped} of {nq} questions left out of the row comparison")
    assert skipped <= 0.02 * nq, skipped


def test_question_shapes(corpus):
    """one bucket; buckets no row holds (all padding); a repeated term (qtf 3); an empty question"""
    ix, ref, csr = corpus
    _, df, _ = ref.stats()
    absent = np.asarray(ABSENT)
    assert np.all(df[absent] == 0)
    common = int(np.argmax(df))
    qs = [([common], [1]), (absent[:2], [1, 1]), ([common, 17, common, common], [1, 2, 1, 1]), ([], []),
          ([common, 17], [3, 2])]
    gs, gr = _search(ix, qs, 10)
    assert lex_ref.compare_topk(gs, gr, ref, qs, 10) == 0
    assert np.all(gr[1] == -1) and np.all(gr[3] == -1) and np.all(np.isneginf(gs[1]))
    assert np.array_equal(gs[2], gs[4]) and np.array_equal(gr[2], gr[4])  # qtf 3 = the term three times


def test_parameters(corpus):
    ix, ref, csr = corpus
    qs, _, params, _ = lex_ref.gpu_question_sets(csr)["parameters"]
    for k1, b in params:
        gs, gr = _search(ix, qs, 10, k1=k1, b=b)
        assert lex_ref.compare_topk(gs, gr, ref, qs, 10, k1=k1, b=b) == 0


def test_alone_and_in_a_batch_bit_identical(corpus):
    ix, ref, csr = corpus
    qs = lex_ref.gpu_question_sets(csr)["batch"][0]
    bs, br = _search(ix, qs, 64)
    for qi in (0, 7, 8, 32):
        s1, r1 = _search(ix, [qs[qi]], 64)
        assert np.array_equal(s1[0], bs[qi]) and np.array_equal(r1[0], br[qi]), qi


def test_row_mask_sparse_empty_and_full_words(corpus):
    ix, ref, csr = corpus
    m, allowed = lex_ref.gpu_mask_words()
    words = m.size
    mask = torch.from_numpy(m.view(np.int32)).cuda()
    qs = lex_ref.gpu_question_sets(csr)["mask"][0]
    gs, gr = _search(ix, qs, 10, row_mask=mask)
    assert lex_ref.compare_topk(gs, gr, ref, qs, 10, allowed=allowed) == 0
    assert allowed[gr[gr >= 0]].all()
    zero = torch.zeros(words, dtype=torch.int32, device="cuda")
    assert np.all(_search(ix, qs, 10, row_mask=zero)[1] == -1)


def test_small_stores():
    from rfx.lexical import LexIndex
    for n, k in ((1, 1), (1, 10), (5, 10)):
        csr = lex_ref.gen_csr(3, n, V=64, lengths=6, skew=1.0)
        ref = lex_ref.RefIndex(64)
        ref.add(*csr)
        ix = LexIndex(64)
        ix.add_csr(*csr)
        qs = [(csr[1][:3], [1, 1, 1]), (np.arange(64), np.ones(64, np.int64))]
        gs, gr = _search(ix, qs, k)
        assert lex_ref.compare_topk(gs, gr, ref, qs, k) == 0
        assert (gr[1] >= 0).sum() == min(n, k)
        ix.close()
    # an index without rows answers padding
    ix = LexIndex(64)
    gs, gr = _search(ix, [([1], [1])], 4)
    assert np.all(gr == -1) and np.all(np.isneginf(gs))
    ix.close()


def test_wide_vocabulary_top_bit_of_the_packing():
    from rfx.lexical import LexIndex
    W = 65536
    csr = lex_ref.gen_csr(13, 3000, V=W, max_len=80, skew=0.5)  # skew < 1: most buckets in the upper half
    assert (csr[1] >= 32768).mean() > 0.4 and csr[1].max() >= 65000
    ref = lex_ref.RefIndex(W)
    ref.add(*csr)
    ix = LexIndex(W)
    ix.add_csr(*csr)
    hi = np.unique(csr[1][csr[1] >= 32768])
    qs = [(hi[i::97][:8], np.ones(hi[i::97][:8].size, np.int64)) for i in range(9)] + [([65535, 32768], [1, 1])]
    for group in (qs, qs[:1]):
        gs, gr = _search(ix, group, 10)
        assert lex_ref.compare_topk(gs, gr, ref, group, 10) == 0
    assert np.array_equal(ix.df(), ref.stats()[1])
    ix.close()


def test_tombstones_change_the_statistics_and_dead_rows_never_return():
    from rfx.lexical import LexIndex
    csr = lex_ref.gen_csr(31, 3000, max_len=120)
    ref = lex_ref.RefIndex(V)
    ref.add(*csr)
    ix = LexIndex(V)
    ix.add_csr(*csr)
    qs = lex_ref.gen_questions(5, 9)
    before_s, before_r = _search(ix, qs, 10)
    dead = np.unique(np.concatenate([before_r[:, 0][before_r[:, 0] >= 0], np.arange(0, 3000, 3)]))  # every best row, and a third
    ix.tombstone(dead)
    ix.tombstone(dead[:5])  # again: nothing changes
    ref.tombstone(dead)
    assert ix.live_rows == 3000 - dead.size and np.array_equal(ix.df(), ref.stats()[1])
    gs, gr = _search(ix, qs, 10)
    assert lex_ref.compare_topk(gs, gr, ref, qs, 10) == 0
    assert not np.isin(gr, dead).any() and not np.array_equal(gs, before_s)
    # ... and equal a fresh index over the live rows, bit for bit, under the renumbering
    fresh_ref, old = ref.fresh()
    keep = np.zeros(3000, bool)
    keep[old] = True
    ip = np.asarray(csr[0], np.int64)
    sel = np.repeat(keep, np.diff(ip))
    fip = np.concatenate([[0], np.cumsum(np.diff(ip)[keep])]).astype(np.int32)
    fx = LexIndex(V)
    fx.add_csr(fip, csr[1][sel], csr[2][sel])
    fs, fr = _search(fx, qs, 10)
    assert np.array_equal(fs, gs) and np.array_equal(np.where(fr >= 0, old[np.maximum(fr, 0)], -1), gr)
    ix.close()
    fx.close()


def test_refused_arguments_leave_the_outputs_untouched(corpus):
    ix, ref, csr = corpus
    q = lex_ref.question_csr([([1, 2], [1, 1])])
    s = torch.full((1, 10), 7.0, dtype=torch.float32, device="cuda")
    r = torch.full((1, 10), 7, dtype=torch.int64, device="cuda")
    small = torch.empty(64, dtype=torch.uint8, device="cuda")
    short_mask = torch.zeros(3, dtype=torch.int32, device="cuda")
    nan = float("nan")
    bad = [dict(k=0), dict(k=65), dict(k=10, k1=-1.0), dict(k=10, k1=nan), dict(k=10, b=-0.5), dict(k=10, b=1.5),
           dict(k=10, b=nan), dict(k=10, workspace=small), dict(k=10, row_mask=short_mask)]
    for kw in bad:
        with pytest.raises(ValueError):
            ix.search(q, out=(s, r), **kw)
    for csr_bad in ((np.array([0, 2, 1]), [1, 2], [1, 1]), (np.array([0, 1]), [V], [1]), (np.array([0, 1]), [-1], [1]),
                    (np.array([0]), [], [])):  # non-monotone, bucket >= V, bucket < 0, nq = 0
        with pytest.raises(ValueError):
            ix.search((csr_bad[0], np.asarray(csr_bad[1], np.int32), np.asarray(csr_bad[2], np.int16)), 10, out=(s, r))
    big = lex_ref.question_csr([([1], [1])] * 1025)
    with pytest.raises(ValueError):
        ix.search(big, 10)
    with pytest.raises(ValueError):
        ix.add_csr(np.array([0, 1]), [V], [1])
    with pytest.raises(ValueError):
        ix.tombstone([ROWS])
    torch.cuda.synchronize()
    assert torch.all(s == 7.0) and torch.all(r == 7) and ix.rows == ROWS and ix.live_rows == ROWS
