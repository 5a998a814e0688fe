"""GPU: the deep BM25 scan (rfx_lex_search_deep, k in 65..1,024) against the numpy reference (tests/lex_ref.py)
under test_gpu_lex.py's comparison rule, and bit for bit against rfx_lex_search on the first 64 entries."""
import numpy as np
import pytest
import torch

import lex_ref

pytestmark = pytest.mark.gpu

ROWS, V = lex_ref.GPU_ROWS, lex_ref.GPU_V


def _index(csr, v=V):
    from rfx.lexical import LexIndex
    ref = lex_ref.RefIndex(v)
    ref.add(*csr)
    ix = LexIndex(v)
    ix.add_csr(*csr)
    return ix, ref


@pytest.fixture(scope="module")
def corpus():
    """lex_ref.gpu_corpus (20,000 rows, special rows at tile and workgroup edges) and the 45 questions: 11 groups
    of 4 and a ragged one"""
    csr = lex_ref.gpu_corpus()
    ix, ref = _index(csr)
    yield ix, ref, lex_ref.gpu_special_questions(csr) + lex_ref.gen_questions(7, 33)
    ix.close()


def _deep(ix, questions, k, **kw):
    s, r = ix.search_deep(lex_ref.question_csr(questions), k, **kw)
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy()


@pytest.mark.parametrize("k", [65, 128, 129, 1000, 1024])
def test_grid_matches_the_reference(corpus, k):
    """The near-tie rule leaves 0 of the 45 questions out of the row comparison at k <= 129 and 3 at k >= 1,000
    (the reference alone, on the CPU); at k >= 1,000 one question matches 269 rows only (padding)."""
    ix, ref, qs = corpus
    assert len(qs) == 45
    gs, gr = _deep(ix, qs, k)
    skipped = lex_ref.compare_topk(gs, gr, ref, qs, k)
    print(f"k {k}: {skipped} of 45 questions left out of the row comparison")
    assert skipped <= (0 if k <= 129 else 3), skipped
    s1, r1 = _deep(ix, qs[:1], k)  # a lone question: the one-question kernel
    lex_ref.compare_topk(s1, r1, ref, qs[:1], k)
    assert np.array_equal(s1[0], gs[0]) and np.array_equal(r1[0], gr[0])


def test_first_64_are_the_shallow_search_bit_for_bit(corpus):
    _, _, qs = corpus
    ix, _ = _index(lex_ref.gpu_corpus())  # an index of its own: it tombstones
    try:
        csr = lex_ref.question_csr(qs)
        ix.tombstone(np.unique(ix.search(csr, 8)[1].cpu().numpy()[:, :3].clip(0)))
        mask = torch.from_numpy(lex_ref.gpu_mask_words()[0].view(np.int32)).cuda()
        for m in (None, mask):
            for k in (65, 1024):
                ds, dr = ix.search_deep(csr, k, row_mask=m)
                ss, sr = ix.search(csr, 64, row_mask=m)
                assert torch.equal(ds[:, :64].contiguous().view(torch.int32), ss.view(torch.int32)), (m is None, k)
                assert torch.equal(dr[:, :64], sr), (m is None, k)
    finally:
        ix.close()


@pytest.mark.parametrize("blocks", ["1", "3"])
@pytest.mark.parametrize("reverse", [False, True])
def test_cuts_when_every_row_beats_the_threshold(monkeypatch, blocks, reverse):
    """3,000 rows of equal length whose score ascends with the row in ties of four (tf = 1 + r // 4 in the
    question's bucket): every row a workgroup meets beats its threshold, so its buffers fill and are cut at the
    fastest rate there is; and the same corpus reversed.  Distinct tf give well separated scores: exact rows."""
    monkeypatch.setenv("RFX_LEX_DEEP_BLOCKS", blocks)
    n = 3000
    tf = 1 + np.arange(n) // 4
    if reverse:
        tf = tf[::-1]
    bucket = np.tile(np.array([7, 9], np.int32), n)
    count = np.stack([tf, 800 - tf], 1).reshape(-1).astype(np.int16)  # the filler bucket: every len is 800
    ix, ref = _index((np.arange(n + 1, dtype=np.int32) * 2, bucket, count), 64)
    try:
        q = [([7], [1])]
        for k in (65, 1024):
            assert not ref.topk(q[0][0], q[0][1], k)[2]
            gs, gr = _deep(ix, q, k)
            assert lex_ref.compare_topk(gs, gr, ref, q, k) == 0
    finally:
        ix.close()


def test_small_store_and_a_question_without_a_match():
    csr = lex_ref.gen_csr(3, 33, V=256, lengths=6, skew=1.0)
    ix, ref = _index(csr, 256)
    try:
        absent = int(np.nonzero(ref.stats()[1] == 0)[0][0])
        qs = [(csr[1][:4], [1, 1, 1, 1]), ([absent], [1]), (csr[1][-3:], [2, 1, 1])]
        gs, gr = _deep(ix, qs, 65)
        assert lex_ref.compare_topk(gs, gr, ref, qs, 65) == 0
        assert np.all(gr[1] == -1) and np.all(np.isneginf(gs[1]))
    finally:
        ix.close()


def test_refused_arguments_leave_the_outputs_untouched(corpus):
    ix, _, qs = corpus
    csr = lex_ref.question_csr(qs[:2])
    for k, ws in ((64, None), (1025, None), (128, torch.empty(ix.deep_workspace_bytes(2, 128) - 256, dtype=torch.uint8,
                                                                 device="cuda"))):
        out = (torch.full((2, k), 7.0, dtype=torch.float32, device="cuda"),
               torch.full((2, k), 7, dtype=torch.int64, device="cuda"))
        with pytest.raises(ValueError):
            ix.search_deep(csr, k, out=out, workspace=ws)
        torch.cuda.synchronize()
        assert bool(torch.all(out[0] == 7)) and bool(torch.all(out[1] == 7))
