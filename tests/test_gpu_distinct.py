"""GPU: distinct-document search.  The collapse kernel alone (rfx_distinct_collapse) against the
numpy collapse of tests/distinct_ref.py, and DeviceIndex.search_distinct against the rule's CPU reference on
the corpora built to break it: rows and docs equal to the reference, scores bit-equal to the plain search's
for the same rows, and the rounds each corpus is constructed to take."""
import numpy as np
import pytest
import torch

import distinct_ref as ref

pytestmark = pytest.mark.gpu

_CACHE = {}


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda()


def corpus(name, d, dtype):
    """(Corpus, index, queries on the device, row_doc on the device): built once per (name, d, dtype)."""
    key = (name, d, dtype)
    if key not in _CACHE:
        from rfx import _lib
        from rfx.index import DeviceIndex
        c = ref.build(name, d)
        ix = DeviceIndex(d, dtype, 0)
        ix.add(dev(c.rows, _lib.TORCH_DTYPES[dtype]))
        if len(c.dead_rows):
            ix.tombstone(c.dead_rows)
        _CACHE[key] = (c, ix, dev(c.queries, _lib.TORCH_DTYPES[dtype]), dev(c.row_doc))
    return _CACHE[key]


def check(c, ix, q, got, rounds, want_rounds, allowed=None, row_mask=None):
    s, r, d, = (t.cpu().numpy() for t in got)
    want_s, want_r, want_d = ref.reference(c.q64, c.x64, c.row_doc, c.k, allowed)
    print(f"{c.name}: rounds {rounds} (constructed {want_rounds}); rows of question 0: {r[0].tolist()}")
    assert np.array_equal(r, want_r), (c.name, r[0], want_r[0])
    assert np.array_equal(d, want_d), c.name
    # scores: bit-equal to what the plain search gives the same rows
    plain_s, plain_r = (t.cpu().numpy() for t in ix.search(q, 64, row_mask=row_mask))
    full = {}
    for i in range(len(r)):
        full.update({(i, int(row)): sc for sc, row in zip(plain_s[i], plain_r[i]) if row >= 0})
    hit = 0
    for i in range(len(r)):
        for sc, row in zip(s[i], r[i]):
            if row < 0:
                assert sc == -np.inf
            elif (i, int(row)) in full:
                hit += 1
                assert np.float32(sc).tobytes() == np.float32(full[(i, int(row))]).tobytes(), (c.name, i, row)
    assert hit >= len(r), "every question's first hit is a row of the plain search"
    assert s.tobytes() == want_s.tobytes(), "and (exact corpora) the reference's scores bit for bit"
    assert rounds == want_rounds, (c.name, rounds, want_rounds)


# ---- the kernel alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 5, 257])
@pytest.mark.parametrize("n_cand,k", [(1, 1), (2, 1), (2, 10), (63, 10), (64, 10), (64, 64), (63, 64), (1, 64)])
def test_collapse_kernel(n_cand, k, nq):
    c, ix, _, row_doc = corpus("holes", 64, "f32")
    rows = len(c.rows)
    rng = np.random.default_rng(n_cand * 1000 + k * 10 + nq)
    # candidate rows drawn from a handful of files (many repeats of a document), with out-of-range rows and
    # padding mixed in; question 0 is all padding, question 1 (when there is one) all out of range
    pool = np.concatenate([np.arange(f0, f0 + n) for f0, n, _ in c.files[:9]])
    cr = rng.choice(pool, size=(nq, n_cand)).astype(np.int64)
    cr[rng.random((nq, n_cand)) < 0.1] = -1
    cr[rng.random((nq, n_cand)) < 0.05] = rows + 5
    cr[rng.random((nq, n_cand)) < 0.02] = np.iinfo(np.int64).max
    cr[0] = -1
    if nq > 1:
        cr[1] = rows
    cs = np.sort(rng.standard_normal((nq, n_cand)).astype(np.float32), axis=1)[:, ::-1].copy()
    for have in sorted({0, min(3, k - 1), k - 1}):
        # the picks an earlier round left: `have` documents no candidate may repeat, and junk above them
        out = (np.full((nq, k), 7.0, np.float32), np.full((nq, k), -9, np.int64), np.full((nq, k), -9, np.int32),
               np.full(nq, have, np.int32), np.zeros(nq, np.int32))
        live_docs = [o for o, f in enumerate(c.files) if not f[2]]
        for qi in range(nq):
            # (more picks than the corpus has live files: ordinals past its files too, which no candidate holds)
            docs = rng.choice(live_docs if have <= len(live_docs) else np.arange(100), size=have, replace=False)
            out[2][qi, :have] = docs
            out[1][qi, :have] = 1000 + docs
            out[0][qi, :have] = np.arange(have, 0, -1) + 10
        want = ref.collapse(cs, cr, c.row_doc, rows, k, out[3].copy(), tuple(a.copy() for a in out))
        g = tuple(dev(a) for a in out)
        got = ix.distinct_collapse(dev(cs), dev(cr), k, row_doc, have=g[3] if have else None, out=g if have else None)
        for name, a, b in zip(("scores", "rows", "docs", "n", "done"), got, want):
            a = a.cpu().numpy()  # (have 0 runs on fresh tensors: every slot is written)
            assert a.tobytes() == b.tobytes(), (name, have, a[:2], b[:2])
        if have:  # the earlier picks were left as they were
            assert np.array_equal(got[1].cpu().numpy()[:, :have], out[1][:, :have])
            assert np.array_equal(got[0].cpu().numpy()[:, :have], out[0][:, :have])
    assert int(got[3][0]) == min(have, k) and int(got[4][0]) == 1, "all padding: nothing added, and done"


def test_refused_arguments():
    from rfx import _lib
    from rfx._lib import lib, ptr, stream_ptr
    c, ix, q, row_doc = corpus("plain", 64, "f32")
    nq, n_cand, k = 4, 16, 8
    q = q[:nq].contiguous()
    cs, cr = ix.search(q, n_cand)
    o_s = torch.full((nq, 64), 123.0, dtype=torch.float32, device="cuda")
    o_r = torch.full((nq, 64), -77, dtype=torch.int64, device="cuda")
    o_d = torch.full((nq, 64), -77, dtype=torch.int32, device="cuda")
    o_n = torch.full((nq,), -77, dtype=torch.int32, device="cuda")
    o_done = torch.full((nq,), -77, dtype=torch.int32, device="cuda")
    P = dict(handle=ix.handle, row_doc=ptr(row_doc), n_row_doc=row_doc.numel(), nq=nq, n_cand=n_cand, k=k, cs=ptr(cs),
             cr=ptr(cr), have=None, o_s=ptr(o_s), o_r=ptr(o_r), o_d=ptr(o_d), o_n=ptr(o_n), o_done=ptr(o_done))

    def call(**kw):
        a = dict(P, **kw)
        return lib.rfx_distinct_collapse(a["handle"], a["row_doc"], a["n_row_doc"], a["nq"], a["n_cand"], a["k"],
                                         a["cs"], a["cr"], a["have"], a["o_s"], a["o_r"], a["o_d"], a["o_n"],
                                         a["o_done"], stream_ptr())

    def good():
        assert call() == _lib.RFX_OK
        torch.cuda.synchronize()
        want = ref.collapse(cs.cpu().numpy(), cr.cpu().numpy(), c.row_doc, len(c.rows), k)
        assert np.array_equal(o_r.view(-1)[:nq * k].cpu().numpy().reshape(nq, k), want[1])
        assert (o_r.view(-1)[nq * k:] == -77).all()
        assert np.array_equal(o_n.cpu().numpy(), want[3]) and np.array_equal(o_done.cpu().numpy(), want[4])

    bad = [dict(k=0), dict(k=65), dict(n_cand=0), dict(n_cand=65), dict(nq=0), dict(nq=1025),
           dict(n_row_doc=len(c.rows) - 1), dict(n_row_doc=0), dict(handle=0xdead), dict(row_doc=None), dict(cs=None),
           dict(cr=None), dict(o_s=None), dict(o_r=None), dict(o_d=None), dict(o_n=None), dict(o_done=None)]
    for kw in bad:
        for t in (o_r, o_d, o_n, o_done):
            t.fill_(-77)
        assert call(**kw) == _lib.RFX_EINVAL, kw
        torch.cuda.synchronize()
        assert (o_r == -77).all() and (o_n == -77).all() and (o_done == -77).all(), kw
        good()  # a good call on the same stream still answers
    with pytest.raises(ValueError):
        ix.search_distinct(q, 10, row_doc, c.doc_ranges, fetch_k=9)
    with pytest.raises(ValueError):
        ix.search_distinct(q, 10, row_doc, c.doc_ranges, fetch_k=65)


# ---- search_distinct against the rule ----------------------------------------------------------------------------
@pytest.mark.parametrize("d,dtype", [(64, "f32"), (64, "bf16"), (256, "f16"), (256, "bf16"), (256, "f32")])
@pytest.mark.parametrize("name", ref.CORPORA)
def test_search_distinct(name, d, dtype):
    c, ix, q, row_doc = corpus(name, d, dtype)
    s, r, docs, rounds = ix.search_distinct(q, c.k, row_doc, c.doc_ranges, fetch_k=c.fetch_k)
    check(c, ix, q, (s, r, docs), rounds, c.rounds)


def test_fetch_k_changes_the_rounds_not_the_answer():
    c, ix, q, row_doc = corpus("dominant2", 256, "bf16")
    base = ix.search_distinct(q, c.k, row_doc, c.doc_ranges)
    for fetch_k in (c.k, 64):
        got = ix.search_distinct(q, c.k, row_doc, c.doc_ranges, fetch_k=fetch_k)
        assert all(torch.equal(a, b) for a, b in zip(got[:3], base[:3])) and got[3] == base[3] == 3
    # a lone question, and a batch larger than a block of the collapse
    one = ix.search_distinct(q[2:3], c.k, row_doc, c.doc_ranges)
    assert torch.equal(one[1][0], base[1][2]) and torch.equal(one[0][0], base[0][2])
    many = ix.search_distinct(q.repeat(13, 1), c.k, row_doc, c.doc_ranges)
    assert torch.equal(many[1], base[1].repeat(13, 1)) and many[3] == 3


@pytest.mark.parametrize("nq,kernel", [(1, 11), (5, 11)])
def test_round_one_is_the_two_pass_scan(nq, kernel):
    """The two-pass scan needs d 768 or 1024, so this case leaves the small dims of the others."""
    c, ix, q, row_doc = corpus("dominant", 768, "bf16")
    ix.enable_screen(1)
    try:
        assert ix.search_plan(nq, 20) == kernel
        s, r, docs, rounds = ix.search_distinct(q[:nq], c.k, row_doc, c.doc_ranges)
    finally:
        ix.enable_screen(0)
    want = ref.reference(c.q64[:nq], c.x64, c.row_doc, c.k)
    assert np.array_equal(r.cpu().numpy(), want[1]) and np.array_equal(docs.cpu().numpy(), want[2])
    assert s.cpu().numpy().tobytes() == want[0].tobytes() and rounds == 2


@pytest.mark.parametrize("name", ["dominant", "dups", "holes"])
@pytest.mark.parametrize("refuse", [False, True])
def test_under_a_row_mask(name, refuse, monkeypatch):
    """A filter: the row mask in round 1, the same selection as ranges in the completion; and the masked
    fallback when the segmented search is made to refuse the shape."""
    from rfx import _lib, filters
    from rfx.index import DeviceIndex
    c, ix, q, row_doc = corpus(name, 64, "bf16")
    keep = [o for o, f in enumerate(c.files) if o % 3 != 2 and not f[2]]
    sel = filters.subtract_ranges([(0, len(c.rows))], [(f0, n) for o, (f0, n, _) in enumerate(c.files) if o not in keep])
    allowed = ref._allowed(len(c.rows), sel)
    mask = ix.mask_tensor(filters.row_mask_words(len(c.rows), sel))
    calls = []
    if refuse:
        def refused(self, *a, **kw):
            calls.append("segmented")
            raise _lib.RfxError(_lib.RFX_EUNSUPPORTED, "segmented scan: refused for the test")
        monkeypatch.setattr(DeviceIndex, "search_segmented", refused)
    s, r, docs, rounds = ix.search_distinct(q, c.k, row_doc, c.doc_ranges, fetch_k=c.fetch_k, row_mask=mask,
                                            select_ranges=sel)
    # dominant: the big file is selected and owns the best rows, the four small files left fit one completion;
    # dups: Z and A fill the best 64 selected rows, D and the small files fit one completion; holes: one round
    # exactly when the best fetch_k selected rows hold k files
    from rfx import distinct
    fetch = c.fetch_k or distinct.default_fetch_k(c.k)
    want_rounds = 2 if name != "holes" else (1 if min(c.files_in_best(fetch, allowed)) >= c.k else rounds)
    assert name != "holes" or want_rounds == 1 or rounds > 1
    check(c, ix, q, (s, r, docs), rounds, want_rounds, allowed=allowed, row_mask=mask)
    assert set(docs.cpu().numpy().ravel().tolist()) <= set(keep) | {-1}
    assert bool(calls) == (refuse and rounds > 1)
