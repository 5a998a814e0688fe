"""GPU parity of the metadata-filtered IVF search (rfx_ivf_search_masked / rfx_ivf_search_rerank_masked, DESIGN
§4.15) against tests/ivf_mask_ref.py: oracle/ivf.py called with the unselected rows' labels set to -1, so the
filter applies before the ranking.  Corpora: tests/hostile_ivf.py's edges (every chunk edge), skew (one 12,000-row
list: waves go past their two seed chunks) and dups (tied scores: the tie is cut by row id among the eligible rows
only).  Masks: all ones, all zero, alternating bits, word edges, the first / the last row of every list, file-like
ranges, every wave's seed chunks of the long list cleared, fewer than k eligible rows.  No corpus has a multiple
of 32 rows and the spare bits of the last mask word are SET.  The bar is BIT-EXACT (rows equal, scores equal as
uint32); for the f32 re-rank, rows equal to the wrapper followed by oracle.ivf.rerank on every query and scores
within 1e-5 of the f64 dot (the store test's tolerance), on cases chosen so that the reference decides every query's
rows beyond the f32 dot's own error bound (RERANK, decidable()).
tests/test_ivf_masked_ref.py shows on the CPU that a kernel ignoring the mask, or masking a finished top-k, fails
every case here but the all-ones and all-zero masks."""
import ctypes

import numpy as np
import pytest
import torch

import hostile
import hostile_ivf as hi
import ivf_mask_ref as mr
from oracle import ivf as oivf
from oracle import search as osearch

pytestmark = pytest.mark.gpu

_corpora, _indexes, _masks = {}, {}, {}


@pytest.fixture(scope="module")
def rivf():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rfx.ivf as rivf
    yield rivf
    for ix in _indexes.values():
        ix.close()
    _indexes.clear()
    _masks.clear()


def corpus(name):
    if name not in _corpora:
        c = getattr(hi, name)("bf16")
        c.rows.setflags(write=False)
        _corpora[name] = c
    return _corpora[name]


def up(x):
    t = torch.from_numpy(np.array(x, dtype=np.float32)).to(torch.bfloat16)
    assert np.array_equal(t.to(torch.float32).numpy(), x)
    return t.cuda()


def index_of(rivf, c):
    if c.name not in _indexes:
        ix = rivf.IvfIndex(c.rows.shape[1], c.nlist)
        ix.set_centroids(torch.from_numpy(c.qc).cuda())
        ix.add(up(c.rows))
        _indexes[c.name] = ix
    return _indexes[c.name]


def mask_of(c, name, splits=1):
    """(selection bool [n], device mask words with the spare bits set), built once per (corpus, mask)."""
    key = (c.name, name, splits if name == "seedless" else 1)
    if key not in _masks:
        sel = mr.selection(name, c.quantized()[2], splits)
        sel.setflags(write=False)
        _masks[key] = (sel, torch.from_numpy(mr.to_words(sel)).cuda())
    return _masks[key]


def assert_same(s, r, ref_s, ref_r, what):
    s, r = s.cpu().numpy(), r.cpu().numpy()
    bad = np.flatnonzero((r != ref_r).any(axis=1) | (s.view(np.uint32) != ref_s.view(np.uint32)).any(axis=1))
    if bad.size:
        i = bad[0]
        j = np.flatnonzero((r[i] != ref_r[i]) | (s[i].view(np.uint32) != ref_s[i].view(np.uint32)))[0]
        pytest.fail(f"{what}: {bad.size} of {len(r)} queries differ; query {i} from place {j}: rows "
                    f"{r[i][j:j + 6].tolist()} scores {s[i][j:j + 6].tolist()}, reference rows "
                    f"{ref_r[i][j:j + 6].tolist()} scores {ref_s[i][j:j + 6].tolist()}")


@pytest.mark.parametrize("name,mask,splits,k,nq,nprobe", mr.CASES)
def test_search_masked(rivf, monkeypatch, name, mask, splits, k, nq, nprobe):
    c = corpus(name)
    assert c.rows.shape[0] % 32, "the last mask word must have spare bits"
    codes, inv, lab, fc = c.quantized()
    ix = index_of(rivf, c)
    nprobe = nprobe or min(c.nlist, 64)
    q = c.queries["law"][:nq]
    sel, words = mask_of(c, mask, splits)
    monkeypatch.setenv("RFX_IVF_SPLITS", str(splits))
    s, r = ix.search(up(q), k, nprobe, row_mask=words)
    what = f"{name}/{mask} splits {splits} k {k} nq {nq} nprobe {nprobe}"
    qq, qinv = oivf.quantize(q)
    if mask == "ones":  # bit-identical to rfx_ivf_search (and so to the oracle)
        us, ur = ix.search(up(q), k, nprobe)
        assert_same(s, r, us.cpu().numpy(), ur.cpu().numpy(), what + " vs the unmasked call")
    ref_s, ref_r = mr.search(qq, qinv, codes, inv, lab, c.qc, fc, nprobe, k, sel)
    assert_same(s, r, ref_s, ref_r, what)
    if mask == "zeros":
        assert (r.cpu().numpy() == -1).all() and np.isneginf(s.cpu().numpy()).all()
    if mask == "few" and k > 3:
        assert (ref_r == -1).any()  # fewer than k eligible rows: the padded tail is part of the comparison above


def test_search_cases_cover_every_value():
    for n in mr.PLAN:
        mine = [c[2:] for c in mr.CASES if c[0] == n]
        assert {m[0] for m in mine} == {1, 2, 4} and {m[1] for m in mine} == {1, 4, 5, 16, 17, 64}
        assert {m[2] for m in mine} == {1, 9, 33} and {m[3] for m in mine} == {1, 3, mr.FULL}
        assert {c[1] for c in mr.CASES if c[0] == n} >= {"ones", "zeros", "alt", "wordedge", "first", "last", "ranges",
                                                        "few"}
    assert {corpus(n).rows.shape[1] for n in mr.PLAN} == {256, 768}
    assert {c[2] for c in mr.CASES if c[:2] == ("skew", "seedless")} == {1, 2, 4}


# The re-rank is f32, the reference f64: "rows equal" can be asked only of a query whose rows the reference decides
# beyond the f32 dot's own error (decidable, below).  The rows are bf16, so many f64 scores of a list's rows stand
# closer than that; the cases — mask, k, re-rank depth and the QUERIES of each corpus — are therefore chosen on the
# CPU, from the reference alone, so that every query of every case is decided (with twice the margin or more to
# spare), and the test asserts it before it compares.  All 33 queries where no list is given.  Queries 0, 14 and 28
# of skew are the ones aimed at its 12,000-row list.
RERANK = [
    ("edges", "alt", 5, 20, 3, [0, 3, 5, 6, 8, 10, 11, 12, 13, 15, 16, 17, 18, 19, 20, 23, 28, 29, 31, 32]),
    ("edges", "few", 10, 64, mr.FULL, None),
    ("dups", "wordedge", 5, 16, mr.FULL, None),
    ("skew", "ranges", 5, 64, 3, [2, 3, 7, 8, 10, 11, 12, 13, 18, 21, 22, 24, 25, 26, 27, 30]),
    ("skew", "seedless", 2, 64, 3, [0, 1, 2, 3, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 20, 21, 22, 23, 24, 26, 27,
                                    28, 29, 30, 31, 32]),
    ("skew", "wordedge", 5, 16, 3, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 17, 18, 19, 20, 21, 22, 23, 24,
                                    25, 26, 27, 28, 29, 30, 31, 32]),
]


@pytest.mark.parametrize("name,mask,k,rk,nprobe,queries", RERANK, ids=[f"{c[0]}-{c[1]}-k{c[2]}-rk{c[3]}" for c in RERANK])
def test_search_rerank_masked(rivf, name, mask, k, rk, nprobe, queries):
    c = corpus(name)
    codes, inv, lab, fc = c.quantized()
    ix = index_of(rivf, c)
    nprobe = nprobe or min(c.nlist, 64)
    q = c.queries["law"] if queries is None else c.queries["law"][queries]
    nq = len(q)
    sel, words = mask_of(c, mask)
    qq, qinv = oivf.quantize(q)
    _, cand = mr.search(qq, qinv, codes, inv, lab, c.qc, fc, nprobe, rk, sel)
    rows64, q64 = c.rows.astype(np.float64), q.astype(np.float64)
    ref_s, ref_r = oivf.rerank(cand, q64, rows64, k)
    S = hostile.scale_bound(c.rows, q)
    sure = decidable(cand, q64, rows64, k, 2 * (c.rows.shape[1] // 64 + 7) * 2.0 ** -24 * S)
    assert sure.all(), f"queries {np.flatnonzero(~sure).tolist()} do not decide their rows: pick other queries"
    s, r = ix.search_rerank(up(q), k, nprobe, up(c.rows), rerank_k=rk, row_mask=words)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    assert np.array_equal(r, ref_r), f"{(r != ref_r).any(axis=1).sum()} of {nq} queries differ in rows"
    assert sel[r[r >= 0]].all() and np.isneginf(s[r == -1]).all()
    for i in range(nq):
        ok = r[i] >= 0
        assert np.all(np.abs(s[i][ok] - rows64[r[i][ok]] @ q64[i]) <= 1e-5)
    # (an extra: the existing re-rank test's bar)
    probs = osearch.check_topk(s, r, ref_s, ref_r, lambda qi, rr: rows64[rr] @ q64[qi], tol=1e-5 * S, tie_band=2e-6 * S)
    assert not probs, probs[:5]
    if mask == "few":
        assert (r == -1).any()
    if name == "skew" and queries[0] == 0:  # the long list's own queries answer from the long list
        long_list = np.argmax(np.bincount(lab))
        assert (lab[r[0]] == long_list).all()


def decidable(cand, q64, rows64, k, margin):
    """bool [nq]: the queries whose rows the CPU reference decides for an f32 re-rank — among the query's k + 1
    best candidates, two f64 scores are either more than `margin` apart or belong to identical rows (whose f32
    scores are identical too, so the row id decides on both sides).  margin = twice the f32 dot's error bound:
    the re-rank kernel sums D / 64 fused multiply-adds per lane and six cross-lane adds, so a score is within
    (D / 64 + 7) 2^-24 |row| |query| of the exact dot (the inputs are exact: stored bf16 values), and no two
    scores further apart than twice that can swap."""
    out = np.ones(len(cand), dtype=bool)
    for i in range(len(cand)):
        rr = cand[i][cand[i] >= 0]
        sc = rows64[rr] @ q64[i]
        o = np.lexsort((rr, -sc))[:k + 1]
        for a, b in zip(o[:-1], o[1:]):
            if not (sc[a] - sc[b] > margin or np.array_equal(rows64[rr[a]], rows64[rr[b]])):
                out[i] = False
    return out


def _raw_search(ix, q, k, nprobe, mask_ptr, mask_words):
    from rfx._lib import lib, ptr, stream_ptr, DTYPE_CODES
    nq = q.shape[0]
    out_s = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    out_r = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    ws = torch.empty(max(ix.workspace_bytes(nq, k, nprobe), 1), dtype=torch.uint8, device="cuda")
    rc = lib.rfx_ivf_search_masked(ix.handle, ptr(q), nq, DTYPE_CODES["bf16"], k, nprobe, mask_ptr, mask_words,
                                   ptr(out_s), ptr(out_r), ptr(ws), ws.numel(), stream_ptr(None))
    torch.cuda.synchronize()
    return rc, out_s, out_r


def test_null_mask_and_short_mask(rivf):
    from rfx import _lib
    c = corpus("edges")
    ix = index_of(rivf, c)
    q = up(c.queries["law"][:9])
    n = c.rows.shape[0]
    us, ur = ix.search(q, 10, 3)
    rc, s, r = _raw_search(ix, q, 10, 3, ctypes.c_void_p(0), 0)  # NULL mask = the unmasked call, whatever mask_words
    assert rc == _lib.RFX_OK
    assert_same(s, r, us.cpu().numpy(), ur.cpu().numpy(), "NULL mask")
    sel, words = mask_of(c, "alt")
    need = (n + 31) // 32
    assert words.numel() == need
    rc, _, _ = _raw_search(ix, q, 10, 3, _lib.ptr(words), need - 1)
    assert rc == _lib.RFX_EINVAL and b"row mask" in _lib.lib.rfx_last_error()
    with pytest.raises(ValueError, match="row mask has"):  # (the binding raises RFX_EINVAL as ValueError)
        ix.search(q, 10, 3, row_mask=words[:need - 1].contiguous())
    with pytest.raises(ValueError, match="row mask has"):
        ix.search_rerank(q, 10, 3, up(c.rows), row_mask=words[:need - 1].contiguous())
    rc, s, r = _raw_search(ix, q, 10, 3, _lib.ptr(words), need)  # exactly enough words
    assert rc == _lib.RFX_OK
    ms, mrows = ix.search(q, 10, 3, row_mask=words)
    assert_same(s, r, ms.cpu().numpy(), mrows.cpu().numpy(), "raw call vs binding")


def test_sharded_filtered_store_equals_one_device(tmp_path, monkeypatch):
    """An IVF store read through 4 logical shards answers a filtered question from its lists (RFX_IVF_FILTERED=1)
    bit-identically to the same store on one device."""
    from rfx import ivf as rivf_
    from rfx import store as rstore
    from rfx.sharded import ShardedIndex, ShardedIvf

    dim, spec = 768, {"kind": "ivf", "nlist": 32, "nprobe": 8, "train_min": 4000}
    root = str(tmp_path)
    st = rstore.StoreRegistry(root=root, device=0).create("ivf-sh", dim, "bf16", spec=spec)
    docs = [rivf_.synth_clustered(7, 48, 200 + i, 1500 * i, 1500, dim, "bf16") for i in range(4)]
    fids = [st.add_document([f"d{i}-{j}" for j in range(1500)], v, f"d{i}.md", {"tenant": f"t{i % 2}"})[0]
            for i, v in enumerate(docs)]
    st.delete_file(fids[2])  # tenant t0 keeps rows 0 .. 1499, t1 rows 1500 .. 2999 and 4500 .. 5999
    st.add_document([f"e-{j}" for j in range(37)], rivf_.synth_clustered(7, 48, 300, 0, 37, dim, "bf16"), "e.md",
                    {"tenant": "t1"})  # 6,037 rows: not a multiple of 32
    assert st.ivf_ready()
    plain = rstore.StoreRegistry(root=root, device=0).get(st.name)
    shard = rstore.StoreRegistry(root=root, device=0, devices="0x4").get(st.name)
    assert isinstance(shard.index, ShardedIndex) and isinstance(shard.ivf, ShardedIvf)
    assert plain.ivf_ready() and shard.ivf_ready()
    monkeypatch.setenv("RFX_IVF_FILTERED", "1")
    q = rivf_.synth_clustered(7, 48, 999, 0, 33, dim, "bf16")
    for filt, lo_hi in (({"tenant": "t0"}, [(0, 1500)]), ({"tenant": "t1"}, [(1500, 3000), (4500, 6037)])):
        for k in (1, 10, 20):
            a_s, a_r, a_p = plain.search_filtered(q, k, filt)
            b_s, b_r, b_p = shard.search_filtered(q, k, filt)
            assert a_p == b_p == "ivf"
            assert np.array_equal(a_r.numpy(), b_r.numpy())
            assert np.array_equal(a_s.numpy().view(np.uint32), b_s.numpy().view(np.uint32))
            r = a_r.numpy()
            assert (r >= 0).all() and np.any([(r >= lo) & (r < hi) for lo, hi in lo_hi], axis=0).all()
