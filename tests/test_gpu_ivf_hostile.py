"""GPU parity of the IVF-Flat int8 path on the hostile corpora of tests/hostile_ivf.py against
oracle/ivf.py: equal scores cut by the row id, +0.0 and -0.0 side by side, row scales 2^200 apart, planted list
lengths around every chunk edge, duplicate centroids, 1 / 2 / 4 list splits at every list template.  The bar is
BIT-EXACT everywhere — rows equal, scores equal as uint32, the sign of zero included — except the f32 re-rank,
which keeps check_topk's bars scaled by hostile.scale_bound.  tests/test_ivf_hostile_oracle.py holds the corpora
to their promises on the CPU."""
import numpy as np
import pytest
import torch

import hostile
import hostile_ivf as hi
from oracle import ivf as oivf
from oracle import search as osearch

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
_corpora, _indexes = {}, {}


@pytest.fixture(scope="module")
def rivf():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rfx.ivf as rivf
    yield rivf
    for ix in _indexes.values():
        ix.close()
    _indexes.clear()


def corpus(name, dtype="bf16"):
    if (name, dtype) not in _corpora:
        c = getattr(hi, name)(dtype)
        c.rows.setflags(write=False)
        _corpora[name, dtype] = c
    return _corpora[name, dtype]


def up(x, dtype):
    """Stored f32 values -> a device tensor of `dtype` (exact: the values are representable)."""
    t = torch.from_numpy(np.array(x, dtype=np.float32)).to(TORCH[dtype])  # (a copy: the corpora are read-only)
    assert np.array_equal(t.to(torch.float32).numpy(), x)
    return t.cuda()


def index_of(rivf, c):
    """The corpus in an index under its planted centroid table (built once per module)."""
    if (c.name, c.dtype) not in _indexes:
        ix = rivf.IvfIndex(c.rows.shape[1], c.nlist)
        ix.set_centroids(torch.from_numpy(c.qc).cuda())
        ix.add(up(c.rows, c.dtype))
        _indexes[c.name, c.dtype] = ix
    return _indexes[c.name, c.dtype]


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def assert_same(s, r, ref_s, ref_r, what):
    s, r = s.cpu().numpy(), r.cpu().numpy()
    bad = np.flatnonzero((r != ref_r).any(axis=1) | (s.view(np.uint32) != ref_s.view(np.uint32)).any(axis=1))
    if bad.size:
        i = bad[0]
        j = np.flatnonzero((r[i] != ref_r[i]) | (s[i].view(np.uint32) != ref_s[i].view(np.uint32)))[0]
        pytest.fail(f"{what}: {bad.size} of {len(r)} queries differ; query {i} from place {j}: rows "
                    f"{r[i][j:j + 6].tolist()} scores {s[i][j:j + 6].tolist()}, oracle rows "
                    f"{ref_r[i][j:j + 6].tolist()} scores {ref_s[i][j:j + 6].tolist()}")


# ---- quantise ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("scales", "f32"), ("scales", "bf16"), ("scales", "f16"),
                                        ("subscale", "f32"), ("subscale", "bf16")])
def test_quantize(rivf, name, dtype):
    c = corpus(name, dtype)
    codes, inv = rivf.quantize(up(c.rows, dtype))
    ref_c, ref_inv = oivf.quantize(c.rows)
    gc, gi = codes.cpu().numpy(), inv.cpu().numpy()
    bad = np.flatnonzero((gc != ref_c).any(axis=1) | (gi.view(np.uint32) != ref_inv.view(np.uint32)))
    if bad.size:
        i = bad[0]
        pytest.fail(f"{bad.size} rows differ; row {i} (amax {np.abs(c.rows[i]).max()!r}): inv {gi[i]!r} vs {ref_inv[i]!r}, "
                    f"codes min {gc[i].min()} max {gc[i].max()} vs min {ref_c[i].min()} max {ref_c[i].max()}")
    if name == "subscale":
        assert not gc[c.notes["sub"]].any() and (gi[c.notes["sub"]] == 0).all()
    else:
        assert not gc[c.notes["zero_rows"]].any() and (gi[c.notes["zero_rows"]] == 0).all()


# ---- assign and lists --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges", "skew", "dup_centroids"])
def test_assign_and_lists(rivf, name):
    c = corpus(name)
    codes, inv, lab, fc = c.quantized()
    ix = index_of(rivf, c)
    gqc, gfc = ix.centroids()
    assert np.array_equal(gqc.cpu().numpy(), c.qc) and np.array_equal(bits(gfc), fc.view(np.uint32))
    gc, ginv, glab = ix.codes()
    assert np.array_equal(gc.cpu().numpy(), codes) and np.array_equal(bits(ginv), inv.view(np.uint32))
    glab = glab.cpu().numpy()
    assert np.array_equal(glab, lab), f"{(glab != lab).sum()} labels differ, first at row {np.flatnonzero(glab != lab)[:5]}"
    off, ids = ix.lists()
    order, ref_off = oivf.build_lists(lab, c.nlist)
    assert np.array_equal(off.cpu().numpy(), ref_off) and np.array_equal(ids.cpu().numpy(), order)


# ---- train -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 3])
def test_train_equal_initial_centroids(rivf, iters):
    c = corpus("dup_sample")
    nlist, step = c.notes["nlist"], c.notes["step"]
    x = up(c.rows, c.dtype)
    ix = rivf.IvfIndex(c.rows.shape[1], nlist)
    ix.train(x, iters=iters)
    ix.add(x)
    xq = oivf.quantize(c.rows)[0]
    qc, fc = oivf.train(xq, nlist, iters)
    gqc, gfc = ix.centroids()
    assert np.array_equal(gqc.cpu().numpy(), qc), "k-means centroids differ"
    assert np.array_equal(bits(gfc), fc.view(np.uint32))
    assert np.array_equal(gqc.cpu().numpy()[2], xq[2 * step])  # the empty list's centroid is its initial row still
    assert np.array_equal(ix.codes()[2].cpu().numpy(), oivf.assign(xq, qc, fc))
    ix.close()


# ---- search ------------------------------------------------------------------------------------------------
FULL = 0  # nprobe: every list (capped at 64)
# (splits, k, nq, nprobe): every value of each axis once per corpus
BASE = [(1, 1, 1, 1), (2, 4, 9, 3), (4, 5, 33, FULL), (1, 16, 33, 3), (2, 17, 1, FULL), (4, 64, 9, 1)]
EXTRA = {
    ("edges", "law"): [(1, 64, 33, 1)],                                        # lists of 1 .. 3 rows: the padded tail
    ("dups", "law"): [(4, 64, 33, 3), (1, 64, 33, 3), (2, 16, 33, 3), (1, 4, 33, 3)],
    ("scales", "tiny"): [(1, 64, 33, 3), (4, 64, 33, 3), (2, 16, 33, FULL), (1, 4, 33, 3)],
}
SEARCH = [(n, q) + case for n, q in [("edges", "law"), ("skew", "law"), ("dups", "law"), ("neg", "neg"),
                                     ("scales", "unit"), ("scales", "tiny"), ("scales", "zero")]
          for case in BASE + EXTRA.get((n, q), [])]


@pytest.mark.parametrize("name,qset,splits,k,nq,nprobe", SEARCH)
def test_search(rivf, monkeypatch, name, qset, splits, k, nq, nprobe):
    c = corpus(name)
    codes, inv, lab, fc = c.quantized()
    ix = index_of(rivf, c)
    nprobe = nprobe or min(c.nlist, 64)
    q = c.queries[qset][:nq]
    qdt = c.notes.get("tiny_dtype", c.dtype) if qset == "tiny" else c.dtype
    monkeypatch.setenv("RFX_IVF_SPLITS", str(splits))
    s, r = ix.search(up(q, qdt), k, nprobe)
    qq, qinv = oivf.quantize(q)
    ref_s, ref_r = oivf.search(qq, qinv, codes, inv, lab, c.qc, fc, nprobe, k)
    assert_same(s, r, ref_s, ref_r, f"{name}/{qset} splits {splits} k {k} nq {nq} nprobe {nprobe}")
    if (name, k, nq, nprobe) == ("edges", 64, 33, 1):
        tail = ref_r == -1
        assert tail.any() and (r.cpu().numpy()[tail] == -1).all() and np.isneginf(s.cpu().numpy()[tail]).all()
    if qset == "zero":  # the answer is known outright: the lowest row ids of lists 0 .. nprobe-1, all +0.0
        want = np.flatnonzero(lab < nprobe)[:k]
        assert (r.cpu().numpy()[:, :len(want)] == want).all() and not bits(s)[:, :len(want)].any()


def test_search_cases_cover_every_value():
    for n, q in {(c[0], c[1]) for c in SEARCH}:
        mine = [c[2:] for c in SEARCH if c[:2] == (n, q)]
        assert {m[0] for m in mine} == {1, 2, 4} and {m[1] for m in mine} == {1, 4, 5, 16, 17, 64}
        assert {m[2] for m in mine} == {1, 9, 33} and {m[3] for m in mine} == {1, 3, FULL}
    assert ("dups", "law", 4, 64, 33, 3) in SEARCH


# ---- probe selection ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nprobe", [1, 3, 64])
def test_probe_selection_duplicate_centroids(rivf, nprobe):
    c = corpus("dup_centroids")
    codes, inv, lab, fc = c.quantized()
    ix = index_of(rivf, c)
    q = np.concatenate([c.queries["law"], np.zeros((1, c.rows.shape[1]), np.float32)])  # the last one: all-zero
    qq, qinv = oivf.quantize(q)
    pr = oivf.probes(qq, c.qc, fc, nprobe)
    s, r = ix.search(up(q, c.dtype), 64, nprobe)
    ref_s, ref_r = oivf.search(qq, qinv, codes, inv, lab, c.qc, fc, nprobe, 64)
    assert_same(s, r, ref_s, ref_r, f"dup_centroids nprobe {nprobe}")
    r = r.cpu().numpy()
    losers = [b for _, b in c.notes["pairs"]]
    for i in range(len(q)):
        got = set(lab[r[i][r[i] >= 0]].tolist())
        assert got <= set(pr[i].tolist()), f"query {i} returned rows of lists {sorted(got - set(pr[i].tolist()))} not probed"
    if nprobe == 1:  # the tie on top: the higher id of a pair loses, and the winner's rows come back
        assert not np.isin(pr, losers).any()
        for j in range(len(c.notes["pairs"])):
            assert pr[2 * j, 0] == c.notes["pairs"][j][0] and (lab[r[2 * j][r[2 * j] >= 0]] == pr[2 * j, 0]).all()
            assert (r[2 * j] >= 0).any()
    assert pr[-1].tolist() == list(range(nprobe))  # the zero query: every coarse score +0.0, the lowest ids


# ---- nlist above the probe-selection kernel's 4096: the fallback probe merge ---------------------------
def test_nlist_4100(rivf):
    d, nlist, n, nprobe, k = 256, 4100, 6000, 8, 10
    rows = rivf.synth_clustered(7, 48, 5, 0, n, d, "bf16")
    ix = rivf.IvfIndex(d, nlist)
    ix.train(rows, iters=1)
    ix.add(rows)
    x = oivf.stored_to_f32(rows.cpu().view(torch.int16).numpy().view(np.uint16), "bf16")
    codes, inv = oivf.quantize(x)
    qc, fc = oivf.train(codes, nlist, 1)
    gqc, gfc = ix.centroids()
    assert np.array_equal(gqc.cpu().numpy(), qc) and np.array_equal(bits(gfc), fc.view(np.uint32))
    lab = oivf.assign(codes, qc, fc)
    assert np.array_equal(ix.codes()[2].cpu().numpy(), lab)
    q = rivf.synth_clustered(7, 48, 77, 0, 33, d, "bf16")
    qq, qinv = oivf.quantize(oivf.stored_to_f32(q.cpu().view(torch.int16).numpy().view(np.uint16), "bf16"))
    s, r = ix.search(q, k, nprobe)
    ref_s, ref_r = oivf.search(qq, qinv, codes, inv, lab, qc, fc, nprobe, k)
    assert_same(s, r, ref_s, ref_r, "nlist 4100")
    ix.close()


# ---- re-rank with padded candidates ----------------------------------------------------------------------
def test_search_rerank_padded_candidates(rivf):
    c = corpus("edges")
    ix = index_of(rivf, c)
    k, rk, nprobe = 10, 64, 1
    q = c.queries["law"]
    rows_t, q_t = up(c.rows, "f32"), up(q, c.dtype)
    s, r = ix.search_rerank(q_t, k, nprobe, rows_t, rerank_k=rk)
    _, cand = ix.search(q_t, rk, nprobe)
    cand = cand.cpu().numpy()
    assert (cand == -1).any() and ((cand >= 0).sum(axis=1) < k).any()  # padding among the candidates and in the answer
    rows64, q64 = c.rows.astype(np.float64), q.astype(np.float64)
    ref_s, ref_r = oivf.rerank(cand, q64, rows64, k)
    S = hostile.scale_bound(c.rows, q)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    probs = osearch.check_topk(s, r, ref_s, ref_r, lambda qi, rr: rows64[rr] @ q64[qi], tol=1e-5 * S, tie_band=2e-6 * S)
    assert not probs, probs[:5]
    assert np.array_equal(r == -1, ref_r == -1) and np.isneginf(s[r == -1]).all()
