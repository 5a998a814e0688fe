"""GPU: kernel 11 (k_screen_valu.hip / k_screen_valu64.hip) at every top_k from 1 to 64:
lists of 16 with the exact plan's K slot 4 behind them (k <= 4), lists of 64 (17 <= k <= 64).

Bars (as tests/test_gpu_screen_valu.py): every search returns oracle/search.py's brute-force top-k under
check_topk (rows identical outside the 2e-6 tie band, no duplicates, scores within 1e-5 of the f64 score);
the forced fallback (screen mode 2) and the exact scan (screen off) return the same rows."""
import numpy as np
import pytest
import torch

from oracle import search as osearch
from oracle import synth as osynth

pytestmark = pytest.mark.gpu

TOL, TIE = 1e-5, 2e-6
KS = (1, 2, 4, 17, 32, 33, 63, 64)
NQS = (1, 2, 4, 8)
STORES = [("f32", 768), ("bf16", 768), ("f16", 768), ("bf16", 1024)]


@pytest.fixture(scope="module")
def rindex():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rfx.index as ri
    return ri


def _widen(stored, dtype):
    return osynth.to_f64(stored, dtype).astype(np.float32)


def _make(rindex, n, d, dtype, seed=31, screen=1):
    ix = rindex.DeviceIndex(d, dtype)
    ix.add_synthetic(seed, n)
    if screen:
        ix.enable_screen(screen)
    return ix, _widen(osynth.synth_rows(seed, 0, n, d, dtype), dtype)


def _queries(rindex, nq, d, dtype, seed=32):
    return rindex.synth_rows(seed, 0, nq, d, dtype), _widen(osynth.synth_rows(seed, 0, nq, d, dtype), dtype)


def _check(ix, rows32, q, q32, k, row_mask=None, allowed=None, stream=None):
    s, r = ix.search(q, k, row_mask=row_mask) if stream is None else ix.search(q, k, stream=stream)
    torch.cuda.synchronize()
    return _verify(s, r, rows32, q32, k, allowed)


def _verify(s, r, rows32, q32, k, allowed=None):
    s, r = s.cpu().numpy(), r.cpu().numpy()
    rows64 = rows32.astype(np.float64)
    if allowed is not None:
        rows64 = rows64.copy()
        rows64[~allowed] = np.nan
    q64 = q32.astype(np.float64)
    ref_s, ref_r = osearch.topk(q64, rows64, k)
    probs = osearch.check_topk(s, r, ref_s, ref_r, lambda qi, rr: rows64[rr] @ q64[qi], tol=TOL, tie_band=TIE)
    assert not probs, probs[:5]
    return s, r


@pytest.fixture(scope="module")
def stores30k(rindex):
    """The 30,000-row screened stores of cases 1 and 2, built once."""
    made = {}

    def get(dtype, d):
        if (dtype, d) not in made:
            made[(dtype, d)] = _make(rindex, 30000, d, dtype)
        return made[(dtype, d)]
    return get


# ---- 1. plan ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", STORES)
def test_plan_is_kernel11_at_every_k(rindex, dtype, d):
    ix = rindex.DeviceIndex(d, dtype)
    ix.add_synthetic(31, 30000)
    before = {(nq, k): ix.workspace_bytes(nq, k) for nq in NQS for k in (1, 4, 17, 64)}
    for nq in NQS:
        for k in KS:
            assert ix.search_plan(nq, k) == 0, (nq, k)
    ix.enable_screen(1)
    for nq in NQS:
        for k in KS:
            assert ix.search_plan(nq, k) == 11, (nq, k, ix.search_plan(nq, k))
    # a workspace sized before enable_screen fits afterwards
    assert before == {(nq, k): ix.workspace_bytes(nq, k) for nq in NQS for k in (1, 4, 17, 64)}
    ix.enable_screen(0)
    for nq in NQS:
        for k in KS:
            assert ix.search_plan(nq, k) == 0, (nq, k)
    ix.close()


# ---- 2. oracle parity, kept-score path (30,000 rows: 32 rows per wave) ----------------------------
GRID = [("bf16", 768, nq, k) for nq in NQS for k in KS]
GRID += [(dt, d, nq, k) for dt, d in STORES if (dt, d) != ("bf16", 768) for nq, k in ((1, 1), (2, 4), (4, 17), (8, 64))]


@pytest.mark.parametrize("dtype,d,nq,k", GRID)
def test_kept_score_path_matches_oracle(rindex, stores30k, dtype, d, nq, k):
    ix, rows32 = stores30k(dtype, d)
    assert ix.search_plan(nq, k) == 11
    q, q32 = _queries(rindex, nq, d, dtype)
    _check(ix, rows32, q, q32, k)


# ---- 3. sorted-list path (200,000 rows: ~200 rows per wave) ---------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_sorted_list_path_and_ties_past_a_wave_list(rindex, dtype):
    ix, rows32 = _make(rindex, 200_000, 768, dtype)
    cases = ((1, 64), (8, 32), (3, 1))
    qs = {nq: _queries(rindex, nq, 768, dtype, seed=7) for nq, _ in cases}
    for nq, k in cases:
        assert ix.search_plan(nq, k) == 11
        _check(ix, rows32, *qs[nq], k)
    top = int(osearch.topk(qs[1][1][:1].astype(np.float64), rows32.astype(np.float64), 1)[1][0, 0])
    first = ix.add(ix.read(top, 1).repeat(80, 1))  # 80 copies of query 0's winner: more than a list of 64 holds
    rows32 = np.concatenate([rows32, np.repeat(rows32[top:top + 1], 80, axis=0)])
    for nq, k in cases:
        s, r = _check(ix, rows32, *qs[nq], k)
        if k > 1:  # ties ordered by row: the winner, then its copies in row order
            assert r[0, 0] == top and list(r[0, 1:k]) == list(range(first, first + k - 1))
    ix.close()


# ---- 4. fallbacks agree ---------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 4])
def test_fallbacks_and_exact_agree(rindex, nq):
    ix, rows32 = _make(rindex, 40000, 768, "f32")
    q, q32 = _queries(rindex, nq, 768, "f32")
    for k in (1, 4, 64):
        got = {}
        for mode in (1, 2, 0, 1):  # the screen, every search forced to the fallback, exact, the screen again
            ix.enable_screen(mode)
            assert ix.search_plan(nq, k) == (11 if mode else 0)
            s, r = _check(ix, rows32, q, q32, k)
            got.setdefault(mode, []).append((s, r))
        for mode in (1, 2):
            for s, r in got[mode]:
                assert np.array_equal(r, got[0][0][1]), (k, mode)
    ix.close()


# ---- 5. edges -------------------------------------------------------------------------------------
def test_k_larger_than_live_rows(rindex):
    ix, rows32 = _make(rindex, 100, 768, "f32", seed=41)
    dead = list(range(3, 73))
    ix.tombstone(dead)
    rows32[dead] = np.nan
    q, q32 = _queries(rindex, 2, 768, "f32")
    for nq in (1, 2):
        assert ix.search_plan(nq, 64) == 11
        s, r = _check(ix, rows32, q[:nq].contiguous(), q32[:nq], 64)
        assert (r[:, 30:] == -1).all() and np.isneginf(s[:, 30:]).all() and (r[:, :30] >= 0).all()
    ix.close()
    ix, rows32 = _make(rindex, 33, 768, "bf16", seed=42)  # two tiles, the second nearly empty
    q, q32 = _queries(rindex, 1, 768, "bf16")
    s, r = _check(ix, rows32, q, q32, 64)
    assert (r[0, 33:] == -1).all() and np.isneginf(s[0, 33:]).all() and sorted(r[0, :33]) == list(range(33))
    ix.close()


def _mask(allowed):
    words = np.zeros((allowed.shape[0] + 31) // 32, dtype=np.uint32)
    for i in np.nonzero(allowed)[0]:
        words[i >> 5] |= np.uint32(1 << (i & 31))
    return torch.from_numpy(words.view(np.int32)).cuda()


def test_masks_and_tombstones(rindex):
    ix, rows32 = _make(rindex, 20000, 768, "bf16")
    q, q32 = _queries(rindex, 2, 768, "bf16")
    rng = np.random.default_rng(5)
    allowed = rng.random(20000) < 0.01
    _check(ix, rows32, q, q32, 32, row_mask=_mask(allowed), allowed=allowed)
    few = np.zeros(20000, dtype=bool)
    few[[7, 4000, 19999]] = True  # fewer than k rows allowed
    for k in (4, 32):
        s, r = _check(ix, rows32, q[:1].contiguous(), q32[:1], k, row_mask=_mask(few), allowed=few)
        assert sorted(r[0, :3]) == [7, 4000, 19999] and (r[0, 3:] == -1).all() and np.isneginf(s[0, 3:]).all()
    for k in (1, 64):  # the top hit tombstoned
        top = int(osearch.topk(q32[:1].astype(np.float64), rows32.astype(np.float64), 1)[1][0, 0])
        ix.tombstone([top])
        rows32[top] = np.nan
        s, r = _check(ix, rows32, q[:1].contiguous(), q32[:1], k)
        assert top not in r[0]
    ix.close()


# ---- 6. records path (a sharded store's shards) ---------------------------------------------------
def test_two_logical_shards_equal_unsharded(rindex):
    from rfx.sharded import ShardedIndex
    n = 40000
    whole, _ = _make(rindex, n, 768, "bf16", seed=61)
    sh = ShardedIndex(768, "bf16", [0, 0])
    cuts = sh._cuts(n)
    for i, s in enumerate(sh.shards):
        s.add_synthetic(61, cuts[i + 1] - cuts[i], gen_row0=cuts[i])
        sh.bases[i] = cuts[i]
    sh._split = True
    sh.enable_screen(1)
    q, _ = _queries(rindex, 8, 768, "bf16", seed=62)
    for k in (3, 40):
        for nq in (1, 8):
            assert all(s.search_plan(nq, k) == 11 for s in sh.shards) and whole.search_plan(nq, k) == 11
            a = whole.search(q[:nq].contiguous(), k)
            b = sh.search(q[:nq].contiguous(), k)
            assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0]), (nq, k)
    whole.close()


# ---- 7. two streams -------------------------------------------------------------------------------
def test_k32_from_two_streams(rindex):
    ix_a, rows_a = _make(rindex, 60000, 768, "f32", seed=51)
    ix_b, rows_b = _make(rindex, 50000, 768, "bf16", seed=52)
    q, q32 = _queries(rindex, 8, 768, "f32", seed=53)
    qb, qb32 = _queries(rindex, 8, 768, "bf16", seed=54)
    side = torch.cuda.Stream()
    outs = []
    for mode in (1, 2):
        ix_a.enable_screen(mode)
        ix_b.enable_screen(mode)
        assert ix_a.search_plan(1, 32) == 11 and ix_b.search_plan(1, 32) == 11
        for i in range(8):
            a = ix_a.search(q[i:i + 1].contiguous(), 32)
            with torch.cuda.stream(side):
                b = ix_b.search(qb[i:i + 1].contiguous(), 32, stream=side)
            outs.append((i, a, b))
    torch.cuda.synchronize()
    for i, a, b in outs:
        _verify(a[0], a[1], rows_a, q32[i:i + 1], 32)
        _verify(b[0], b[1], rows_b, qb32[i:i + 1], 32)
    ix_a.close()
    ix_b.close()


# ---- 8. adapter -----------------------------------------------------------------------------------
def test_adapter_top_k_3_and_32_reach_kernel11(tmp_path, monkeypatch):
    from rfx import store as rstore
    from rfx.adapter import LocalGpuRag
    from rfx.retriever import GpuRetriever

    words = [f"w{i:04d}" for i in range(1600)]
    text = " ".join(words)
    root = str(tmp_path)
    monkeypatch.setenv("RFX_SCREEN", "1")
    ret = GpuRetriever(registry=rstore.StoreRegistry(root=root, device=0), dtype="bf16")
    name = ret.create_store("topk")
    ret.add_document(name, text, "doc0", {"white_space_config": {"max_tokens_per_chunk": 4, "max_overlap_tokens": 0}}, {})
    ix = ret.registry.get(name).index
    assert ix.rows >= 300 and ix.search_plan(1, 3) == 11 and ix.search_plan(1, 32) == 11

    def cites(retr, k):
        rag = LocalGpuRag(retr, top_k=5)
        chunks = list(rag.ask_stream(contents=[{"role": "user", "parts": [{"text": "w0007 w0100 w1234 w0042"}]}],
                                     store_names=[name], metadata_filter=None, model="m", top_k=k))
        return [(c["index"], c["snippet"]) for c in rag.extract_citations_from_response(chunks[-1])]

    on = {k: cites(ret, k) for k in (3, 32)}
    monkeypatch.setenv("RFX_SCREEN", "0")
    plain = GpuRetriever(registry=rstore.StoreRegistry(root=root, device=0), dtype="bf16")
    assert plain.registry.get(name).index.search_plan(1, 3) == 0
    for k in (3, 32):
        assert len(on[k]) == k and on[k] == cites(plain, k)
