"""GPU parity of the segmented search (rfx_search_segmented): ONE launch answers questions under
different metadata filters, each over its own filter's row ranges only, and returns what the oracle returns
over those rows (everything else NaN, the tombstone rule) under the parity bars of test_gpu_filters.py;
its scores are bit-identical to the masked search's (one score rule).  Then the retriever: concurrent
questions of several tenants share one batch and one launch."""
import threading

import numpy as np
import pytest
import torch

from oracle import search as osearch
from oracle import synth as osynth

pytestmark = pytest.mark.gpu

TOL, TIE = 1e-5, 2e-6
N = 20_011  # ragged: no multiple of a chunk, a wave's share or a 64-row block
SEED, QSEED = 21, 22
FILES = [(0, 7), (31, 2), (1000, 337), (15_000, 5011)]
# tombstones inside the ranges below (whole small ranges too) and outside all of them
TOMBS = [3, 32, 1005, 1336, 15_000, 15_064, 20_010, 201, 220, 221, 500, 9000, 12_345]
# (name, queries, ranges): 1 / 8 / 9 / 40 queries cover the 8-query slice boundaries
GROUPS = [
    ("single row", 1, [(5000, 1)]),
    ("two ranges", 8, [(100, 900), (3000, 4000)]),
    ("everything", 9, [(0, N)]),
    ("files", 40, FILES),
    ("fewer live rows than k", 3, [(200, 3)]),       # 201 is tombstoned: 2 live rows
    ("only tombstoned rows", 2, [(220, 2)]),
    ("no range", 2, []),
]
NQ = sum(n for _, n, _ in GROUPS)
CASES = [(768, "bf16"), (1024, "f16"), (256, "f32")]


@pytest.fixture(scope="module")
def rindex():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rfx.index as rindex
    return rindex


def query_groups():
    """The groups with their query indices: a seeded shuffle of 0..NQ-1, so group order != caller order."""
    order = np.random.default_rng(7).permutation(NQ)
    out, at = [], 0
    for name, n, rngs in GROUPS:
        out.append((name, order[at:at + n].tolist(), rngs))
        at += n
    return out


def allowed_rows(rngs):
    a = np.zeros(N, dtype=bool)
    for first, count in rngs:
        a[first:first + count] = True
    return a


def mask_words(allowed):
    pad = np.zeros((N + 31) // 32 * 32, dtype=np.uint8)
    pad[:N] = allowed
    return np.packbits(pad, bitorder="little").view("<u4").view(np.int32)


_WORLD = {}


def world(rindex, dim, dtype):
    """Index, queries and the oracle's top-64 per group: built once per (dim, dtype) and shared by the k cases
    (the oracle's top-k is the first k of its top-64: one order, score desc / row asc)."""
    key = (dim, dtype)
    if key not in _WORLD:
        _WORLD.clear()  # one (dim, dtype) at a time: the f64 rows are large
        ix = rindex.DeviceIndex(dim, dtype)
        ix.add_synthetic(SEED, N)
        ix.tombstone(TOMBS)
        rows64 = osynth.to_f64(osynth.synth_rows(SEED, 0, N, dim, dtype), dtype)
        rows64[TOMBS] = np.nan
        q = rindex.synth_rows(QSEED, 0, NQ, dim, dtype)
        q64 = osynth.to_f64(osynth.synth_rows(QSEED, 0, NQ, dim, dtype), dtype)
        refs = []
        for name, qidx, rngs in query_groups():
            allowed = allowed_rows(rngs)
            ref_rows = np.where(allowed[:, None], rows64, np.nan)
            ref_s, ref_r = osearch.topk(q64[qidx], ref_rows, 64)
            # exact scores of this group's queries over its rows (for rows the GPU returns in another order)
            sc = q64[qidx] @ np.where(np.isnan(ref_rows), 0.0, ref_rows).T
            sc[:, np.isnan(ref_rows).any(axis=1)] = -np.inf
            refs.append((name, qidx, rngs, allowed, ref_s, ref_r, sc))
        _WORLD[key] = (ix, q, refs)
    return _WORLD[key]


def test_plan_covers_the_kernel_paths(rindex):
    """The call below has a group cut into several chunks and a chunk that spans several ranges."""
    gq = np.cumsum([0] + [n for _, n, _ in GROUPS])
    gr = np.cumsum([0] + [len(r) for _, _, r in GROUPS])
    flat = [v for _, _, rngs in GROUPS for fc in rngs for v in fc]
    items, lists = rindex.segmented_plan(N, 768, "bf16", NQ, 10, gq, gr, flat)
    assert 2 <= lists <= rindex.SEGMENT_LISTS
    chunks_of = lambda g: len({int(p) for gg, _, p, _ in items if gg == g})
    assert chunks_of(2) >= 2 and chunks_of(3) >= 2
    ends = np.cumsum([c for _, c in FILES])
    starts = ends - np.array([c for _, c in FILES])
    spanned = [int(((starts < p + n) & (ends > p)).sum()) for g, _, p, n in items if g == 3]
    assert max(spanned) >= 2
    assert not (items[:, 0] == 6).any()


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("dim,dtype", CASES)
def test_segmented_matches_oracle_and_masked(rindex, dim, dtype, k):
    ix, q, refs = world(rindex, dim, dtype)
    s, r = ix.search_segmented(q, k, [(qidx, rngs) for _, qidx, rngs, *_ in refs])
    torch.cuda.synchronize()
    s, r = s.cpu().numpy(), r.cpu().numpy()
    assert s.shape == (NQ, k) and r.shape == (NQ, k)
    for name, qidx, rngs, allowed, ref_s, ref_r, sc in refs:
        gs, gr = s[qidx], r[qidx]
        probs = osearch.check_topk(gs, gr, ref_s[:, :k], ref_r[:, :k], lambda qi, rows: sc[qi][rows], tol=TOL,
                                   tie_band=TIE)
        assert not probs, (name, probs[:5])
        live = gr[gr >= 0]
        assert allowed[live].all(), f"{name}: a row outside the group's ranges was returned"
        assert not np.isin(live, TOMBS).any(), f"{name}: a tombstoned row was returned"
        n_live = int(allowed.sum() - np.isin(TOMBS, np.nonzero(allowed)[0]).sum())
        assert ((gr >= 0).sum(axis=1) == min(k, n_live)).all(), name
        assert (gr[:, min(k, n_live):] == -1).all() and np.isneginf(gs[:, min(k, n_live):]).all(), name
        if not rngs:
            continue
        # one score rule: where the masked search returns the same row at the same place, the same bits
        m = torch.from_numpy(mask_words(allowed)).cuda()
        ms, mr = ix.search(q[qidx], k, row_mask=m)
        ms, mr = ms.cpu().numpy(), mr.cpu().numpy()
        same = (mr == gr) & (gr >= 0)
        assert same.any() or n_live == 0, name
        assert np.array_equal(ms[same].view(np.uint32), gs[same].view(np.uint32)), name


def test_validation_errors_leave_the_index_usable(rindex):
    ix = rindex.DeviceIndex(768, "bf16")
    ix.add_synthetic(1, 300)
    q = rindex.synth_rows(2, 0, 4, 768, "bf16")
    all4 = [0, 1, 2, 3]
    bad = [
        [(all4, [(50, 5), (10, 5)])],          # unsorted
        [(all4, [(10, 5), (14, 5)])],          # overlapping
        [(all4, [(296, 5)])],                  # past the end
        [(all4, [(300, 1)])],
        [(all4, [(-1, 2)])],
        [(all4, [(10, 0)])],                   # count <= 0
        [(all4, [(10, -1)])],
        [([0, 1], [(0, 10)])],                 # not every query in a group
        [([0, 1, 2, 3, 3], [(0, 10)])],
    ]
    for groups in bad:
        with pytest.raises(ValueError):
            ix.search_segmented(q, 5, groups)
    for k in (0, 65):
        with pytest.raises(ValueError):
            ix.search_segmented(q, k, [(all4, [(0, 10)])])
    with pytest.raises(ValueError):  # more queries than one call takes
        ix.search_segmented(rindex.synth_rows(2, 0, 1025, 768, "bf16"), 5, [(list(range(1025)), [(0, 10)])])
    # the raw entry point: non-monotone group arrays, group_q[n_groups] != nq
    from rfx import _lib
    out_s = torch.empty((4, 5), dtype=torch.float32, device="cuda")
    out_r = torch.empty((4, 5), dtype=torch.int64, device="cuda")
    ws = torch.empty(1 << 22, dtype=torch.uint8, device="cuda")
    a64 = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.int64))
    for gq, gr in (([0, 3, 2, 4], [0, 1, 2, 3]), ([0, 1, 2, 4], [0, 2, 1, 3]), ([0, 1, 2, 3], [0, 1, 2, 3]),
                   ([1, 2, 3, 4], [0, 1, 2, 3])):
        gq, gr, rg = a64(gq), a64(gr), a64([0, 1, 2, 1, 4, 1])
        rc = _lib.lib.rfx_search_segmented(ix.handle, _lib.ptr(q), 4, 5, 3, gq.ctypes.data, gr.ctypes.data,
                                           rg.ctypes.data, _lib.ptr(out_s), _lib.ptr(out_r), _lib.ptr(ws), ws.numel(),
                                           _lib.stream_ptr())
        assert rc == _lib.RFX_EINVAL, (gq, gr)
    # a valid search afterwards: the segmented answer over everything is the plain search's
    s, r = ix.search_segmented(q, 5, [([2, 0], [(0, 300)]), ([1, 3], [(0, 100), (100, 200)])])
    s0, r0 = ix.search(q, 5)
    assert torch.equal(r, r0) and torch.equal(s, s0)
    s, r = ix.search_segmented(q[:0], 5, [])
    assert s.shape == (0, 5) and r.shape == (0, 5)


# ---- the retriever: tenants' questions in one batch ------------------------------------------------------

def tenant_store(tmp_path, n_tenants, words_per_doc=600):
    from rfx.adapter import LocalGpuRag
    from rfx.retriever import GpuRetriever
    from rfx.store import StoreRegistry, set_registry

    set_registry(StoreRegistry(root=str(tmp_path / "stores")))
    ret = GpuRetriever(dtype="bf16")
    rag = LocalGpuRag(ret, top_k=5)
    st = rag.create_store("tenants")
    rng = np.random.default_rng(3)
    docs = {}
    for t in range(n_tenants):
        tenant = f"tenant{t}"
        docs[tenant] = [f"w{v}" for v in rng.integers(0, 400, size=words_per_doc)]
        p = tmp_path / f"{tenant}.txt"
        p.write_text(" ".join(docs[tenant]))
        rag.upload_file(st, str(p), display_name=f"{tenant}.txt",
                        custom_metadata=[{"key": "tenant", "string_value": tenant}, {"key": "kind", "string_value": "doc"}],
                        chunking_config={"white_space_config": {"max_tokens_per_chunk": 4, "max_overlap_tokens": 0}})
    return rag, ret, st, docs


def ask_all(rag, st, asks, k=5):
    """Every (question, filter) from its own thread, released together."""
    out = [None] * len(asks)
    gate = threading.Barrier(len(asks))

    def ask(i):
        gate.wait()
        out[i] = [(h.row, h.score, h.title) for h in rag.retrieve(asks[i][0], [st], k, metadata_filter=asks[i][1])]

    th = [threading.Thread(target=ask, args=(i,)) for i in range(len(asks))]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    return out


def test_tenants_share_one_batch(rindex, tmp_path, monkeypatch):
    from rfx import retriever as rret

    monkeypatch.delenv("RFX_SEGMENTED", raising=False)
    monkeypatch.delenv("RFX_SEGMENTED_MAX_FRACTION", raising=False)
    rag, ret, st, docs = tenant_store(tmp_path, 4)
    asks = []
    for i in range(32):  # 8 questions per tenant filter, interleaved; two spellings of one filter
        tenant = f"tenant{i % 4}"
        w = docs[tenant]
        filt = {"tenant": tenant, "kind": "doc"} if i % 8 < 4 else {"kind": "doc", "tenant": tenant}
        asks.append((" ".join(w[7 * i:7 * i + 4]), filt))
    ret.batching = False
    solo = [[(h.row, h.score, h.title) for h in rag.retrieve(q, [st], 5, metadata_filter=f)] for q, f in asks]
    assert ret.last_filter_path == "segmented"
    assert all(len(o) == 5 for o in solo)
    assert all(t == f"{f['tenant']}.txt" for o, (_, f) in zip(solo, asks) for _, _, t in o)
    ret.batching = True
    out = ask_all(rag, st, asks)
    assert out == solo  # the same rows, titles and score bits
    assert ret.last_filter_path == "segmented"
    filtered = [v for k, v in rret._BATCHERS.items() if k[0] == st]
    assert len(filtered) == 1, "filtered questions of a store share ONE batcher"
    assert filtered[0].items == 32 and filtered[0].batches < 32
    # RFX_SEGMENTED=0: the parent's path, a batcher and a masked search per filter; the same hits
    monkeypatch.setenv("RFX_SEGMENTED", "0")
    masked = ask_all(rag, st, asks)
    assert ret.last_filter_path == "masked"
    assert masked == solo
    assert len([k for k in rret._BATCHERS if k[0] == st]) == 1 + 4
    # a filter that matches no file answers nothing, on either path
    monkeypatch.setenv("RFX_SEGMENTED", "1")
    assert rag.retrieve("w1 w2", [st], 5, metadata_filter={"tenant": "nobody"}) == []
    rag.delete_store(st)


def test_auto_picks_the_path_by_selectivity(rindex, tmp_path, monkeypatch):
    monkeypatch.delenv("RFX_SEGMENTED", raising=False)
    monkeypatch.delenv("RFX_SEGMENTED_MAX_FRACTION", raising=False)
    rag, ret, st, docs = tenant_store(tmp_path, 8, words_per_doc=200)
    q = " ".join(docs["tenant3"][:4])
    everything = rag.retrieve(q, [st], 5)
    # every file is kind=doc: the filter selects the whole store, so reading its rows saves nothing
    hits = rag.retrieve(q, [st], 5, metadata_filter={"kind": "doc"})
    assert ret.last_filter_path == "masked"
    assert [(h.row, h.score) for h in hits] == [(h.row, h.score) for h in everything]
    # one tenant of eight
    hits = rag.retrieve(q, [st], 5, metadata_filter={"tenant": "tenant3"})
    assert ret.last_filter_path == "segmented"
    assert hits and all(h.title == "tenant3.txt" for h in hits)
    # the fraction is a setting: at 1 the whole-store filter goes segmented too, with the same answer
    monkeypatch.setenv("RFX_SEGMENTED_MAX_FRACTION", "1.0")
    hits = rag.retrieve(q, [st], 5, metadata_filter={"kind": "doc"})
    assert ret.last_filter_path == "segmented"
    assert [(h.row, h.score) for h in hits] == [(h.row, h.score) for h in everything]
    rag.delete_store(st)
