"""GPU: diversified retrieval — the MMR selection over the top candidates of a search (rfx_mmr_select,
DESIGN §4.13) against the numpy float64 reference of the rule (tests/mmr_ref.py): parity for every dtype and
dim, the two properties of the contract (lambda = 1, prefix stability), independence of the batch, padding
and tombstones, masked and union-view candidates, every refused argument, and LocalGpuRag end to end."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mmr_ref

pytestmark = pytest.mark.gpu

ROWS, NQ = 4096, 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def to64(t):
    """Stored rows (a device tensor of the index dtype) widened exactly to float64."""
    return t.float().cpu().numpy().astype(np.float64)


def corpus(kind, dtype, dim):
    """(index, rows64, queries, the reference's answers so far): built once per (kind, dtype, dim); rows seed 7,
    queries seed 11, 16 centres of seed 3 for the clustered kind."""
    key = (kind, dtype, dim)
    if key not in _CACHE:
        from rfx.index import DeviceIndex, synth_rows
        from rfx.ivf import synth_clustered
        ix = DeviceIndex(dim, dtype, 0)
        if kind == "synth":
            ix.add_synthetic(7, ROWS)
            q = synth_rows(11, 0, NQ, dim, dtype, 0)
        else:
            ix.add(synth_clustered(3, 16, 7, 0, ROWS, dim, dtype))
            q = synth_clustered(3, 16, 11, 0, NQ, dim, dtype)
        _CACHE[key] = (ix, to64(ix.read(0, ROWS)), q)
    return _CACHE[key]


def compare(got_s, got_r, cs, cr, rows64, k, lam, n_cand=None, max_out=2):
    """The GPU's selection against the reference on the same candidates.  A query whose reference margin is
    below mmr_ref.MARGIN at some step is only checked for validity; at most max_out such queries.  Returns
    the number of queries whose selection differs from the plain top-k."""
    got_s, got_r, cs, cr = (t.cpu().numpy() for t in (got_s, got_r, cs, cr))
    ref_s, ref_r, _, margin = mmr_ref.select_batch(cs, cr, rows64, k, lam, n_cand)
    out = 0
    for q in range(len(cs)):
        if margin[q] < mmr_ref.MARGIN:
            out += 1
            mmr_ref.check_valid(got_s[q], got_r[q], cs[q], cr[q])
            continue
        assert np.array_equal(got_r[q], ref_r[q]), (q, got_r[q], ref_r[q], margin[q])
        assert got_s[q].tobytes() == ref_s[q].tobytes(), q
    print(f"left out of the row comparison: {out} of {len(cs)}")
    assert out <= max_out, out
    return int(sum(not np.array_equal(got_r[q], cr[q, :k]) for q in range(len(cs))))


@pytest.mark.parametrize("dim", [768, 1024])
@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("kind,fetch_k,k,lam", [("synth", 64, 10, 0.5), ("synth", 20, 10, 0.7),
                                                ("clustered", 64, 10, 0.5), ("clustered", 64, 32, 0.3)])
def test_parity(kind, fetch_k, k, lam, dtype, dim):
    ix, rows64, q = corpus(kind, dtype, dim)
    cs, cr = ix.search(q, fetch_k)
    s, r = ix.mmr_select(q, cs, cr, k, lam=lam)
    differ = compare(s, r, cs, cr, rows64, k, lam)
    print(f"selections that differ from the plain top-{k}: {differ} of {NQ}")
    assert differ >= NQ // 2  # (an identity kernel cannot pass)


@pytest.mark.parametrize("dtype,dim", [("bf16", 768), ("f16", 1024), ("f32", 768)])
def test_lambda_one_and_prefix_stability(dtype, dim):
    ix, rows64, q = corpus("clustered", dtype, dim)
    cs, cr = ix.search(q, 64)
    s, r = ix.mmr_select(q, cs, cr, 32, lam=1.0)
    assert torch.equal(r, cr[:, :32]) and torch.equal(s.view(torch.int32), cs[:, :32].contiguous().view(torch.int32))
    for lam in (0.0, 0.3):
        s32, r32, o32 = ix.mmr_select(q, cs, cr, 32, lam=lam, return_objective=True)
        s10, r10, o10 = ix.mmr_select(q, cs, cr, 10, lam=lam, return_objective=True)
        assert torch.equal(r32[:, :10], r10) and torch.equal(s32[:, :10], s10) and torch.equal(o32[:, :10], o10)
    # the objectives are the reference's, rounded to f32
    _, ref_r, ref_o, margin = mmr_ref.select_batch(cs.cpu().numpy(), cr.cpu().numpy(), rows64, 10, 0.3)
    ok = margin >= mmr_ref.MARGIN
    assert ok.sum() >= NQ - 2
    assert np.array_equal(o10.cpu().numpy()[ok], ref_o[ok].astype(np.float32))


def test_batch_independence():
    ix, rows64, q = corpus("clustered", "bf16", 768)
    cs, cr = ix.search(q, 64)
    rng = np.random.default_rng(5)
    lam = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0], dtype=np.float32), NQ)
    nc = rng.integers(1, 65, NQ).astype(np.int32)
    nc[:4] = (1, 64, 33, 4)
    k = 8
    s, r = ix.mmr_select(q, cs, cr, k, lam=lam, n_cand=nc)
    for i in range(0, NQ, 3):  # the same queries alone
        s1, r1 = ix.mmr_select(q[i:i + 1], cs[i:i + 1], cr[i:i + 1], k, lam=float(lam[i]), n_cand=int(nc[i]))
        assert torch.equal(r1[0], r[i]) and torch.equal(s1[0], s[i]), i
    compare(s, r, cs, cr, rows64, k, lam, nc)
    r = r.cpu().numpy()
    for i in range(NQ):  # n_cand below k: the tail is padding, and nothing past n_cand is picked
        n = min(int(nc[i]), k)
        assert (r[i, :n] >= 0).all() and (r[i, n:] == -1).all()
        assert set(r[i, :n].tolist()) <= set(cr[i, :nc[i]].tolist())


def test_padding_and_tombstones():
    from rfx.index import DeviceIndex, synth_rows
    q = synth_rows(11, 0, 4, 768, "bf16", 0)
    # fewer live rows than k
    small = DeviceIndex(768, "bf16", 0)
    small.add_synthetic(7, 6)
    small.tombstone([2])
    s, r = small.search_mmr(q, 8, 16, lam=0.5)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    for i in range(4):
        assert sorted(r[i, :5].tolist()) == [0, 1, 3, 4, 5] and (r[i, 5:] == -1).all() and np.isneginf(s[i, 5:]).all()
    small.close()
    # a candidate tombstoned between the search and the select is never returned
    ix = DeviceIndex(768, "bf16", 0)
    ix.add_synthetic(7, ROWS)
    cs, cr = ix.search(q, 32)
    dead = [int(cr[i, j]) for i in range(4) for j in (0, 3)]
    ix.tombstone(dead)
    rows64 = to64(ix.read(0, ROWS))
    assert np.isnan(rows64[dead]).all()
    s, r = ix.mmr_select(q, cs, cr, 10, lam=0.5)
    assert not set(r.cpu().numpy().ravel().tolist()) & set(dead)
    compare(s, r, cs, cr, rows64, 10, 0.5)
    # hand-assembled candidates: row -1 in the middle, a row past the end
    cr2 = cr.clone()
    cr2[:, 5] = -1
    cr2[:, 9] = ROWS
    cr2[:, 11] = 1 << 40
    s, r = ix.mmr_select(q, cs, cr2, 12, lam=0.6)
    got = r.cpu().numpy()
    assert (got >= 0).all() and (got < ROWS).all() and not set(got.ravel().tolist()) & set(dead)
    ref_s, ref_r, _, margin = mmr_ref.select_batch(cs.cpu().numpy(), cr2.cpu().numpy(), rows64, 12, 0.6)
    assert (margin >= mmr_ref.MARGIN).all()
    assert np.array_equal(got, ref_r) and s.cpu().numpy().tobytes() == ref_s.tobytes()
    ix.close()


def test_masked_candidates():
    ix, rows64, q = corpus("clustered", "bf16", 768)
    allowed = np.zeros(ROWS, dtype=bool)
    allowed[np.random.default_rng(3).permutation(ROWS)[:ROWS // 3]] = True
    words = np.packbits(allowed.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).ravel().view(np.int32)
    mask = ix.mask_tensor(words)
    s, r = ix.search_mmr(q, 10, 48, lam=0.4, row_mask=mask)
    cs, cr = ix.search(q, 48, row_mask=mask)
    assert allowed[r.cpu().numpy()].all()
    assert compare(s, r, cs, cr, rows64, 10, 0.4) >= NQ // 2


def test_union_view():
    from rfx._lib import check, lib, stream_ptr
    from rfx.index import DeviceIndex
    from rfx.ivf import synth_clustered
    a, b = DeviceIndex(768, "bf16", 0), DeviceIndex(768, "bf16", 0)
    a.add(synth_clustered(3, 16, 7, 0, 1500, 768, "bf16"))
    b.add(synth_clustered(3, 16, 7, 1500, 1100, 768, "bf16"))
    handles, bases, h = (ctypes.c_uint64 * 2)(a.handle, b.handle), (ctypes.c_int64 * 2)(), ctypes.c_uint64()
    check(lib.rfx_union_create(handles, 2, stream_ptr(), ctypes.byref(h), bases))
    view = DeviceIndex(768, "bf16", 0, _handle=h.value)
    rows64 = to64(view.read(0, view.rows))  # the members back to back, NaN between them
    q = synth_clustered(3, 16, 11, 0, NQ, 768, "bf16")
    s, r = view.search_mmr(q, 10, 64, lam=0.5)
    cs, cr = view.search(q, 64)
    assert compare(s, r, cs, cr, rows64, 10, 0.5) >= NQ // 2
    got = r.cpu().numpy()
    assert ((got >= bases[1]) & (got < bases[1] + 1100)).any() and (got < 1500).any()  # picks from both members
    view.close()
    a.close()
    b.close()


def test_refused_arguments():
    from rfx import _lib
    from rfx._lib import lib, ptr, stream_ptr
    ix, _, q = corpus("synth", "bf16", 768)
    nq, n_max, k = 4, 16, 8
    q = q[:nq].contiguous()
    cs, cr = ix.search(q, n_max)
    out_s = torch.full((nq, 64), 123.0, dtype=torch.float32, device="cuda")
    out_r = torch.full((nq, 64), -77, dtype=torch.int64, device="cuda")
    out_o = torch.full((nq, 64), 123.0, dtype=torch.float32, device="cuda")
    ws = torch.empty(ix.mmr_workspace_bytes(1024, 64), dtype=torch.uint8, device="cuda")

    def call(nq=nq, n_max=n_max, k=k, lam=None, nc=None, ws_bytes=ws.numel(), handle=ix.handle):
        lam_a = None if lam is None else np.asarray(lam, dtype=np.float32)
        nc_a = None if nc is None else np.asarray(nc, dtype=np.int32)
        return lib.rfx_mmr_select(handle, ptr(q), nq, n_max, k, lam_a.ctypes.data if lam_a is not None else None,
                                  nc_a.ctypes.data if nc_a is not None else None, ptr(cs), ptr(cr), ptr(out_s),
                                  ptr(out_r), ptr(out_o), ptr(ws), ws_bytes, stream_ptr())

    bad = [dict(k=0), dict(k=65, n_max=64),dict(n_max=0), dict(n_max=65), dict(k=n_max + 1), dict(nq=0), dict(nq=1025),
           dict(lam=[0.5, -0.01, 0.5, 0.5]), dict(lam=[0.5, 0.5, 1.5, 0.5]), dict(lam=[0.5, 0.5, 0.5, float("nan")]),
           dict(nc=[16, 0, 16, 16]), dict(nc=[16, 16, 17, 16]), dict(nc=[-1, 16, 16, 16]),
           dict(ws_bytes=ix.mmr_workspace_bytes(nq, n_max) - 1), dict(ws_bytes=0), dict(handle=0xdead)]
    for kw in bad:
        assert call(**kw) == _lib.RFX_EINVAL, kw
    torch.cuda.synchronize()
    assert (out_s == 123.0).all() and (out_r == -77).all() and (out_o == 123.0).all()
    need = ctypes.c_size_t()
    for args in ((0, 16), (1025, 16), (4, 0), (4, 65)):
        assert lib.rfx_mmr_workspace_bytes(ix.handle, *args, ctypes.byref(need)) == _lib.RFX_EINVAL, args
    # the same call with nothing wrong writes [nq][k]
    assert call(lam=[0.5] * 4, nc=[16] * 4) == _lib.RFX_OK
    torch.cuda.synchronize()
    assert (out_r.view(-1)[:nq * k] >= 0).all() and (out_r.view(-1)[nq * k:] == -77).all()
    with pytest.raises(ValueError):
        ix.search_mmr(q, 10, 8)
    with pytest.raises(ValueError):
        ix.mmr_select(q, cs, cr, 8, lam=2.0)


def test_local_gpu_rag_end_to_end(tmp_path):
    from rfx import store as rstore
    from rfx.adapter import LocalGpuRag
    from rfx.retriever import GpuRetriever

    ws = {"white_space_config": {"max_tokens_per_chunk": 12, "max_overlap_tokens": 2}}
    report = os.path.join(ROOT, "tests", "golden", "sample_report.md")
    reg = rstore.StoreRegistry(root=str(tmp_path / "flat"), device=0)
    ret = GpuRetriever(registry=reg, dtype="bf16")
    rag = LocalGpuRag(ret, top_k=4)
    st = rag.create_store("reports")
    for name in ("report.md", "report-copy.md"):  # the same file under two names
        rag.upload_file(st, report, display_name=name, chunking_config=ws)
    questions = ["document stores for authenticated users", "source citations in chat answers",
                 "mock responses in demo mode"]

    def hits(q, **kw):
        return [(h.score, h.row, h.title, h.text) for h in rag.retrieve(q, [st], **kw)]

    for batching in (False, True):
        ret.batching = batching
        for q in questions:
            plain = hits(q)
            assert ret.last_diversity is None
            assert plain[0][3] == plain[1][3] and plain[0][2] != plain[1][2]  # the two copies of one chunk
            div = hits(q, diversity=0.5)
            assert ret.last_diversity == "store"
            assert div[0] == plain[0] and div[1][3] != div[0][3], (q, div)
            assert len({h[1] for h in div}) == 4
            # lambda 1 over the default fetch_k, and diversity=None, are the plain answer
            assert hits(q, diversity={"lambda": 1.0, "fetch_k": 16}) == plain
            assert hits(q, diversity=None) == plain
            # ask / ask_stream carry the keyword; the response shape is the plain one
            resp = rag.ask(contents=q, store_names=[st], metadata_filter=None, model="m", diversity=0.5)
            cites = rag.extract_citations_from_response(resp)
            assert [c["snippet"] for c in cites] == [h[3] for h in div]
            last = list(rag.ask_stream(contents=q, store_names=[st], metadata_filter=None, model="m", diversity=0.5))[-1]
            assert [c["snippet"] for c in rag.extract_citations_from_response(last)] == [h[3] for h in div]
    with pytest.raises(ValueError):
        hits(questions[0], k=4, diversity={"lambda": 0.5, "fetch_k": 3})

    # two stores in one question: diversified across the stores on the union view
    st2 = rag.create_store("reports-2")
    rag.upload_file(st2, report, display_name="report-third.md", chunking_config=ws)
    both = [(h.score, h.store, h.text) for h in rag.retrieve(questions[0], [st, st2], diversity=0.5)]
    assert ret.last_path == "union" and ret.last_diversity == "union"
    assert len({t for _, _, t in both}) == len(both)  # no chunk text twice among the 4
    ret.union = False
    per = [(h.score, h.store, h.text) for h in rag.retrieve(questions[0], [st, st2], diversity=0.5)]
    assert ret.last_path == "per-store" and ret.last_diversity == "store" and len(per) == 4
    ret.union = True

    # RFX_MMR_LAMBDA: the default lambda of an adapter
    os.environ["RFX_MMR_LAMBDA"] = "0.5"
    try:
        rag2 = LocalGpuRag(ret, top_k=4)
    finally:
        del os.environ["RFX_MMR_LAMBDA"]
    assert rag2.diversity == 0.5 and rag.diversity is None
    got = [(h.score, h.row, h.title, h.text) for h in rag2.retrieve(questions[1], [st])]
    assert got == hits(questions[1], diversity=0.5)

    # a sharded store refuses
    sreg = rstore.StoreRegistry(root=str(tmp_path / "flat"), device=0, devices="0x2")
    srag = LocalGpuRag(GpuRetriever(registry=sreg, dtype="bf16"), top_k=4)
    assert [h.text for h in srag.retrieve(questions[0], [st])] == [h[3] for h in hits(questions[0])]
    with pytest.raises(ValueError, match="flat single-device store"):
        srag.retrieve(questions[0], [st], diversity=0.5)
