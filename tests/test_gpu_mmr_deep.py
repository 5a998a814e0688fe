"""GPU: diversified retrieval at depth — the MMR selection over 65..1,024 candidates (rfx_mmr_select_deep,
DESIGN §4.22) against the numpy float64 reference of the rule (tests/mmr_ref.py) over the exactly widened rows.
The candidates are search_deep's on synth_rows stores of 5,000 rows.  A question whose reference margin is under
mmr_ref.MARGIN is left out of the row comparison (and still checked for validity), at most one in eight of a
cell; the question seeds of every cell were chosen on the CPU so that the reference alone meets this."""
import os

import numpy as np
import pytest
import torch

import mmr_ref

pytestmark = pytest.mark.gpu

ROWS = 5000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_STORES, _REFS = {}, {}
S8 = (11, 12, 13, 14, 15, 16, 17, 18)
# (n_cand, dim, dtype, k, lambda): the seeds of its 8 questions
CELLS = {(65, 64, "bf16", 1, 0.3): S8, (65, 768, "f16", 10, 0.7): S8,
         (128, 64, "f16", 64, 0.3): (11, 13, 14, 15, 16, 17, 18, 19),
         (128, 768, "bf16", 65, 0.7): (11, 13, 15, 16, 18, 19, 20, 21), (128, 768, "f16", 1, 0.7): S8,
         (1000, 64, "bf16", 65, 0.3): (11, 12, 13, 14, 16, 17, 18, 19), (1000, 64, "bf16", 10, 0.3): S8,
         (1000, 64, "bf16", 200, 0.7): (11, 17, 20, 21, 22, 24, 25, 26),
         (1024, 64, "f16", 200, 0.3): (11, 12, 18, 19, 24, 28, 29, 35), (1024, 768, "bf16", 10, 0.7): S8,
         (1024, 768, "bf16", 64, 0.3): (11, 12, 13, 14, 16, 17, 18, 19)}


def store(dim, dtype):
    """(index, rows64): 5,000 synth_rows of seed 7, built once per (dim, dtype)."""
    if (dim, dtype) not in _STORES:
        from rfx.index import DeviceIndex
        ix = DeviceIndex(dim, dtype, 0)
        ix.add_synthetic(7, ROWS)
        _STORES[(dim, dtype)] = (ix, ix.read(0, ROWS).float().cpu().numpy().astype(np.float64))
    return _STORES[(dim, dtype)]


def questions(seeds, dim, dtype):
    from rfx.index import synth_rows
    return torch.cat([synth_rows(s, 0, 1, dim, dtype, 0) for s in seeds])


def cell(n, dim, dtype, k, lam):
    """(index, rows64, q, candidates, the reference's answer): computed once per cell."""
    key = (n, dim, dtype, k, lam)
    if key not in _REFS:
        ix, rows64 = store(dim, dtype)
        q = questions(CELLS[key], dim, dtype)
        cs, cr = ix.search_deep(q, n)
        _REFS[key] = (ix, rows64, q, cs, cr, mmr_ref.select_batch(cs.cpu().numpy(), cr.cpu().numpy(), rows64, k, lam))
    return _REFS[key]


def compare(got, cs, cr, ref):
    """Rows, scores and f32 objectives equal to the reference's; at most one question in eight left out."""
    (s, r, o), cs, cr = (t.cpu().numpy() for t in got), cs.cpu().numpy(), cr.cpu().numpy()
    ref_s, ref_r, ref_o, margin = ref
    out = 0
    for q in range(len(cs)):
        print(f"question {q}: reference margin {margin[q]:.3g}")
        if margin[q] < mmr_ref.MARGIN:
            out += 1
            mmr_ref.check_valid(s[q], r[q], cs[q], cr[q])
            continue
        assert np.array_equal(r[q], ref_r[q]), (q, r[q], ref_r[q])
        assert s[q].tobytes() == ref_s[q].tobytes() and np.array_equal(o[q], ref_o[q].astype(np.float32)), q
    assert out * 8 <= len(cs), out
    return int(sum(not np.array_equal(r[q], cr[q, :r.shape[1]]) for q in range(len(cs))))


@pytest.mark.parametrize("n,dim,dtype,k,lam", list(CELLS))
def test_parity(n, dim, dtype, k, lam):
    ix, rows64, q, cs, cr, ref = cell(n, dim, dtype, k, lam)
    *got, stats = ix.mmr_select_deep(q, cs, cr, k, lam=lam, return_objective=True, stats=True)
    differ = compare(got, cs, cr, ref)
    print(f"differ from the plain top-{k}: {differ} of 8; contenders, exact dots per question: {stats.cpu().tolist()}")
    assert k == 1 or differ >= 4  # (an identity kernel cannot pass)
    s2, r2 = ix.mmr_select_deep(q, cs, cr, k, lam=lam)  # without the objectives: fewer exact dots, the same picks
    assert torch.equal(r2, got[1]) and torch.equal(s2, got[0])


def test_lambda_one_bit_for_bit():
    ix, _, q, cs, cr, _ = cell(1024, 768, "bf16", 10, 0.7)
    s, r = ix.mmr_select_deep(q, cs, cr, 1024, lam=1.0)
    assert torch.equal(r, cr) and torch.equal(s.view(torch.int32), cs.view(torch.int32))


def test_prefix_stability():
    ix, _, q, cs, cr, _ = cell(1024, 64, "f16", 200, 0.3)
    s200, r200, o200 = ix.mmr_select_deep(q, cs, cr, 200, lam=0.3, return_objective=True)
    s64, r64, o64 = ix.mmr_select_deep(q, cs, cr, 64, lam=0.3, return_objective=True)
    assert torch.equal(r200[:, :64], r64) and torch.equal(s200[:, :64], s64) and torch.equal(o200[:, :64], o64)


def test_identical_rows_go_to_the_lower_position():
    from rfx.index import DeviceIndex
    ix0, _ = store(64, "bf16")
    q = questions((11,), 64, "bf16")
    best = int(ix0.search_deep(q, 65)[1][0, 0])
    ix = DeviceIndex(64, "bf16", 0)
    ix.add(ix0.read(0, ROWS))
    ix.write(1000, ix0.read(best, 1).expand(300, 64).contiguous())  # 300 copies of the question's best row
    cs, cr = ix.search_deep(q, 1024)
    block = cr[0, :301].cpu().numpy()  # the copies and the original: one score, rows ascending
    assert set(range(1000, 1300)) <= set(block.tolist()) and (cs[0, :301] == cs[0, 0]).all()
    s, r = ix.mmr_select_deep(q, cs, cr, 1024, lam=0.5)  # every candidate: the copies are picked at some step
    mmr_ref.check_valid(s[0].cpu().numpy(), r[0].cpu().numpy(), cs[0].cpu().numpy(), cr[0].cpu().numpy())
    got = [x for x in r[0].cpu().tolist() if x in set(block.tolist())]
    assert got == sorted(got) and len(got) == 301  # equal objectives at every step: the lower position first
    ix.close()
    # every candidate the same row: n 128, k 65 — the first 65 in order
    same = DeviceIndex(64, "bf16", 0)
    same.add(ix0.read(best, 1).expand(200, 64).contiguous())
    cs, cr = same.search_deep(q, 128)
    s, r, o = same.mmr_select_deep(q, cs, cr, 65, lam=0.5, return_objective=True)
    assert torch.equal(r, cr[:, :65]) and torch.equal(s, cs[:, :65]) and (o[0, 1:] == o[0, 1]).all()
    same.close()


def test_batch_independence():
    ix, rows64, q, cs, cr, _ = cell(1024, 768, "bf16", 10, 0.7)
    lam, nc = [0.2, 0.9, 0.5, 1.0, 0.0, 0.6, 0.3, 0.8], [65, 700, 1024, 700, 65, 1024, 129, 64]
    s, r, o = ix.mmr_select_deep(q, cs, cr, 70, lam=lam, n_cand=nc, return_objective=True)
    for i in range(8):  # the same question alone, with its own list length
        s1, r1, o1 = ix.mmr_select_deep(q[i:i + 1], cs[i:i + 1, :max(nc[i], 65)].contiguous(),
                                        cr[i:i + 1, :max(nc[i], 65)].contiguous(), 70 if nc[i] >= 70 else 65, lam=lam[i],
                                        n_cand=nc[i], return_objective=True)
        m = min(70, s1.shape[1])
        assert torch.equal(r1[0, :m], r[i, :m]) and torch.equal(s1[0, :m], s[i, :m]) and torch.equal(o1[0, :m], o[i, :m]), i
    r = r.cpu().numpy()
    for i in range(8):  # n_cand below k: the tail is padding, and nothing past n_cand is picked
        m = min(nc[i], 70)
        assert (r[i, :m] >= 0).all() and (r[i, m:] == -1).all() and set(r[i, :m].tolist()) <= set(cr[i, :nc[i]].tolist())


def test_padding_and_tombstones():
    from rfx.index import DeviceIndex
    ix0, _ = store(768, "bf16")
    ix = DeviceIndex(768, "bf16", 0)
    ix.add(ix0.read(0, ROWS))
    q = questions(S8, 768, "bf16")
    cs, cr = ix.search_deep(q, 200)
    dead = [int(cr[i, j]) for i in range(8) for j in (0, 3, 60)]
    ix.tombstone(dead)  # tombstoned between the search and the select
    rows64 = ix.read(0, ROWS).float().cpu().numpy().astype(np.float64)
    cr2 = cr.clone()
    cr2[:, 5], cr2[:, 9], cr2[:, 150] = -1, ROWS, 1 << 40
    s, r, o = ix.mmr_select_deep(q, cs, cr2, 20, lam=0.6, return_objective=True)
    got = r.cpu().numpy()
    assert (got >= 0).all() and (got < ROWS).all() and not set(got.ravel().tolist()) & set(dead)
    compare((s, r, o), cs, cr2, mmr_ref.select_batch(cs.cpu().numpy(), cr2.cpu().numpy(), rows64, 20, 0.6))
    # fewer valid candidates than k: 66 asked of 70, of which at least 5 are dead, -1 or past the end
    s, r = ix.mmr_select_deep(q, cs, cr2, 66, lam=0.5, n_cand=70)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    for i in range(8):
        nv = sum(0 <= x < ROWS and x not in dead for x in cr2[i, :70].tolist())
        assert nv <= 65 and (r[i, :nv] >= 0).all() and (r[i, nv:] == -1).all() and np.isneginf(s[i, nv:]).all()
    ix.close()


def test_refused_arguments():
    import ctypes
    from rfx import _lib
    from rfx._lib import lib, ptr, stream_ptr
    from rfx.index import DeviceIndex
    ix, _, q, cs, cr, _ = cell(128, 768, "bf16", 65, 0.7)
    nq, n_max, k = 4, 128, 80
    out_s = torch.full((nq, 128), 123.0, dtype=torch.float32, device="cuda")
    out_r = torch.full((nq, 128), -77, dtype=torch.int64, device="cuda")
    out_o = torch.full((nq, 128), 123.0, dtype=torch.float32, device="cuda")
    ws = torch.empty(ix.mmr_deep_workspace_bytes(nq, n_max) + 256, dtype=torch.uint8, device="cuda")

    def call(nq=nq, n_max=n_max, k=k, lam=None, nc=None, ws_bytes=ws.numel() - 256, handle=ix.handle, off=0):
        lam_a = None if lam is None else np.asarray(lam, dtype=np.float32)
        nc_a = None if nc is None else np.asarray(nc, dtype=np.int32)
        return lib.rfx_mmr_select_deep(handle, ptr(q), nq, n_max, k, lam_a.ctypes.data if lam_a is not None else None,
                                       nc_a.ctypes.data if nc_a is not None else None, ptr(cs), ptr(cr), ptr(out_s),
                                       ptr(out_r), ptr(out_o), ctypes.c_void_p(ws.data_ptr() + off), ws_bytes, stream_ptr())

    bad = [dict(k=0), dict(n_max=64, k=10), dict(n_max=1025), dict(k=n_max + 1), dict(nq=0), dict(nq=1025),
           dict(lam=[0.5, -0.01, 0.5, 0.5]), dict(lam=[0.5, 0.5, 1.5, 0.5]), dict(lam=[0.5, 0.5, 0.5, float("nan")]),
           dict(nc=[128, 0, 128, 128]), dict(nc=[128, 128, 129, 128]), dict(nc=[-1, 128, 128, 128]),
           dict(ws_bytes=ix.mmr_deep_workspace_bytes(nq, n_max) - 1), dict(ws_bytes=0), dict(off=16), dict(handle=0xdead)]
    for kw in bad:
        assert call(**kw) == _lib.RFX_EINVAL, kw
    f32 = DeviceIndex(768, "f32", 0)
    f32.add_synthetic(7, 256)
    assert call(handle=f32.handle) == _lib.RFX_EUNSUPPORTED
    need = ctypes.c_size_t()
    assert lib.rfx_mmr_deep_workspace_bytes(f32.handle, 4, 128, ctypes.byref(need)) == _lib.RFX_EUNSUPPORTED
    f32.close()
    for args in ((0, 128), (1025, 128), (4, 64), (4, 1025)):
        assert lib.rfx_mmr_deep_workspace_bytes(ix.handle, *args, ctypes.byref(need)) == _lib.RFX_EINVAL, args
    torch.cuda.synchronize()
    assert (out_s == 123.0).all() and (out_r == -77).all() and (out_o == 123.0).all()
    assert call(lam=[0.5] * 4, nc=[128] * 4) == _lib.RFX_OK  # the same call with nothing wrong writes [nq][k]
    torch.cuda.synchronize()
    assert (out_r.view(-1)[:nq * k] >= 0).all() and (out_r.view(-1)[nq * k:] == -77).all()
    with pytest.raises(ValueError):
        ix.search_mmr_deep(q, 10, 64)


def test_local_gpu_rag_end_to_end(tmp_path):
    from rfx import store as rstore
    from rfx.adapter import LocalGpuRag
    from rfx.retriever import GpuRetriever
    ws = {"white_space_config": {"max_tokens_per_chunk": 12, "max_overlap_tokens": 2}}
    report = os.path.join(ROOT, "tests", "golden", "sample_report.md")
    ret = GpuRetriever(registry=rstore.StoreRegistry(root=str(tmp_path / "flat"), device=0), dtype="bf16")
    rag = LocalGpuRag(ret, top_k=4)
    st = rag.create_store("reports")
    for name in ("report.md", "report-copy.md"):  # the same file under two names
        rag.upload_file(st, report, display_name=name, chunking_config=ws)
    question = "document stores for authenticated users"
    plain = rag.retrieve(question, [st], top_k=100)
    div = rag.retrieve(question, [st], top_k=100, diversity=0.5)
    assert ret.last_diversity == "store" and plain[0].text == plain[1].text
    assert [(h.score, h.row) for h in div] == [(h.score, h.row) for h in ret.candidates([st], question, 100, diversity=0.5)]
    # the picks in order, with their objectives: a text repeats only when no unseen text has a positive objective
    store_ = ret.registry.get(st)
    q = ret.embedder(store_.dim).embed_texts([question], "bf16")
    cs, cr = store_.index.search_deep(q, 400)
    _, r, o = store_.index.mmr_select_deep(q, cs, cr, 100, lam=0.5, return_objective=True)
    picks = [x for x in r[0].tolist() if x >= 0]
    assert sorted(picks) == sorted(h.row for h in div) and len(picks) == store_.index.rows
    text_of, seen = {h.row: h.text for h in plain}, set()
    for t, row in enumerate(picks):
        if text_of[row] in seen and len(seen) < len(set(text_of.values())):
            assert float(o[0, t]) <= 0.0, (t, float(o[0, t]))
        seen.add(text_of[row])
    assert text_of[picks[0]] != text_of[picks[1]]
    # k <= 64 with a pool beyond 64 takes the deep route; hybrid with it is refused
    small = ret.candidates([st], question, 8, diversity={"lambda": 0.5, "fetch_k": 200})
    assert ret.last_diversity == "store" and sorted(h.row for h in small) == sorted(picks[:8])
    with pytest.raises(ValueError, match="together with hybrid"):
        ret.candidates([st], question, 100, diversity=0.5, hybrid=0.5)
