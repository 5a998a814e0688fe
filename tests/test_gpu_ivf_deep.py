"""GPU: the IVF deep search (rfx_ivf_search_deep, csrc/k_ivf_deep.hip) against oracle/ivf.py.  The
int8 stage is integer / single-IEEE-op arithmetic: rows exactly equal, scores equal as floats."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import ivf as oivf
from oracle import search as osearch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def to_np(t, dtype="bf16"):
    t = t.cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if dtype == "bf16" else t.numpy()


def build_from(rows, nlist, iters=4, sample_step=2):
    """tests/test_gpu_ivf.py's recipe over given bf16 rows -> (index, codes, inv, labels, qc, fc)."""
    import rfx.ivf as rivf
    ix = rivf.IvfIndex(rows.shape[1], nlist)
    sample = rows[::sample_step].contiguous()
    ix.train(sample, iters=iters)
    ix.add(rows)
    codes, inv = oivf.quantize(oivf.stored_to_f32(to_np(rows), "bf16"))
    sc, _ = oivf.quantize(oivf.stored_to_f32(to_np(sample), "bf16"))
    qc, fc = oivf.train(sc, nlist, iters)
    return ix, codes, inv, oivf.assign(codes, qc, fc), qc, fc


@functools.lru_cache(maxsize=None)
def built(n, dim, nlist, iters=4, sample_step=2):
    import rfx.ivf as rivf
    rows = rivf.synth_clustered(7, 48, 5, 0, n, dim, "bf16")
    return (rows,) + build_from(rows, nlist, iters, sample_step)


def questions(nq, dim, seed=77):
    import rfx.ivf as rivf
    q = rivf.synth_clustered(7, 48, seed, 0, nq, dim, "bf16")
    return (q,) + oivf.quantize(oivf.stored_to_f32(to_np(q), "bf16"))


def check(ix, q, qq, qinv, codes, inv, lab, qc, fc, nprobe, k, allowed=None):
    mask = None
    if allowed is not None:  # the oracle on labels with the cleared rows moved to a label no question probes
        lab = np.where(allowed, lab, qc.shape[0])
        words = np.packbits(np.pad(allowed, (0, -len(allowed) % 32)), bitorder="little").view(np.int32)
        mask = torch.from_numpy(words.copy()).to(q.device)
    s, r = ix.search_deep(q, k, nprobe, row_mask=mask)
    ref_s, ref_r = oivf.search(qq, qinv, codes, inv, lab, qc, fc, nprobe, k)
    assert np.array_equal(r.cpu().numpy(), ref_r)
    assert np.array_equal(s.cpu().numpy(), ref_s)
    return ref_r


@pytest.mark.parametrize("dim,nlist", [(256, 32), (768, 64), (1024, 130)])
@pytest.mark.parametrize("nq,k,nprobe", [(1, 65, 4), (9, 128, 8), (40, 129, 16), (17, 1000, 32), (3, 1024, 64)])
def test_int8_stage(dim, nlist, nq, k, nprobe):
    if nprobe > nlist:
        pytest.skip("nprobe > nlist")
    _, ix, codes, inv, lab, qc, fc = built(8000, dim, nlist)
    check(ix, *questions(nq, dim), codes, inv, lab, qc, fc, nprobe, k)


def test_four_splits(monkeypatch):
    monkeypatch.setenv("RFX_IVF_SPLITS", "4")
    _, ix, codes, inv, lab, qc, fc = built(8000, 768, 64)
    check(ix, *questions(40, 768), codes, inv, lab, qc, fc, 16, 129)


def test_padding():
    _, ix, codes, inv, lab, qc, fc = built(600, 256, 200, 2, 1)
    ref_r = check(ix, *questions(33, 256, 78), codes, inv, lab, qc, fc, 3, 100)
    assert (ref_r == -1).any()


@pytest.mark.parametrize("k", [100, 1000])
@pytest.mark.parametrize("n,block,nlist,nprobe", [(6000, 300, 8, 4), (3000, 3000, 4, 2)])
def test_ties(n, block, nlist, nprobe, k):
    """Copies of one row: equal scores, the keys differ in the row bits only and the lower row wins."""
    import rfx.ivf as rivf
    base = rivf.synth_clustered(7, 48, 5, 0, n // block, 256, "bf16")
    rows = base.repeat_interleave(block, 0).contiguous()
    ix, codes, inv, lab, qc, fc = build_from(rows, nlist, iters=2)
    check(ix, *questions(5, 256), codes, inv, lab, qc, fc, nprobe, k)


def test_mask():
    _, ix, codes, inv, lab, qc, fc = built(8000, 768, 64)
    q, qq, qinv = questions(9, 768)
    allowed = np.random.default_rng(3).random(8000) < 0.5
    allowed &= ~np.isin(lab, oivf.probes(qq, qc, fc, 8)[0, :3])  # whole lists of question 0's probes cleared
    check(ix, q, qq, qinv, codes, inv, lab, qc, fc, 8, 128, allowed)


def test_rerank():
    from rfx.index import DeviceIndex
    rows, ix, *_ = built(8000, 768, 64)
    bf = DeviceIndex(768, "bf16")
    bf.add(rows)
    q, _, _ = questions(17, 768, 91)
    s, r = ix.search_deep_index(q, 200, 8, bf, rerank_k=400)
    _, cand = ix.search_deep(q, 400, 8)
    rows64 = oivf.stored_to_f32(to_np(rows), "bf16").astype(np.float64)
    q64 = oivf.stored_to_f32(to_np(q), "bf16").astype(np.float64)
    ref_s, ref_r = oivf.rerank(cand.cpu().numpy(), q64, rows64, 200)
    probs = osearch.check_topk(s.cpu().numpy(), r.cpu().numpy(), ref_s, ref_r, lambda qi, rr: rows64[rr] @ q64[qi],
                               tol=1e-5, tie_band=2e-6)
    assert not probs, probs[:5]


def test_retriever(tmp_path, monkeypatch):
    from rfx import store as rstore
    from rfx.adapter import LocalGpuRag
    from rfx.retriever import DEEP_ERROR, GpuRetriever
    with open(os.path.join(ROOT, "tests", "golden", "sample_report.md"), encoding="utf-8") as f:
        words = list(np.random.default_rng(1).choice(f.read().split(), 3600))  # ~300 chunks a file
    reg = rstore.StoreRegistry(root=str(tmp_path / "s"), device=0)
    ret = GpuRetriever(registry=reg, dtype="bf16")
    rag = LocalGpuRag(ret, top_k=5)
    cfg = {"white_space_config": {"max_tokens_per_chunk": 4, "max_overlap_tokens": 1}}
    stores = {}
    for name, train_min in (("trained", 64), ("untrained", 1 << 30)):
        st = reg.create(name, 768, "bf16", spec={"kind": "ivf", "nlist": 16, "nprobe": 8, "train_min": train_min})
        for i in range(4):
            p = tmp_path / f"part{i}.md"
            p.write_text(" ".join(words[i * len(words) // 4:(i + 1) * len(words) // 4]), encoding="utf-8")
            rag.upload_file(st.name, str(p), display_name=p.name, chunking_config=cfg)
        stores[name] = st
    question = "source citations in chat answers"
    with pytest.raises(ValueError, match=DEEP_ERROR):
        ret.candidates([stores["trained"].name], question, 200)
    monkeypatch.setenv("RFX_IVF_DEEP", "1")
    for name, st in stores.items():
        assert st.ivf_ready() == (name == "trained") and st.index.rows > 400
        if name == "trained":
            st.delete_file(next(iter(st.files)))
        hits = ret.candidates([st.name], question, 200)
        with st.lock, torch.cuda.device(st.device):
            q = ret.embedder(st.dim).embed_texts([question], st.dtype)
            s, r = (st if name == "trained" else st.index).search_deep(q, 200)
        r = r[0].cpu().numpy()
        live = [int(x) for x in r if x >= 0 and st.row_info(int(x)) is not None]
        assert [h.row for h in hits] == live and len(hits) > 100
        assert all(a.score >= b.score for a, b in zip(hits, hits[1:]))
