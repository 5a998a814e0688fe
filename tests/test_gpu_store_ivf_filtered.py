"""GPU: metadata-filtered questions of an IVF store answered from its posting lists (LocalStore.search_filtered,
RFX_IVF_FILTERED).  The store of tests/test_gpu_store_ivf.py: 6,000 clustered rows in four files,
tenants t0 .. t2 on the first three, the second file deleted, nlist 32, nprobe 8.  Tenant t0 owns 1,500 of the
4,500 live rows, so the rule widens nprobe to ceil(8 * 4500 / 1500) = 24 <= 32.

Recall: the floor is the CPU reference's own recall on the same rows minus 0.02 — tests/ivf_mask_ref.py's search
followed by oracle.ivf.rerank, against the oracle's exact filtered top-10; the 0.02 allows for the f32 re-rank
ordering near-equal scores differently from f64.  The reference value, computed by this test before the GPU
answer is looked at, must itself be >= 0.9."""
import numpy as np
import pytest
import torch

import ivf_mask_ref as mr
from oracle import ivf as oivf

pytestmark = pytest.mark.gpu

DIM, NLIST, NPROBE = 768, 32, 8
SPEC = {"kind": "ivf", "nlist": NLIST, "nprobe": NPROBE, "train_min": 4000}
T0 = {"tenant": "t0"}


def to_np_bf16(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from rfx import ivf as rivf
    from rfx import store as rstore
    reg = rstore.StoreRegistry(root=str(tmp_path_factory.mktemp("ivf-filtered")), device=0)
    st = reg.create("ivf-demo", DIM, "bf16", spec=SPEC)
    docs = [rivf.synth_clustered(7, 48, 100 + i, 1500 * i, 1500, DIM, "bf16") for i in range(4)]
    for i, v in enumerate(docs[:3]):
        fid = st.add_document([f"d{i}-{j}" for j in range(1500)], v, f"d{i}.md", {"tenant": f"t{i}"})[0]
        if i == 1:
            st.delete_file(fid)
    st.add_document([f"d3-{j}" for j in range(1500)], docs[3], "d3.md")
    assert st.ivf_ready() and st.dead_rows() == 1500
    q = rivf.synth_clustered(7, 48, 999, 0, 40, DIM, "bf16")
    yield reg, st, np.concatenate([to_np_bf16(v) for v in docs]), q
    reg.drop(st.name)


def test_search_filtered_takes_the_lists(store, monkeypatch):
    from rfx import store as rstore
    from rfx.quality import recall_at_k
    reg, st, all_rows, q = store
    monkeypatch.setenv("RFX_IVF_FILTERED", "auto")
    assert rstore.ivf_filter_nprobe(NPROBE, NLIST, 1500, 4500, "auto") == 24 == st.filtered_nprobe(T0)
    s, r, path = st.search_filtered(q, 10, T0)
    assert path == "ivf"
    s, r = s.numpy(), r.numpy()
    assert (r >= 0).all() and (r < 1500).all(), "a row outside the filter (or a deleted one) came back"

    # the same call, spelled out: bit for bit
    mask = st.row_mask(T0)
    with st.lock:
        ds, dr = st.ivf.search_index(q, 10, 24, st.index, rerank_k=20, row_mask=mask)
    assert np.array_equal(dr.cpu().numpy(), r) and np.array_equal(ds.cpu().numpy().view(np.uint32), s.view(np.uint32))

    # the CPU reference's recall on the same rows, first
    x = oivf.stored_to_f32(all_rows, "bf16")
    codes, inv = oivf.quantize(x)
    qc = st.ivf.centroids()[0].cpu().numpy()
    fc = oivf.centroid_factor(qc)
    lab = oivf.assign(codes, qc, fc)
    q32 = oivf.stored_to_f32(to_np_bf16(q), "bf16")
    qq, qinv = oivf.quantize(q32)
    sel = np.zeros(6000, dtype=bool)
    sel[:1500] = True
    _, cand = mr.search(qq, qinv, codes, inv, lab, qc, fc, 24, 20, sel)
    rows64, q64 = x.astype(np.float64), q32.astype(np.float64)
    _, ref_r = oivf.rerank(cand, q64, rows64, 10)
    exact_r = np.argsort(-(q64 @ rows64[:1500].T), axis=1, kind="stable")[:, :10]  # the exact filtered top-10
    ref_recall = recall_at_k(ref_r.tolist(), exact_r.tolist(), 10)
    print(f"CPU reference recall@10 (t0, nprobe 24 of 32): {ref_recall:.4f}")
    assert ref_recall >= 0.9, ref_recall

    xs, xr = st.index.search(q, 10, row_mask=mask)
    got = recall_at_k(r.tolist(), xr.cpu().tolist(), 10)
    print(f"GPU recall@10 against the exact masked scan: {got:.4f}")
    assert got >= ref_recall - 0.02, (got, ref_recall)
    for i in range(len(q)):
        assert np.all(np.abs(s[i] - rows64[r[i]] @ q64[i]) <= 1e-5) and np.all(np.diff(s[i]) <= 0)


def test_filter_without_a_file_and_the_default(store, monkeypatch):
    reg, st, _, q = store
    monkeypatch.setenv("RFX_IVF_FILTERED", "auto")
    assert st.row_mask({"tenant": "nobody"}) is None and st.filtered_nprobe({"tenant": "nobody"}) is None
    s, r, path = st.search_filtered(q, 10, {"tenant": "nobody"})
    assert path == "exact" and (r.numpy() == -1).all() and np.isneginf(s.numpy()).all()
    # the deleted tenant's file matches no live file either
    assert st.row_mask({"tenant": "t1"}) is None
    monkeypatch.delenv("RFX_IVF_FILTERED")  # the default: the exact masked scan, as LocalStore.search keeps it
    mask = st.row_mask(T0)
    s, r, path = st.search_filtered(q, 10, T0)
    xs, xr = st.index.search(q, 10, row_mask=mask)
    assert path == "exact" and torch.equal(r.cpu(), xr.cpu()) and torch.equal(s.cpu(), xs.cpu())
    fs, fr = st.search(q, 10, row_mask=mask)
    assert torch.equal(fr, xr) and torch.equal(fs, xs)


def test_retriever_reports_the_path(store, monkeypatch):
    from rfx.retriever import GpuRetriever
    reg, st, _, _ = store
    ret = GpuRetriever(registry=reg, dim=DIM, dtype="bf16")
    ret.batching = False
    monkeypatch.setenv("RFX_IVF_FILTERED", "auto")
    hits = ret.search([st.name], "word5 topic3", 5, metadata_filter=T0)
    assert ret.last_filter_path == "ivf" and len(hits) == 5 and all(h.row < 1500 for h in hits)
    monkeypatch.setenv("RFX_SEGMENTED", "0")  # the per-filter batch runner takes the lists too
    ret.last_filter_path = None
    hits0 = ret.search([st.name], "word5 topic3", 5, metadata_filter=T0)
    assert ret.last_filter_path == "ivf" and [h.row for h in hits0] == [h.row for h in hits]
    monkeypatch.delenv("RFX_SEGMENTED")
    assert ret.search([st.name], "word5 topic3", 5, metadata_filter={"tenant": "nobody"}) == []
    monkeypatch.delenv("RFX_IVF_FILTERED")
    ret.last_filter_path = None
    exact = ret.search([st.name], "word5 topic3", 5, metadata_filter=T0)
    assert ret.last_filter_path in ("segmented", "masked") and all(h.row < 1500 for h in exact)
