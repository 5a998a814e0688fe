"""GPU: a retriever batch of filtered questions under DIFFERENT filters answered from an IVF store's posting lists
in ONE list search (LocalStore.search_lists_filtered_multi, RFX_IVF_MULTI).  The store is §4.15's
shape: 6,000 clustered rows in four files, three tenants, one deleted file, nlist 32, nprobe 8 — t0 2,000 rows,
t1 1,500 live (and the 1,500 deleted ones), t2 1,000, so the rule gives 18, 24 and 36 probes: under auto t2 is past
the cap of 32 and stays exact, under 1 it probes 32."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DIM, NLIST, NPROBE = 768, 32, 8
SPEC = {"kind": "ivf", "nlist": NLIST, "nprobe": NPROBE, "train_min": 4000}
T = [{"tenant": f"t{i}"} for i in range(3)]
SPAN = [(0, 2000), (2000, 3500), (3500, 4500)]  # t1's deleted file holds rows 4500 .. 5999


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from rfx import ivf as rivf
    from rfx import store as rstore
    from rfx.retriever import GpuRetriever
    reg = rstore.StoreRegistry(root=str(tmp_path_factory.mktemp("ivf-multi")), device=0)
    st = reg.create("ivf-multi", DIM, "bf16", spec=SPEC)
    for i, (tenant, n) in enumerate(((0, 2000), (1, 1500), (2, 1000), (1, 1500))):
        v = rivf.synth_clustered(7, 48, 100 + i, 1500 * i, n, DIM, "bf16")
        fid = st.add_document([f"d{i}-{j}" for j in range(n)], v, f"d{i}.md", {"tenant": f"t{tenant}"})[0]
    st.delete_file(fid)
    assert st.ivf_ready() and st.dead_rows() == 1500
    ret = GpuRetriever(registry=reg, dim=DIM, dtype="bf16")
    ret.batching = False
    yield reg, st, ret
    reg.drop(st.name)


def batch():
    """Nine questions in filter-group order, three per tenant; every group holds one at the batch's largest k."""
    ks = (10, 3, 7)
    return [(f"word{3 * t + j} topic{t + j}", ks[(t + j) % 3], T[t]) for t in range(3) for j in range(3)]


def rows_of(answers):
    return [list(a[2]) for a in answers]


def check_spans(items, answers):
    for (_, k, filt), a in zip(items, answers):
        lo, hi = SPAN[int(filt["tenant"][1])]
        r = np.array(a[2])
        assert len(r) == k and ((r >= lo) & (r < hi)).all(), "a row outside the filter (or a deleted one) came back"


def test_one_list_search_for_three_tenants(store, monkeypatch):
    reg, st, ret = store
    monkeypatch.setenv("RFX_IVF_FILTERED", "1")
    monkeypatch.delenv("RFX_IVF_MULTI", raising=False)
    assert [st.filtered_nprobe(f) for f in T] == [18, 24, 32]
    items = batch()
    out = ret._run_filtered_batch(st.name, items)
    assert ret.last_filter_path == "ivf" and ret.last_filter_list_searches == 1
    check_spans(items, out)
    # every answer is search_lists_filtered's for its filter at the batch's k (the same embedding call)
    with torch.cuda.device(st.device):
        q = ret.embedder(DIM).embed_texts([it[0] for it in items], st.dtype)
    for t in range(3):
        s, r = st.search_lists_filtered(q[3 * t:3 * t + 3].contiguous(), 10, T[t])
        for j in range(3):
            k = items[3 * t + j][1]
            assert r[j][:k].tolist() == list(out[3 * t + j][2])
            assert np.array_equal(np.array(out[3 * t + j][1], dtype=np.float32).view(np.uint32),
                                  s[j][:k].numpy().view(np.uint32))

    # RFX_IVF_MULTI=0: the per-group loop, the same answers at three list searches
    monkeypatch.setenv("RFX_IVF_MULTI", "0")
    out0 = ret._run_filtered_batch(st.name, items)
    assert ret.last_filter_path == "ivf" and ret.last_filter_list_searches == 3
    assert rows_of(out0) == rows_of(out) and [list(a[1]) for a in out0] == [list(a[1]) for a in out]


def test_one_group_keeps_the_one_mask_search(store, monkeypatch):
    """A batch from ONE tenant (a lone filtered question is the commonest): search_lists_filtered at the group's own
    k, as before — the per-question entry point would only add its table upload and launch."""
    reg, st, ret = store
    monkeypatch.setenv("RFX_IVF_FILTERED", "1")
    monkeypatch.delenv("RFX_IVF_MULTI", raising=False)
    calls = []
    one, multi = type(st).search_lists_filtered, type(st).search_lists_filtered_multi
    monkeypatch.setattr(type(st), "search_lists_filtered", lambda self, q, k, f: calls.append(("one", k)) or one(self, q, k, f))
    monkeypatch.setattr(type(st), "search_lists_filtered_multi",
                        lambda self, q, k, f: calls.append(("multi", k)) or multi(self, q, k, f))
    for items in (batch()[3:6], batch()[4:5]):  # three questions of t1 (k 3, 7, 10); one alone (k 7)
        calls.clear()
        out = ret._run_filtered_batch(st.name, items)
        assert ret.last_filter_path == "ivf" and ret.last_filter_list_searches == 1
        assert calls == [("one", max(it[1] for it in items))]
        check_spans(items, out)
        with torch.cuda.device(st.device):
            q = ret.embedder(DIM).embed_texts([it[0] for it in items], st.dtype)
        s, r = one(st, q, max(it[1] for it in items), T[1])
        for j, it in enumerate(items):
            assert r[j][:it[1]].tolist() == list(out[j][2])
    calls.clear()
    ret._run_filtered_batch(st.name, batch()[:6])  # two tenants: one list search for both
    assert calls == [("multi", 10)] and ret.last_filter_list_searches == 1


def test_a_declined_group_stays_exact(store, monkeypatch):
    reg, st, ret = store
    monkeypatch.setenv("RFX_IVF_FILTERED", "auto")
    monkeypatch.delenv("RFX_IVF_MULTI", raising=False)
    monkeypatch.setenv("RFX_SEGMENTED", "0")  # the declined group takes the masked scan: the call spelled out below
    assert [st.filtered_nprobe(f) for f in T] == [18, 24, None]  # t2: 36 probes > the cap of 32
    items = batch()
    out = ret._run_filtered_batch(st.name, items)
    assert ret.last_filter_list_searches == 1 and ret.last_filter_path == "masked"
    check_spans(items, out)
    with torch.cuda.device(st.device):
        q = ret.embedder(DIM).embed_texts([it[0] for it in items], st.dtype)
        q2 = ret.embedder(DIM).embed_texts([it[0] for it in items[6:]], st.dtype)
    s, r, declined = st.search_lists_filtered_multi(q, 10, [it[2] for it in items])
    assert declined == [6, 7, 8]
    for i in range(6):
        assert r[i][:items[i][1]].tolist() == list(out[i][2])
    xs, xr = st.index.search(q2, 10, row_mask=st.row_mask(T[2]))  # the declined group: the exact filtered top-k
    for j in range(3):
        assert xr[j][:items[6 + j][1]].tolist() == list(out[6 + j][2])


def test_default_keeps_every_filtered_question_exact(store, monkeypatch):
    reg, st, ret = store
    monkeypatch.delenv("RFX_IVF_FILTERED", raising=False)
    items = batch()
    out = ret._run_filtered_batch(st.name, items)
    assert ret.last_filter_list_searches == 0 and ret.last_filter_path in ("segmented", "masked")
    check_spans(items, out)
