"""GPU: deep search on f32 stores (rfx_search_deep on an f32 index) — the exact top-k for k in
65..1024 against the f64 oracle (oracle.search.topk over the widened stored values, judged by check_topk with its
default tolerances)."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import search as osearch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def widen(t):
    return t.cpu().numpy().astype(np.float64)  # exact for f32


def make_index(rows_t):
    from rfx.index import DeviceIndex
    ix = DeviceIndex(rows_t.shape[1], "f32", 0)
    ix.add(rows_t)
    return ix


def synth(seed, rows, dim):
    from rfx.index import synth_rows
    return synth_rows(seed, 0, rows, dim, "f32", 0)


@functools.lru_cache(maxsize=2)
def synth_store(rows, dim):
    x = synth(11, rows, dim)
    return make_index(x), widen(x)


def check(ix, q, x64, k, allowed=None, mask=None):
    """The deep answer against the oracle over the rows of `allowed` (bool per row; None = all)."""
    q64 = widen(q)
    s, r = ix.search_deep(q, k, row_mask=mask)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    ref_s, ref_r = osearch.topk(q64, x64 if allowed is None else np.where(allowed[:, None], x64, np.nan), k)
    live = ref_r >= 0
    assert np.array_equal(r >= 0, live) and np.all(np.isneginf(s[~live])), "padding is (-inf, -1), at the end"
    probs = osearch.check_topk(s, r, ref_s, ref_r, lambda qi, rows: x64[rows] @ q64[qi])
    assert not probs, probs[:3]
    return r


# rows: under one tile, one range / many ranges; k: at and past a KB step, above the row count; nq: a lone question,
# a part of a group, a group and a part; every dim of 64 / 768 / 1024 with every KB (2, 24 and 32 blocks per tile,
# the ring wrapping at the tile boundary); dim 320: a tile of 10 blocks in 16 ring steps
GRID = [(70, 64, 1, 65), (70, 768, 17, 129), (70, 1024, 9, 1000), (1000, 64, 9, 129), (1000, 768, 1, 1024),
        (1000, 1024, 17, 128), (4113, 64, 17, 1000), (4113, 768, 9, 65), (4113, 768, 17, 1000), (4113, 1024, 1, 129),
        (4113, 320, 9, 128), (40001, 64, 1, 1024), (40001, 64, 9, 128), (40001, 768, 17, 128), (40001, 768, 9, 129),
        (40001, 1024, 17, 1024), (40001, 1024, 1, 65)]


@pytest.mark.parametrize("rows,dim,nq,k", GRID)
def test_grid(rows, dim, nq, k):
    ix, x64 = synth_store(rows, dim)
    check(ix, synth(12, nq, dim), x64, k)


@pytest.mark.parametrize("k", [128, 1024])
def test_ties(k):
    x = synth(21, 5000, 768)
    x[1000:1300] = x[1000]
    x[2000:3100] = x[2000]
    q = torch.stack([x[1000], x[2000], x[7]])  # the two blocks as the best rows of a question each, and neither
    r = check(make_index(x), q, widen(x), k)
    assert np.array_equal(r[0, :min(k, 300)], np.arange(1000, 1000 + min(k, 300)))
    assert np.array_equal(r[1, :min(k, 1100)], np.arange(2000, 2000 + min(k, 1100)))


@pytest.mark.parametrize("rows,k", [(9000, 65), (9000, 1024), (70, 128)])
def test_all_equal(rows, k):
    q = synth(5, 3, 64)
    x = q[1:2].repeat(rows, 1).contiguous()
    r = check(make_index(x), q, widen(x), k)
    assert np.array_equal(r, np.tile(np.where(np.arange(k) < rows, np.arange(k), -1), (3, 1)))


@pytest.mark.parametrize("select", ["3%", "half", "all-but-one"])
def test_mask_and_tombstones(select):
    rows, k = 4113, 128
    x = synth(31, rows, 768)
    ix = make_index(x)
    rng = np.random.default_rng(3)
    dead = rng.choice(rows, 200, replace=False)
    ix.tombstone(dead)
    allowed = {"3%": rng.random(rows) < 0.03, "half": np.arange(rows) % 2 == 1,
               "all-but-one": np.arange(rows) != 4100}[select]
    words = np.packbits(np.pad(allowed, (0, -rows % 32)), bitorder="little").view(np.uint32).view(np.int32)
    x64 = widen(x)
    x64[dead] = np.nan
    q = synth(12, 9, 768)
    r = check(ix, q, x64, k, allowed, ix.mask_tensor(words))
    got = r[r >= 0]
    assert allowed[got].all() and not np.isin(got, dead).any()
    check(ix, q, x64, k)  # tombstones alone


@pytest.mark.parametrize("k", [65, 1024])
@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_order_edge(order, k):
    """Ascending scores: every row passes the threshold and the buffers are cut as often as possible; descending:
    one fill, nothing appended after it."""
    x, q = synth(41, 10000, 64), synth(12, 1, 64)
    o = np.argsort(widen(x) @ widen(q)[0], kind="stable")
    x = x[torch.from_numpy(o if order == "ascending" else o[::-1].copy()).to(x.device)].contiguous()
    check(make_index(x), q, widen(x), k)


def test_retriever(tmp_path, monkeypatch):
    from rfx import store as rstore
    from rfx.adapter import LocalGpuRag
    from rfx.retriever import DIVERSITY_ERROR, GpuRetriever
    with open(os.path.join(ROOT, "tests", "golden", "sample_report.md"), encoding="utf-8") as f:
        words = f.read().split()
    reg = rstore.StoreRegistry(root=str(tmp_path / "s"), device=0)
    ret = GpuRetriever(registry=reg, dtype="f32")
    rag = LocalGpuRag(ret, top_k=5)
    name = rag.create_store("reports")
    cfg = {"white_space_config": {"max_tokens_per_chunk": 3, "max_overlap_tokens": 1}}
    for i in range(36):  # every ninth of the report four times: more than 100 rows, and equal rows among them
        p = tmp_path / f"part{i}.md"
        p.write_text(" ".join(words[i % 9 * len(words) // 9:(i % 9 + 1) * len(words) // 9]), encoding="utf-8")
        rag.upload_file(name, str(p), display_name=p.name, chunking_config=cfg,
                        custom_metadata=[{"key": "tenant", "string_value": "abc"[i % 3]}])
    st, question, filt = reg.get(name), "source citations in chat answers", {"tenant": ["a", "c"]}
    assert st.dtype == "f32" and st.index.rows > 100
    with st.lock, torch.cuda.device(st.device):
        x64 = widen(st.index.read(0, st.index.rows))
        q64 = widen(ret.embedder(st.dim).embed_texts([question], st.dtype))
    allowed = np.zeros(len(x64), dtype=bool)
    for first, n in st.mask_ranges(filt):
        allowed[first:first + n] = True
    hits = ret.candidates([name], question, 200, metadata_filter=filt)
    assert hits == rag.retrieve(question, [name], metadata_filter=filt, top_k=200)
    ref_s, ref_r = osearch.topk(q64, np.where(allowed[:, None], x64, np.nan), 200)
    n = int((ref_r >= 0).sum())
    assert 0 < n == len(hits) < len(x64)
    got_s, got_r = np.array([[h.score for h in hits]], dtype=np.float32), np.array([[h.row for h in hits]])
    probs = osearch.check_topk(got_s, got_r, ref_s[:, :n], ref_r[:, :n], lambda qi, rows: x64[rows] @ q64[qi])
    assert not probs, probs[:3]
    monkeypatch.setenv("RFX_DEEP_SAMPLED", "1")  # the sampled scan is bf16 / f16: an f32 store keeps search_deep
    assert ret.candidates([name], question, 200, metadata_filter=filt) == hits
    monkeypatch.delenv("RFX_DEEP_SAMPLED")
    with pytest.raises(ValueError, match=DIVERSITY_ERROR):
        ret.candidates([name], question, 200, metadata_filter=filt, diversity=0.5)
    assert len(ret.candidates([name], question, 100, hybrid=0.5)) == 100
