"""GPU: deep search (rfx_search_deep) — the exact top-k for k in 65..1024 against the f64 oracle
(oracle.search.topk over the widened stored values, judged by check_topk with its default tolerances)."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import search as osearch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def widen(t):
    return t.float().cpu().numpy().astype(np.float64)  # exact for bf16 / f16


def make_index(rows_t, dtype):
    from rfx.index import DeviceIndex
    ix = DeviceIndex(rows_t.shape[1], dtype, 0)
    ix.add(rows_t)
    return ix


@functools.lru_cache(maxsize=2)
def synth_store(rows, dim, dtype):
    from rfx.index import synth_rows
    x = synth_rows(11, 0, rows, dim, dtype, 0)
    return make_index(x, dtype), widen(x)


def queries(nq, dim, dtype, seed=12):
    from rfx.index import synth_rows
    q = synth_rows(seed, 0, nq, dim, dtype, 0)
    return q, widen(q)


def check(ix, q, q64, x64, k, allowed=None, mask=None):
    """The deep answer against the oracle over the rows of `allowed` (bool per row; None = all)."""
    s, r = ix.search_deep(q, k, row_mask=mask)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    ref_x = x64 if allowed is None else np.where(allowed[:, None], x64, np.nan)
    ref_s, ref_r = osearch.topk(q64, ref_x, k)
    live = ref_r >= 0
    assert np.array_equal(r >= 0, live) and np.all(np.isneginf(s[~live])), "padding is (-inf, -1), at the end"
    probs = osearch.check_topk(s, r, ref_s, ref_r, lambda qi, rows: x64[rows] @ q64[qi])
    assert not probs, probs[:3]
    return r, ref_r


def P(rows, dim, dtype, nq, k):
    return pytest.param(rows, dim, dtype, nq, k, id=f"{rows}x{dim}-{dtype}-nq{nq}-k{k}")


# rows: under one tile multiple, one range / many ranges; k: at and past a KB step, above the row count; nq: a lone
# question, a part of a group, a group and a part (17 = 16 + 1 at KB <= 512, 8 + 8 + 1 at KB 1024)
GRID = [
    P(70, 64, "bf16", 1, 65), P(70, 64, "f16", 9, 128), P(70, 768, "bf16", 17, 129), P(70, 768, "f16", 1, 1000),
    P(70, 64, "bf16", 17, 1024), P(70, 768, "f16", 9, 65),
    P(1000, 64, "bf16", 9, 65), P(1000, 64, "f16", 17, 128), P(1000, 64, "f16", 1, 129), P(1000, 64, "bf16", 1, 1000),
    P(1000, 64, "f16", 9, 1024), P(1000, 768, "bf16", 1, 128), P(1000, 768, "bf16", 17, 1000), P(1000, 768, "f16", 9, 129),
    P(1000, 768, "f16", 17, 65), P(1000, 768, "bf16", 9, 1024),
    P(4113, 64, "bf16", 17, 65), P(4113, 64, "bf16", 1, 128), P(4113, 64, "f16", 9, 129), P(4113, 64, "f16", 17, 1000),
    P(4113, 64, "bf16", 9, 1024), P(4113, 768, "bf16", 9, 65), P(4113, 768, "f16", 1, 128), P(4113, 768, "bf16", 17, 129),
    P(4113, 768, "f16", 9, 1000), P(4113, 768, "f16", 1, 1024), P(4113, 768, "bf16", 1, 1000),
    P(40001, 64, "bf16", 1, 65), P(40001, 64, "f16", 17, 128), P(40001, 64, "bf16", 9, 129), P(40001, 64, "f16", 1, 1000),
    P(40001, 64, "bf16", 17, 1024), P(40001, 768, "bf16", 17, 65), P(40001, 768, "bf16", 9, 128), P(40001, 768, "f16", 1, 129),
    P(40001, 768, "f16", 17, 1000), P(40001, 768, "bf16", 1, 1024), P(40001, 768, "f16", 9, 1024),
    P(40001, 768, "bf16", 9, 1000), P(40001, 768, "f16", 17, 129),
]


@pytest.mark.parametrize("rows,dim,dtype,nq,k", GRID)
def test_grid(rows, dim, dtype, nq, k):
    ix, x64 = synth_store(rows, dim, dtype)
    q, q64 = queries(nq, dim, dtype)
    check(ix, q, q64, x64, k)


def rule_rows(q64, x64, k):
    """The ranking rule on the returned scores themselves: fl32 of the f64 dot, score desc, row asc."""
    s = (x64 @ q64.T).astype(np.float32).T
    return np.stack([np.lexsort((np.arange(x64.shape[0]), -si))[:k] for si in s])


@pytest.mark.parametrize("k", [128, 1024])
def test_ties(k):
    from rfx.index import synth_rows
    x = synth_rows(21, 0, 5000, 768, "bf16", 0)
    x[1000:1300] = x[1000]
    x[2000:3100] = x[2000]
    ix, x64 = make_index(x, "bf16"), widen(x)
    q = torch.stack([x[1000], x[2000], x[7]])  # the two blocks as the best rows of a question each, and neither
    q64 = widen(q)
    r, _ = check(ix, q, q64, x64, k)
    assert np.array_equal(r, rule_rows(q64, x64, k))
    assert np.array_equal(r[0, :min(k, 300)], np.arange(1000, 1000 + min(k, 300)))
    assert np.array_equal(r[1, :min(k, 1100)], np.arange(2000, 2000 + min(k, 1100)))


@pytest.mark.parametrize("rows,k", [(9000, 65), (9000, 1024), (70, 128)])
def test_all_equal(rows, k):
    q, q64 = queries(3, 64, "f16", seed=5)
    x = q[1:2].repeat(rows, 1).contiguous()
    r, _ = check(make_index(x, "f16"), q, q64, widen(x), k)
    want = np.where(np.arange(k) < rows, np.arange(k), -1)
    assert np.array_equal(r, np.tile(want, (3, 1)))


@pytest.mark.parametrize("select", ["3%", "half", "all-but-one"])
def test_mask_and_tombstones(select):
    from rfx.index import synth_rows
    rows, k = 4113, 128
    x = synth_rows(31, 0, rows, 768, "bf16", 0)
    ix = make_index(x, "bf16")
    rng = np.random.default_rng(3)
    dead = rng.choice(rows, 200, replace=False)
    ix.tombstone(dead)
    allowed = {"3%": rng.random(rows) < 0.03, "half": np.arange(rows) % 2 == 1,
               "all-but-one": np.arange(rows) != 4100}[select]
    words = np.packbits(np.pad(allowed, (0, -rows % 32)), bitorder="little").view(np.uint32).view(np.int32)
    x64 = widen(x)
    x64[dead] = np.nan
    q, q64 = queries(9, 768, "bf16")
    r, _ = check(ix, q, q64, x64, k, allowed, ix.mask_tensor(words))
    got = r[r >= 0]
    assert allowed[got].all() and not np.isin(got, dead).any()
    check(ix, q, q64, x64, k)  # tombstones alone


@pytest.mark.parametrize("k", [65, 1024])
@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_compaction_edge(order, k):
    """Ascending scores: every row passes the threshold and the buffers are cut as often as possible; descending:
    one fill, nothing appended after it."""
    from rfx.index import synth_rows
    x = synth_rows(41, 0, 10000, 64, "f16", 0)
    q, q64 = queries(1, 64, "f16")
    o = np.argsort(widen(x) @ q64[0], kind="stable")
    x = x[torch.from_numpy(o if order == "ascending" else o[::-1].copy()).to(x.device)].contiguous()
    check(make_index(x, "f16"), q, q64, widen(x), k)


def test_retriever(tmp_path):
    from rfx import store as rstore
    from rfx.adapter import LocalGpuRag
    from rfx.retriever import DEEP_ERROR, GpuRetriever
    with open(os.path.join(ROOT, "tests", "golden", "sample_report.md"), encoding="utf-8") as f:
        words = f.read().split()
    reg = rstore.StoreRegistry(root=str(tmp_path / "s"), device=0)
    ret = GpuRetriever(registry=reg, dtype="bf16")
    rag = LocalGpuRag(ret, top_k=5)
    name = rag.create_store("reports")
    cfg = {"white_space_config": {"max_tokens_per_chunk": 4, "max_overlap_tokens": 1}}
    for i in range(9):
        p = tmp_path / f"part{i}.md"
        p.write_text(" ".join(words[i * len(words) // 9:(i + 1) * len(words) // 9]), encoding="utf-8")
        rag.upload_file(name, str(p), display_name=p.name, chunking_config=cfg,
                        custom_metadata=[{"key": "tenant", "string_value": "abc"[i % 3]}])
    st, question, filt = reg.get(name), "source citations in chat answers", {"tenant": ["a", "c"]}
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
    assert ret.candidates([name], question, 10, metadata_filter=filt) == ret.search([name], question, 10, filt)
    with pytest.raises(ValueError):
        ret.candidates([name], question, 1025)

    ireg = rstore.StoreRegistry(root=str(tmp_path / "ivf"), device=0)
    ist = ireg.create("lists", 768, "bf16", spec={"kind": "ivf", "nlist": 16, "nprobe": 4, "train_min": 100000})
    irag = LocalGpuRag(GpuRetriever(registry=ireg, dtype="bf16"), top_k=3)
    irag.upload_file(ist.name, str(tmp_path / "part0.md"), display_name="part")
    with pytest.raises(ValueError, match=DEEP_ERROR):
        irag.retrieve(question, [ist.name], top_k=100)
