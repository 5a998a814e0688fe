"""GPU: the sampled-threshold deep search (rfx_search_deep_sampled) against the f64 oracle, in the
pattern of tests/test_gpu_deep.py: oracle.search.topk over the widened stored values, judged by check_topk with
its default tolerances.  Every case also states how many questions took the fallback."""
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


def check(ix, q, q64, x64, k, fallbacks, allowed=None, mask=None):
    """The answer against the oracle over the rows of `allowed` (bool per row; None = all), and the fallback count."""
    s, r, fell = ix.search_deep_sampled(q, k, row_mask=mask, stats=True)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    ref_x = x64 if allowed is None else np.where(allowed[:, None], x64, np.nan)
    ref_s, ref_r = osearch.topk(q64, ref_x, k)
    live = ref_r >= 0
    assert np.array_equal(r >= 0, live) and np.all(np.isneginf(s[~live])), "padding is (-inf, -1), at the end"
    probs = osearch.check_topk(s, r, ref_s, ref_r, lambda qi, rows: x64[rows] @ q64[qi])
    assert not probs, probs[:3]
    assert fell == fallbacks, (fell, fallbacks)
    return r


def P(rows, dim, dtype, nq, k):
    return pytest.param(rows, dim, dtype, nq, k, id=f"{rows}x{dim}-{dtype}-nq{nq}-k{k}")


# rows: dense under one tile / dense or sampled by KB / sampled with stride 2-3 at KB <= 256 / sampled at every KB
# over many ranges; nq: the narrow form, 16 + 1 (one staged group of 4 waves), 64 + 1, 128 + 2 (the 8-wave form at
# dim <= 768); k: at and past a KB step
GRID = [
    P(70, 64, "bf16", 1, 65), P(70, 768, "f16", 17, 128), P(70, 1024, "bf16", 65, 1024), P(70, 768, "bf16", 130, 129),
    P(1000, 64, "f16", 17, 65), P(1000, 768, "bf16", 1, 128), P(1000, 768, "f16", 65, 129), P(1000, 1024, "f16", 130, 1000),
    P(1000, 64, "bf16", 130, 1024), P(1000, 1024, "bf16", 17, 128),
    P(4113, 64, "bf16", 1, 65), P(4113, 64, "f16", 130, 128), P(4113, 768, "bf16", 17, 128), P(4113, 768, "f16", 65, 129),
    P(4113, 768, "bf16", 130, 65), P(4113, 1024, "f16", 1, 1000), P(4113, 1024, "bf16", 65, 129), P(4113, 768, "f16", 1, 1024),
    P(4113, 1024, "bf16", 130, 256),
    P(40001, 64, "bf16", 17, 65), P(40001, 64, "f16", 65, 1024), P(40001, 768, "bf16", 1, 128), P(40001, 768, "f16", 17, 129),
    P(40001, 768, "bf16", 65, 1000), P(40001, 768, "f16", 130, 65), P(40001, 768, "bf16", 130, 1024),
    P(40001, 1024, "f16", 1, 1024), P(40001, 1024, "bf16", 17, 1000), P(40001, 1024, "f16", 65, 128),
    P(40001, 1024, "bf16", 130, 129),
]


@pytest.mark.parametrize("rows,dim,dtype,nq,k", GRID)
def test_grid(rows, dim, dtype, nq, k):
    from rfx.index import deep_plan, deep_sampled_plan
    ix, x64 = synth_store(rows, dim, dtype)
    q, q64 = queries(nq, dim, dtype)
    check(ix, q, q64, x64, k, 0)  # random stores stay under 0.61 of cap (DESIGN §4.20's simulation)
    _, S, _, cap, _, _ = deep_sampled_plan(rows, dim, dtype, nq, k)
    assert ix.deep_sampled_workspace_bytes(nq, k) >= nq * max(S, cap) * 8 + ix.deep_workspace_bytes(nq, k)


def rule_rows(q64, x64, k):
    """The ranking rule on the returned scores themselves: fl32 of the f64 dot, score desc, row asc."""
    s = (x64 @ q64.T).astype(np.float32).T
    return np.stack([np.lexsort((np.arange(x64.shape[0]), -si))[:k] for si in s])


def test_ties():
    """Blocks of identical rows at k 128: 1,100 equal scores stay under cap = 1,344, the order is the key's alone."""
    from rfx.index import deep_sampled_plan, synth_rows
    x = synth_rows(21, 0, 5000, 768, "bf16", 0)
    x[1000:1300] = x[1000]
    x[2000:3100] = x[2000]
    assert deep_sampled_plan(5000, 768, "bf16", 3, 128)[3] == 1344
    ix, x64 = make_index(x, "bf16"), widen(x)
    q = torch.stack([x[1000], x[2000], x[7]])
    q64 = widen(q)
    r = check(ix, q, q64, x64, 128, 0)
    assert np.array_equal(r, rule_rows(q64, x64, 128))
    assert np.array_equal(r[0], np.arange(1000, 1128)) and np.array_equal(r[1], np.arange(2000, 2128))


@pytest.mark.parametrize("k", [65, 1024])
def test_overflow(k):
    """All-equal scores: every row passes tau, every count passes cap, the fallback answers rows 0..k-1."""
    rows = 9000
    q, q64 = queries(3, 64, "f16", seed=5)
    x = q[1:2].repeat(rows, 1).contiguous()
    r = check(make_index(x, "f16"), q, q64, widen(x), k, 3)
    assert np.array_equal(r, np.tile(np.arange(k), (3, 1)))


def test_mixed_fallback():
    """The sample rows hold the negated question 0 and every other row question 0: its tau is the lowest score of
    the store and every row passes it, so it falls back.  Question 1 is random, on the side of the sample rows
    (q1 . q0 < 0): only the S <= cap sample rows reach its tau, and it does not."""
    from rfx.index import deep_sampled_plan, synth_rows
    rows, dim, k = 9000, 768, 128
    dense, S, stride, cap, _, _ = deep_sampled_plan(rows, dim, "bf16", 2, k)
    assert not dense and S <= cap < rows
    q = synth_rows(51, 0, 2, dim, "bf16", 0)
    if float(widen(q[0]) @ widen(q[1])) > 0:
        q[1] = -q[1]
    x = q[0:1].repeat(rows, 1).contiguous()
    x[torch.arange(S, device=x.device) * stride] = -q[0]
    check(make_index(x, "bf16"), q, widen(q), widen(x), k, 1)


@pytest.mark.parametrize("select", ["3%", "half", "all-but-one", "tombstones"])
def test_mask_and_tombstones(select):
    from rfx.index import synth_rows
    rows, k = 4113, 128
    x = synth_rows(31, 0, rows, 768, "bf16", 0)
    ix = make_index(x, "bf16")
    rng = np.random.default_rng(3)
    dead = rng.choice(rows, 200, replace=False)
    ix.tombstone(dead)
    x64 = widen(x)
    x64[dead] = np.nan
    q, q64 = queries(9, 768, "bf16")
    if select == "tombstones":
        r = check(ix, q, q64, x64, k, 0)
        assert not np.isin(r, dead).any()
        return
    allowed = {"3%": rng.random(rows) < 0.03,  # fewer than k eligible sample rows: tau is "none"
               "half": np.arange(rows) % 2 == 1, "all-but-one": np.arange(rows) != 4100}[select]
    words = np.packbits(np.pad(allowed, (0, -rows % 32)), bitorder="little").view(np.uint32).view(np.int32)
    r = check(ix, q, q64, x64, k, 0, allowed, ix.mask_tensor(words))
    got = r[r >= 0]
    assert allowed[got].all() and not np.isin(got, dead).any()


@pytest.mark.parametrize("k", [65, 1024])
@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_score_order(order, k):
    """Rows sorted by score: a strided sample sees the whole range of scores either way, so no fallback."""
    from rfx.index import synth_rows
    x = synth_rows(41, 0, 10000, 64, "f16", 0)
    q, q64 = queries(1, 64, "f16")
    o = np.argsort(widen(x) @ q64[0], kind="stable")
    x = x[torch.from_numpy(o if order == "ascending" else o[::-1].copy()).to(x.device)].contiguous()
    check(make_index(x, "f16"), q, q64, widen(x), k, 0)


def test_retriever(tmp_path, monkeypatch):
    from rfx import store as rstore
    from rfx.adapter import LocalGpuRag
    from rfx.index import DeviceIndex
    from rfx.retriever import GpuRetriever
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
    calls = []
    monkeypatch.setattr(DeviceIndex, "search_deep_sampled",
                        lambda self, *a, _f=DeviceIndex.search_deep_sampled, **kw: calls.append(1) or _f(self, *a, **kw))
    monkeypatch.delenv("RFX_DEEP_SAMPLED", raising=False)
    parent = ret.candidates([name], question, 200, metadata_filter=filt)
    assert not calls, "unset: the parent's call"
    monkeypatch.setenv("RFX_DEEP_SAMPLED", "1")
    hits = ret.candidates([name], question, 200, metadata_filter=filt)
    assert calls and hits == rag.retrieve(question, [name], metadata_filter=filt, top_k=200)
    with st.lock, torch.cuda.device(st.device):
        x64 = widen(st.index.read(0, st.index.rows))
        q64 = widen(ret.embedder(st.dim).embed_texts([question], st.dtype))
    allowed = np.zeros(len(x64), dtype=bool)
    for first, n in st.mask_ranges(filt):
        allowed[first:first + n] = True
    ref_s, ref_r = osearch.topk(q64, np.where(allowed[:, None], x64, np.nan), 200)
    n = int((ref_r >= 0).sum())
    assert 0 < n == len(hits) < len(x64) and len(parent) == n
    got_s, got_r = np.array([[h.score for h in hits]], dtype=np.float32), np.array([[h.row for h in hits]])
    probs = osearch.check_topk(got_s, got_r, ref_s[:, :n], ref_r[:, :n], lambda qi, rows: x64[rows] @ q64[qi])
    assert not probs, probs[:3]
