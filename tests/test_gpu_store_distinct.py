"""GPU: distinct-document search end to end — a real LocalStore on disk behind LocalGpuRag: three
tenants, one file uploaded twice, with and without a filter, through a delete, an append and a compaction, from a
second store object, next to plain questions in other threads, and the default that changes nothing."""
import os
import threading

import numpy as np
import pytest
import torch

import distinct_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WS = {"white_space_config": {"max_tokens_per_chunk": 4, "max_overlap_tokens": 1}}  # about 3 chunks a file
QUESTIONS = ["document stores for authenticated users", "source citations in chat answers",
             "mock responses in demo mode"]
K = 5


def rule(st, ret, question, k, filt=None):
    """The rule's answer computed on the CPU from the store's own rows: [(row, file id)]."""
    with st.lock, torch.cuda.device(st.device):
        x64 = st.index.read(0, st.index.rows).float().cpu().numpy().astype(np.float64)  # tombstoned rows NaN
        q64 = ret.embedder(st.dim).embed_texts([question], st.dtype).float().cpu().numpy().astype(np.float64)
        row_doc = np.full(len(x64), -1, dtype=np.int32)
        for o, f in enumerate(st.files.values()):
            if not f["deleted"]:
                row_doc[f["first"]:f["first"] + f["n"]] = o
        allowed = ref._allowed(len(x64), st.mask_ranges(filt)) if filt is not None else None
        _, rows, _ = ref.reference(q64, x64, row_doc, k, allowed)
        return [(int(r), st.rows[r][0]) for r in rows[0] if r >= 0]


def test_store_end_to_end(tmp_path, monkeypatch):
    from rfx import store as rstore
    from rfx.adapter import LocalGpuRag
    from rfx.retriever import GpuRetriever, _BATCHERS, _DISTINCT

    monkeypatch.delenv("RFX_DISTINCT", raising=False)
    with open(os.path.join(ROOT, "tests", "golden", "sample_report.md"), encoding="utf-8") as f:
        words = f.read().split()
    parts = [" ".join(words[i * len(words) // 9:(i + 1) * len(words) // 9]) for i in range(9)]
    reg = rstore.StoreRegistry(root=str(tmp_path / "s"), device=0)
    ret = GpuRetriever(registry=reg, dtype="bf16")
    rag = LocalGpuRag(ret, top_k=K)
    assert rag.distinct is None
    name = rag.create_store("reports")
    ids = []

    def upload(i, title=None):
        p = tmp_path / f"part{i}.md"
        p.write_text(parts[i], encoding="utf-8")
        res = rag.upload_file(name, str(p), display_name=title or f"part{i}.md", chunking_config=WS,
                              custom_metadata=[{"key": "tenant", "string_value": "abc"[i % 3]}])
        ids.append(res.file_id)

    for i in range(8):
        upload(i)
    upload(0, "part0-again.md")  # the same file a second time: its rows tie with the first copy's
    st = reg.get(name)
    assert min(f["n"] for f in st.files.values()) >= 2, "every file is several chunks"

    def hits(q, r=rag, **kw):
        return [(h.row, h.file_id) for h in r.retrieve(q, [name], **kw)]

    def check_all(r=rag, ret_=ret, store=st):
        for q in QUESTIONS:
            for filt in (None, {"tenant": "a"}, {"tenant": ["b", "c"]}):
                kw = {} if filt is None else {"metadata_filter": filt}
                want = rule(store, ret_, q, K, filt)
                got = hits(q, r, distinct=True, **kw)
                assert got == want, (q, filt, got, want)
                assert len({fid for _, fid in got}) == len(got) == min(K, len(want))
                assert ret_.last_distinct_rounds >= 1

    # the plain answers, as the parent gives them: the k best chunks, some of one file
    plain = {q: [(h.score, h.row, h.file_id) for h in rag.retrieve(q, [name])] for q in QUESTIONS}
    for q in QUESTIONS:
        with torch.cuda.device(0):
            s, r = st.search(ret.embedder(st.dim).embed_texts([q], st.dtype), K)
        assert [(a, b) for a, b, _ in plain[q]] == list(zip(s[0].cpu().tolist(), r[0].cpu().tolist()))
    print("files among the plain top-5:", [len({fid for _, _, fid in p}) for p in plain.values()])

    for batching in (False, True):
        ret.batching = batching
        check_all()
    got = hits(QUESTIONS[0], distinct=True, k=9)
    assert len({fid for _, fid in got}) == 9 and got == rule(st, ret, QUESTIONS[0], 9)
    assert hits(QUESTIONS[0], distinct={"fetch_k": K}) == hits(QUESTIONS[0], distinct=True)
    both = {ids[0], ids[8]}  # the two copies are two documents: equal scores, the lower row first
    g = [fid for _, fid in hits(QUESTIONS[0], distinct=True, k=9)]
    assert abs(g.index(ids[0]) - g.index(ids[8])) == 1 and g.index(ids[0]) < g.index(ids[8]) and both <= set(g)
    # ask / ask_stream carry the keyword
    resp = rag.ask(contents=QUESTIONS[1], store_names=[name], metadata_filter=None, model="m", distinct=True)
    want_rows = [r for r, _ in hits(QUESTIONS[1], distinct=True)]
    assert [c.retrieved_context.row for c in resp.candidates[0].grounding_metadata.grounding_chunks] == want_rows
    last = list(rag.ask_stream(contents=QUESTIONS[1], store_names=[name], metadata_filter=None, model="m",
                               distinct=True))[-1]
    assert [c.retrieved_context.row for c in last.candidates[0].grounding_metadata.grounding_chunks] == want_rows

    # an append after the first distinct question (the cached row_doc is extended), then a delete, then a compaction
    p = tmp_path / "late.md"
    p.write_text(parts[8] + " " + QUESTIONS[0], encoding="utf-8")
    late = rag.upload_file(name, str(p), display_name="late.md", chunking_config=WS,
                           custom_metadata=[{"key": "tenant", "string_value": "a"}]).file_id
    assert st._row_docs["extended"] is False
    check_all()
    assert st._row_docs["extended"] is True
    assert late in [fid for _, fid in hits(QUESTIONS[0], distinct=True)]
    top = hits(QUESTIONS[0], distinct=True)[0][1]
    rag.delete_document_from_store(name, 1, file_id=top)
    check_all()
    assert top not in [fid for _, fid in hits(QUESTIONS[0], distinct=True, k=9)]
    # a second store object follows the writer
    reg2 = rstore.StoreRegistry(root=str(tmp_path / "s"), device=0)
    ret2 = GpuRetriever(registry=reg2, dtype="bf16")
    rag2 = LocalGpuRag(ret2, top_k=K)
    check_all(rag2, ret2, reg2.get(name))
    before = [fid for _, fid in hits(QUESTIONS[0], distinct=True)]
    out = rag.compact_store(name)
    assert out["rows"] < out["rows_before"]
    check_all()
    assert [fid for _, fid in hits(QUESTIONS[0], distinct=True)] == before, "the same files under the new numbering"
    check_all(rag2, ret2, reg2.get(name))

    # without the argument and without RFX_DISTINCT nothing changed: the plain answers of untouched files' rows
    for q in QUESTIONS:
        again = [(h.score, h.row, h.file_id) for h in rag.retrieve(q, [name])]
        with torch.cuda.device(0):
            s, r = st.search(ret.embedder(st.dim).embed_texts([q], st.dtype), K)
        assert [(a, b) for a, b, _ in again] == list(zip(s[0].cpu().tolist(), r[0].cpu().tolist()))
        assert hits(q, distinct=False) == [(b, c) for _, b, c in again]

    # RFX_DISTINCT=1: the default of an adapter built under it
    monkeypatch.setenv("RFX_DISTINCT", "1")
    rag3 = LocalGpuRag(ret, top_k=K)
    monkeypatch.delenv("RFX_DISTINCT")
    assert rag3.distinct is True and hits(QUESTIONS[2], rag3) == hits(QUESTIONS[2], distinct=True)
    assert hits(QUESTIONS[2], rag3, distinct=False) == hits(QUESTIONS[2])

    # concurrent distinct and plain questions never share a batch
    ret.batching = True
    seen = {"plain": [], "distinct": []}
    run_batch, run_distinct = ret._run_batch, ret._run_distinct_batch
    monkeypatch.setattr(ret, "_run_batch", lambda n, f, items: (seen["plain"].append(list(items)), run_batch(n, f, items))[1])
    monkeypatch.setattr(ret, "_run_distinct_batch",
                        lambda n, f, items: (seen["distinct"].append(list(items)), run_distinct(n, f, items))[1])
    solo = {(q, d): hits(q, distinct=d) for q in QUESTIONS for d in (True, False)}
    seen["plain"].clear(), seen["distinct"].clear()
    answers, errors = {}, []

    def ask(q, d, i):
        try:
            answers[(q, d, i)] = hits(q, distinct=d)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=ask, args=(q, d, i)) for i in range(4) for q in QUESTIONS for d in (True, False)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all(answers[(q, d, i)] == solo[(q, d)] for (q, d, i) in answers)
    assert seen["plain"] and all(len(it) == 2 for b in seen["plain"] for it in b)
    assert seen["distinct"] and all(len(it) == 3 and it[2] == 20 for b in seen["distinct"] for it in b)
    assert sum(len(b) for b in seen["plain"]) == sum(len(b) for b in seen["distinct"]) == 12
    assert any(isinstance(key[1], str) and key[1].startswith(_DISTINCT) for key in _BATCHERS)

    # two stores: each answers on its own, merged by score — never a union view
    name2 = rag.create_store("more")
    p.write_text(parts[3], encoding="utf-8")
    rag.upload_file(name2, str(p), display_name="other.md", chunking_config=WS)
    two = rag.retrieve(QUESTIONS[0], [name, name2], distinct=True)
    assert ret.last_path == "per-store" and len({(h.store, h.file_id) for h in two}) == K
    assert [h.score for h in two] == sorted((h.score for h in two), reverse=True)
    assert sum(h.store == name2 for h in two) <= 1

    # a sharded store refuses
    sreg = rstore.StoreRegistry(root=str(tmp_path / "s"), device=0, devices="0x2")
    srag = LocalGpuRag(GpuRetriever(registry=sreg, dtype="bf16"), top_k=K)
    with pytest.raises(ValueError, match="flat single-device store"):
        srag.retrieve(QUESTIONS[0], [name], distinct=True)
