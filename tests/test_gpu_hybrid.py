"""GPU: hybrid retrieval end to end through LocalGpuRag on a temporary store root: the keyword case, the store's
lexical index against a LexIndex fed the same chunks, delete and compaction, a second process, a metadata filter,
batching, and the refused combinations."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import lex_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKEN = "zxq7714b"  # an invented part number: one document alone holds it
DOCS = [("pump", "the coolant pump housing is cast aluminium and bolts to the engine block with four studs"),
        ("valve", "a relief valve opens when the line pressure passes the rated limit of the hydraulic circuit"),
        ("part", f"replacement impeller for the coolant pump order part {TOKEN} from the regional warehouse"),
        ("belt", "the drive belt tension is checked with a gauge at the longest free span between pulleys"),
        ("filter", "replace the oil filter element at every second service and inspect the seal for cracks"),
        ("sensor", "the temperature sensor reports to the controller over the two wire bus every second"),
        ("hose", "coolant hoses are clamped at both ends and routed away from the exhaust manifold"),
        ("fan", "the radiator fan engages when the coolant temperature passes the thermostat set point"),
        ("tank", "the expansion tank holds the coolant that the warm engine pushes out of the radiator"),
        ("gasket", "a new head gasket is fitted dry and the bolts are tightened in the given sequence"),
        ("bearing", "the pump shaft runs in a sealed bearing that needs no grease for its service life"),
        ("manual", "the workshop manual lists every torque figure for the coolant pump and the housing")]
QUESTION = f"where do I order the impeller {TOKEN} for the coolant pump"


@pytest.fixture()
def rag(tmp_path):
    from rfx import store as rstore
    from rfx.adapter import LocalGpuRag
    from rfx.retriever import GpuRetriever
    reg = rstore.StoreRegistry(root=str(tmp_path / "root"), device=0)
    ret = GpuRetriever(registry=reg, dtype="bf16")
    r = LocalGpuRag(ret, top_k=3)
    st = r.create_store("parts")
    ids = {}
    for i, (name, text) in enumerate(DOCS):
        p = tmp_path / f"{name}.txt"
        p.write_text(text)
        ids[name] = r.upload_file(st, str(p), display_name=name,
                                  custom_metadata=[{"key": "team", "string_value": "a" if i % 2 else "b"}]).file_id
    return r, ret, reg, st, ids


def _hits(r, st, q=QUESTION, **kw):
    return [(h.score, h.row, h.title) for h in r.retrieve(q, [st] if isinstance(st, str) else st, **kw)]


def test_keyword_case(rag):
    r, ret, reg, st, _ = rag
    for batching in (False, True):
        ret.batching = batching
        plain = _hits(r, st)
        assert ret.last_hybrid is None
        assert _hits(r, st, hybrid=None) == plain  # today's answer exactly
        lexical = _hits(r, st, hybrid=0.0)
        assert ret.last_hybrid == "store" and ret.last_path == "per-store"
        assert lexical[0][2] == "part"
        assert [h[1] for h in _hits(r, st, hybrid=1.0)] == [h[1] for h in plain]
        # alpha 0.5: the reference, computed from the same candidate lists
        store = reg.get(st)
        lex = store.lexical()
        fetch = 16  # default_fetch_k(3)
        q = ret.embedder(store.dim).embed_texts([QUESTION], store.dtype)
        _, rd = store.index.search(q, fetch)
        _, rl = lex.search([QUESTION], fetch)
        rs, rr, _ = lex_ref.rrf(rd.cpu().numpy()[0], rl.cpu().numpy()[0], 3, 0.5)
        half = _hits(r, st, hybrid=0.5)
        assert [h[1] for h in half] == rr.tolist() and half[0][2] == "part"
        assert np.array_equal(np.asarray([h[0] for h in half], np.float32), rs)
        # ask / ask_stream carry the keyword
        resp = r.ask(contents=QUESTION, store_names=[st], metadata_filter=None, model="m", hybrid=0.0)
        assert TOKEN in r.extract_citations_from_response(resp)[0]["snippet"]
        last = list(r.ask_stream(contents=QUESTION, store_names=[st], metadata_filter=None, model="m", hybrid=0.0))[-1]
        assert TOKEN in r.extract_citations_from_response(last)[0]["snippet"]


def test_store_index_agrees_with_a_lexindex_fed_the_same_chunks(rag):
    from rfx.embedder import featurize_texts
    from rfx.lexical import LexIndex
    r, ret, reg, st, _ = rag
    store = reg.get(st)
    lex = store.lexical()
    own = LexIndex()
    own.add_csr(*featurize_texts([t for _, t in store.rows]))
    assert np.array_equal(lex.df(), own.df()) and lex.info() == own.info()
    for q in (QUESTION, "coolant pump housing", "torque figure"):
        a, b = lex.search([q], 5), own.search([q], 5)
        torch.cuda.synchronize()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    own.close()


def test_delete_and_compaction_keep_the_lexical_scores(rag):
    r, ret, reg, st, ids = rag
    ret.batching = False
    r.retrieve(QUESTION, [st], hybrid=0.0)  # the lexical index exists before the delete: it must follow it
    for name in ("valve", "pump"):
        r.delete_document_from_store(st, 0, file_id=ids[name])
    before = _hits(r, st, "coolant pump housing studs", k=5, hybrid=0.0)
    assert before and not {"valve", "pump"} & {h[2] for h in before}
    out = r.compact_store(st)
    assert out["rows"] < out["rows_before"]
    after = _hits(r, st, "coolant pump housing studs", k=5, hybrid=0.0)
    assert [(s, t) for s, _, t in after] == [(s, t) for s, _, t in before]  # the same scores and chunks
    assert [h[1] for h in after] != [h[1] for h in before]  # renumbered rows
    assert reg.get(st).lexical().rows == out["rows"]


CHILD = """
import json, sys
sys.path[:0] = [%r, %r]
from rfx import store as rstore
from rfx.adapter import LocalGpuRag
from rfx.retriever import GpuRetriever
reg = rstore.StoreRegistry(root=sys.argv[1], device=0)
rag = LocalGpuRag(GpuRetriever(registry=reg, dtype="bf16"), top_k=3)
print(json.dumps([[h.score, h.row, h.title] for h in rag.retrieve(sys.argv[3], [sys.argv[2]], hybrid=0.5)]))
"""


def test_a_second_process_gives_the_identical_answer(rag, tmp_path):
    r, ret, reg, st, _ = rag
    mine = _hits(r, st, hybrid=0.5)
    script = tmp_path / "child.py"
    script.write_text(CHILD % (ROOT, os.path.join(ROOT, "rag-foundation_amd")))
    p = subprocess.run([sys.executable, str(script), reg.root, st, QUESTION], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    theirs = [tuple(h) for h in json.loads(p.stdout.strip().splitlines()[-1])]
    assert theirs == mine


def test_a_metadata_filter_restricts_both_lists(rag):
    r, ret, reg, st, _ = rag
    titles_b = {name for i, (name, _) in enumerate(DOCS) if i % 2 == 0}  # "part" is document 2: team b
    for alpha in (0.0, 0.5, 1.0):
        got = _hits(r, st, k=8, metadata_filter={"team": "b"}, hybrid=alpha)
        assert got and {h[2] for h in got} <= titles_b
        other = _hits(r, st, k=8, metadata_filter={"team": "a"}, hybrid=alpha)
        assert "part" not in {h[2] for h in other} and not {h[2] for h in other} & titles_b
    assert _hits(r, st, metadata_filter={"team": "b"}, hybrid=0.0)[0][2] == "part"
    assert _hits(r, st, metadata_filter={"team": "nobody"}, hybrid=0.5) == []


def _queued(batcher):
    with batcher._lock:
        return len(batcher._queue)


def test_a_mixed_batch_matches_the_questions_alone(rag):
    """Hybrid questions with different alpha, k and fetch_k in ONE batch (the batch runner called with all five
    items: one dense and one lexical search at the largest fetch_k, one fusion with each item's own alpha and
    list lengths) are answered identically to the same questions asked alone; and concurrent callers through
    the batcher, with the batcher held busy so that they queue up, ride one batch of five."""
    from rfx.retriever import parse_hybrid
    r, ret, reg, st, _ = rag
    asks = [(QUESTION, 3, 0.0), ("coolant pump housing", 5, {"alpha": 0.5, "fetch_k": 8}),
            ("torque figure in the manual", 1, {"alpha": 0.25, "fetch_k": 64}), ("drive belt tension gauge", 4, 1.0),
            ("radiator fan thermostat", 2, {"alpha": 0.75, "fetch_k": 12})]
    ret.batching = False
    alone = [_hits(r, st, q, k=k, hybrid=h) for q, k, h in asks]
    items = [(q, k, parse_hybrid(h, k)) for q, k, h in asks]
    assert len({it[2][1] for it in items}) == 4 and len({it[1] for it in items}) == 5  # fetch_k 16, 8, 64, 12
    out = ret._run_hybrid_batch(st, None, items)
    for (q, k, _), ans, ref in zip(asks, out, alone):
        _, s, rows = ans
        assert len(s) == k and [(sc, row) for sc, row in zip(s, rows) if row >= 0] == [(h[0], h[1]) for h in ref], q

    # through the batcher: a first question occupies it (its batch runner waits on an event), five more queue up
    ret.batching = True
    sizes, started, release = [], threading.Event(), threading.Event()
    run = ret._run_hybrid_batch

    def gated(n, f, its):
        sizes.append(len(its))
        if len(sizes) == 1:
            started.set()
            assert release.wait(60)
        return run(n, f, its)

    ret._run_hybrid_batch = gated
    got = [None] * len(asks)

    def ask(i):
        q, k, h = asks[i]
        got[i] = _hits(r, st, q, k=k, hybrid=h)

    first = threading.Thread(target=lambda: _hits(r, st, "expansion tank", k=2, hybrid=0.5))
    first.start()
    assert started.wait(60)
    threads = [threading.Thread(target=ask, args=(i,)) for i in range(len(asks))]
    for t in threads:
        t.start()
    b = ret._hybrid_batcher(st, None, items[0][2])
    for _ in range(2000):  # until all five are queued behind the running batch
        if _queued(b) >= len(asks):
            break
        threading.Event().wait(0.005)
    release.set()
    first.join()
    for t in threads:
        t.join()
    assert got == alone
    assert sizes == [1, len(asks)], sizes


def test_refused_combinations(rag, tmp_path):
    from rfx import store as rstore
    from rfx.adapter import LocalGpuRag
    from rfx.retriever import HYBRID_ERROR, GpuRetriever
    r, ret, reg, st, _ = rag
    with pytest.raises(ValueError, match=HYBRID_ERROR):
        r.retrieve(QUESTION, [st], hybrid=0.5, diversity=0.5)
    for bad in (1.5, -0.1, float("nan"), {"fetch_k": 8}, {"alpha": 0.5, "fetch_k": 2}, {"alpha": 0.5, "rrf_c": 0},
                {"alpha": 0.5, "b": 2.0}, {"alpha": 0.5, "k1": -1.0}, {"alpha": 0.5, "beta": 1}):
        with pytest.raises(ValueError):
            r.retrieve(QUESTION, [st], hybrid=bad)
    ireg = rstore.StoreRegistry(root=str(tmp_path / "ivf"), device=0)
    ist = ireg.create("lists", 768, "bf16", spec={"kind": "ivf", "nlist": 16, "nprobe": 4, "train_min": 100000})
    irag = LocalGpuRag(GpuRetriever(registry=ireg, dtype="bf16"), top_k=3)
    p = tmp_path / "d.txt"
    p.write_text(DOCS[2][1])
    irag.upload_file(ist.name, str(p), display_name="part")
    assert irag.retrieve(QUESTION, [ist.name])
    with pytest.raises(ValueError, match=HYBRID_ERROR):
        irag.retrieve(QUESTION, [ist.name], hybrid=0.5)
    # RFX_HYBRID_ALPHA: the default alpha of an adapter
    os.environ["RFX_HYBRID_ALPHA"] = "0.0"
    try:
        r2 = LocalGpuRag(ret, top_k=3)
    finally:
        del os.environ["RFX_HYBRID_ALPHA"]
    assert r2.hybrid == 0.0 and r.hybrid is None
    assert _hits(r2, st) == _hits(r, st, hybrid=0.0)
