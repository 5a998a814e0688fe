"""GPU: hybrid candidates beyond 64 end to end (GpuRetriever.candidates(hybrid=), LocalGpuRag.retrieve(top_k > 64)) on
a temporary store of more than 64 chunks, against the hand composition of the three deep calls."""
import pytest
import torch

pytestmark = pytest.mark.gpu

PARTS = ["pump", "valve", "impeller", "belt", "filter", "sensor", "hose", "fan", "tank", "gasket", "bearing", "manual"]
PLACES = ["engine block", "hydraulic circuit", "regional warehouse", "free span", "service bay", "two wire bus"]
QUESTION = "where is the coolant pump impeller kept in the regional warehouse"
K = 100


@pytest.fixture(scope="module")
def rag(tmp_path_factory):
    from rfx import store as rstore
    from rfx.adapter import LocalGpuRag
    from rfx.retriever import GpuRetriever
    tmp = tmp_path_factory.mktemp("hybrid_deep")
    reg = rstore.StoreRegistry(root=str(tmp / "root"), device=0)
    ret = GpuRetriever(registry=reg, dtype="bf16")
    r = LocalGpuRag(ret, top_k=3)
    st = r.create_store("parts")
    for i in range(72):  # one chunk each
        p = tmp / f"doc{i}.txt"
        p.write_text(f"note {i}: the coolant {PARTS[i % 12]} number {i * 37} is kept near the {PLACES[i % 6]} "
                     f"and checked every {2 + i % 5} weeks")
        r.upload_file(st, str(p), display_name=f"doc{i}")
    assert reg.get(st).index.rows > 64
    return r, ret, reg, st, tmp


def _pairs(hits):
    return [(h.score, h.row) for h in hits]


def _by_hand(ret, store, alpha):
    """(dense answer, fused answer) as [(score, row)], composed from the three deep calls"""
    from rfx.embedder import featurize_texts
    from rfx.store import flat_search_deep
    lex = store.lexical()
    csr = featurize_texts([QUESTION], lex.V, lex.hash_seed)
    q = ret.embedder(store.dim).embed_csr(*csr, dtype=store.dtype)
    sd, rd0 = flat_search_deep(store.index, ret.embedder(store.dim).embed_texts([QUESTION], store.dtype), K, None)
    _, rd = flat_search_deep(store.index, q, K, None)
    _, rl = lex.search_deep(csr, K)
    s, r = lex.fuse_deep(rd, rl, K, alpha)
    torch.cuda.synchronize()
    keep = lambda ss, rr: [(a, b) for a, b in zip(ss[0].cpu().tolist(), rr[0].cpu().tolist()) if b >= 0]
    return keep(sd, rd0), keep(s, r)


def test_candidates_fuse_both_answers_at_depth(rag):
    r, ret, reg, st, _ = rag
    dense, fused = _by_hand(ret, reg.get(st), 0.5)
    got = _pairs(ret.candidates([st], QUESTION, K, hybrid=0.5))
    assert len(got) == 72 and got == fused and ret.last_hybrid == "store"
    assert _pairs(r.retrieve(QUESTION, [st], top_k=K, hybrid=0.5)) == fused
    assert [row for _, row in got] != [row for _, row in dense]  # the keyword half moved something
    # alpha 1: the dense candidates' rows in their order
    assert [h.row for h in ret.candidates([st], QUESTION, K, hybrid=1.0)] == [row for _, row in dense]
    # hybrid=None: today's answer exactly
    assert _pairs(ret.candidates([st], QUESTION, K, hybrid=None)) == dense
    assert _pairs(ret.candidates([st], QUESTION, K)) == dense and _pairs(r.retrieve(QUESTION, [st], top_k=K)) == dense


def test_an_ivf_store_is_refused(rag):
    from rfx import store as rstore
    from rfx.adapter import LocalGpuRag
    from rfx.retriever import HYBRID_ERROR, GpuRetriever
    _, _, _, _, tmp = rag
    ireg = rstore.StoreRegistry(root=str(tmp / "ivf"), device=0)
    ist = ireg.create("lists", 768, "bf16", spec={"kind": "ivf", "nlist": 16, "nprobe": 4, "train_min": 100000})
    irag = LocalGpuRag(GpuRetriever(registry=ireg, dtype="bf16"), top_k=3)
    irag.upload_file(ist.name, str(tmp / "doc0.txt"), display_name="doc0")
    with pytest.raises(ValueError, match=HYBRID_ERROR):
        irag.retrieve(QUESTION, [ist.name], top_k=K, hybrid=0.5)
