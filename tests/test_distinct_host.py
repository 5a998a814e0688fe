"""Host (no GPU): distinct-document search — the exported symbol, the range subtraction, the
rounds of rfx.distinct.run_rounds against numpy stand-ins for the device operations, two mutants the corpora
are built to catch, the properties the corpora are named for, LocalStore.row_docs over host stand-ins, the
`distinct` argument and the refusals."""
import numpy as np
import pytest

import distinct_ref as ref
from fakes import HostIndex

D = 64
_CORPORA = {}


def corpus(name):
    if name not in _CORPORA:
        _CORPORA[name] = ref.build(name, D)
    return _CORPORA[name]


def fetch_of(c):
    from rfx import distinct
    return c.fetch_k or distinct.default_fetch_k(c.k)


def test_symbol_exported_and_declared():
    from rfx import _lib
    assert "rfx_distinct_collapse" in _lib.SIGNATURES
    assert hasattr(_lib.lib, "rfx_distinct_collapse")
    with open(_lib.CSRC + "/../../include/rfx.h", encoding="utf-8") as f:
        assert "int rfx_distinct_collapse(" in f.read()


# ---- subtract_ranges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranges,minus,want", [
    ([], [], []),
    ([], [(0, 5)], []),
    ([(0, 10)], [], [(0, 10)]),
    ([(0, 10)], [(0, 0), (3, 0)], [(0, 10)]),                          # empty ranges are skipped
    ([(0, 10)], [(0, 10)], []),                                         # the whole range
    ([(0, 10)], [(0, 30)], []),
    ([(5, 10)], [(0, 5)], [(5, 10)]),                                   # touching below
    ([(5, 10)], [(15, 5)], [(5, 10)]),                                  # touching above
    ([(5, 10)], [(5, 3)], [(8, 7)]),                                    # nested at the lower edge
    ([(5, 10)], [(12, 3)], [(5, 7)]),                                   # nested at the upper edge
    ([(5, 10)], [(7, 2)], [(5, 2), (9, 6)]),                            # nested inside
    ([(5, 10)], [(3, 4), (9, 1), (14, 9)], [(7, 2), (10, 4)]),
    ([(0, 4), (4, 4), (10, 5)], [(2, 9)], [(0, 2), (11, 4)]),           # one minus range over several ranges
    ([(0, 4), (10, 5), (20, 5)], [(1, 1), (3, 8), (24, 1)], [(0, 1), (2, 1), (11, 4), (20, 4)]),
])
def test_subtract_ranges(ranges, minus, want):
    from rfx import filters
    got = filters.subtract_ranges(ranges, minus)
    assert got == want
    # against sets of rows
    rows = lambda rg: {r for f, n in rg for r in range(f, f + n)}
    assert rows(got) == rows(ranges) - rows(minus)


@pytest.mark.parametrize("ranges,minus", [([(10, 5), (0, 5)], []), ([(0, 20)], [(8, 2), (3, 2)]),
                                          ([(0, 5), (4, 5)], []), ([(0, 20)], [(3, 5), (7, 2)]),
                                          ([(-1, 5)], []), ([(0, 5)], [(2, -1)])])
def test_subtract_ranges_refuses_unsorted_or_overlapping(ranges, minus):
    from rfx import filters
    with pytest.raises(ValueError):
        filters.subtract_ranges(ranges, minus)


# ---- the corpora have the properties they are named for --------------------------------------------------------
def test_corpus_properties():
    for name in ("plain", "holes"):  # the best fetch_k rows hold k files: the first search suffices
        c = corpus(name)
        assert min(c.files_in_best(fetch_of(c))) >= c.k, name
    c = corpus("dominant")
    assert max(c.files_in_best(64)) < c.k and max(c.files_in_best(64)) == 1
    c = corpus("dominant2")
    dom = [o for o, (_, n, _) in enumerate(c.files) if n == 200]
    for _, r in ref.ranking(c.q64, c.x64):  # the best 200 rows are the first file's, the next 200 the second's
        assert set(c.row_doc[r[:200]]) == {dom[0]} and set(c.row_doc[r[200:400]]) == {dom[1]}
    c = corpus("dups")
    for s, r in ref.ranking(c.q64, c.x64):
        assert len(set(s[:68].tolist())) == 1, "68 rows tie for the first place: Z, 64 of A, two of C, D"
        assert r[:68].tolist() == [1] + list(range(3, 67)) + [67, 69, 70]
        # the tie crosses the rank-64 edge: the best 64 rows hold Z and A alone, C and D come after them
        assert set(c.row_doc[r[:64]].tolist()) == {0, 1} and c.row_doc[r[64:68]].tolist() == [1, 2, 2, 3]
    c = corpus("few")
    assert len(c.files) == 3 and len(c.rows) < fetch_of(c) and c.k == 10
    c = corpus("few_big")
    assert len(c.files) == 3 and len(c.rows) > 64 and min(c.files_in_best(fetch_of(c))) == 3
    c = corpus("holes")
    dead = [o for o, f in enumerate(c.files) if f[2]]
    assert dead[0] == 0 and dead[-1] == len(c.files) - 1 and len(dead) == 4
    raw = c.rows.astype(np.float64)  # were they alive, the deleted files would own the best rows
    assert all(set(np.argsort(-(raw @ q))[:8]) <= set(c.dead_rows) for q in c.q64)


# ---- the rounds against numpy stand-ins ----------------------------------------------------------------------------
@pytest.mark.parametrize("refuse", [False, True])
@pytest.mark.parametrize("name", ref.CORPORA)
def test_rounds_equal_the_reference(name, refuse):
    from rfx import distinct
    c = corpus(name)
    ops = ref.NumpyOps(c, c.k, fetch_of(c), refuse_segmented=refuse)
    rounds = distinct.run_rounds(ops, len(c.queries), c.k, len(c.rows), c.doc_ranges)
    want = ref.reference(c.q64, c.x64, c.row_doc, c.k)
    for got, w in zip(ops.out[:3], want):
        assert np.array_equal(got, w), name
    assert rounds == c.rounds, (name, rounds)
    assert len([x for x in ops.calls if x[0] == ("masked" if refuse else "segmented")]) == c.rounds - 1
    if name in ("few", "few_big"):
        assert (ops.out[1][:, 3:] == -1).all() and (ops.out[1][:, :3] >= 0).all()


@pytest.mark.parametrize("name", ["dominant", "dups", "holes", "plain"])
def test_rounds_under_a_filter(name):
    from rfx import distinct, filters
    c = corpus(name)
    keep = [o for o, f in enumerate(c.files) if o % 3 != 2 and not f[2]]  # two files of three
    sel = filters.subtract_ranges([(0, len(c.rows))],
                                  [(f0, n) for o, (f0, n, _) in enumerate(c.files) if o not in keep])
    allowed = ref._allowed(len(c.rows), sel)
    ops = ref.NumpyOps(c, c.k, fetch_of(c), allowed=allowed)
    distinct.run_rounds(ops, len(c.queries), c.k, len(c.rows), c.doc_ranges, select_ranges=sel)
    want = ref.reference(c.q64, c.x64, c.row_doc, c.k, allowed)
    for got, w in zip(ops.out[:3], want):
        assert np.array_equal(got, w), name
    assert set(ops.out[2].ravel().tolist()) <= set(keep) | {-1}


def test_rounds_are_bounded():
    """Candidates that never add a document and never run out: the loop stops with an error, it does not spin."""
    from rfx import distinct
    c = corpus("dominant")

    class Stuck(ref.NumpyOps):
        def segmented(self, open_q, ranges):  # the rows of the dominant file again
            return ref.np_search(self.c.q64, self.c.x64, 64)

    with pytest.raises(RuntimeError):
        distinct.run_rounds(Stuck(c, c.k, 40), len(c.queries), c.k, len(c.rows), c.doc_ranges)


def test_mutants_are_caught():
    c = corpus("dominant")
    want = ref.reference(c.q64, c.x64, c.row_doc, c.k)
    assert not np.array_equal(ref.mutant_first64(c, c.k)[1], want[1])
    c = corpus("dups")
    want = ref.reference(c.q64, c.x64, c.row_doc, c.k)
    assert not np.array_equal(ref.mutant_first64(c, c.k)[1], want[1])
    assert not np.array_equal(ref.mutant_ignores_ties(c, c.k), want[1])
    assert want[1][0, :4].tolist() == [1, 3, 67, 70], "Z, A, the LOWER of C's two copies, D"
    c = corpus("plain")  # and where nothing ties, the tie mutant is the rule
    assert np.array_equal(ref.mutant_ignores_ties(c, c.k), ref.reference(c.q64, c.x64, c.row_doc, c.k)[1])


# ---- LocalStore.row_docs over host stand-ins ---------------------------------------------------------------------
def vecs(n, seed):
    return np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)


class CompactingIndex(HostIndex):
    def compact(self, ranges):
        keep = np.concatenate([np.arange(f, f + n) for f, n in ranges]) if ranges else np.zeros(0, dtype=np.int64)
        self.data = self.data[keep]
        return int(keep.size)


def test_row_docs_extends_rebuilds_and_renumbers(tmp_path):
    from rfx import store as rstore
    reg = rstore.StoreRegistry(root=str(tmp_path), device=0, index_factory=CompactingIndex)
    st = reg.create("demo", D, "f32")
    ids = [st.add_document([f"{i}{j}" for j in range(n)], vecs(n, i), f"{i}.md")[0] for i, n in enumerate((3, 2, 4))]
    row_doc, ranges, fids = st.row_docs()
    assert row_doc.tolist() == [0, 0, 0, 1, 1, 2, 2, 2, 2] and row_doc.dtype == np.int32
    assert ranges.tolist() == [[0, 3], [3, 2], [5, 4]] and fids == ids
    assert st.row_docs()[0] is row_doc, "cached per (generation, version)"
    assert st._row_docs["extended"] is False

    # an append extends the cached copy with the new rows only
    ids.append(st.add_document(["a", "b"], vecs(2, 7), "3.md")[0])
    ids.append(st.add_document([], vecs(0, 8), "empty.md")[0])
    row_doc2, ranges2, fids2 = st.row_docs()
    assert st._row_docs["extended"] is True
    assert row_doc2.tolist() == [0, 0, 0, 1, 1, 2, 2, 2, 2, 3, 3]
    assert ranges2.tolist() == [[0, 3], [3, 2], [5, 4], [9, 2], [11, 0]] and fids2 == ids

    # a second store object follows the writer's commits
    reader = rstore.StoreRegistry(root=str(tmp_path), device=0, index_factory=CompactingIndex).get(st.name)
    assert reader.row_docs()[0].tolist() == row_doc2.tolist()

    # a delete rebuilds: the rows of the deleted file are -1, the ordinals stay
    st.delete_file(ids[1])
    row_doc3, ranges3, fids3 = st.row_docs()
    assert st._row_docs["extended"] is False
    assert row_doc3.tolist() == [0, 0, 0, -1, -1, 2, 2, 2, 2, 3, 3] and fids3 == ids
    assert reader.refresh() and reader.row_docs()[0].tolist() == row_doc3.tolist()

    # an append after the delete extends again (no new delete since the cached copy)
    ids.append(st.add_document(["z"], vecs(1, 9), "5.md")[0])
    assert st.row_docs()[0].tolist() == [0, 0, 0, -1, -1, 2, 2, 2, 2, 3, 3, 5]
    assert st._row_docs["extended"] is True

    # a compaction renumbers: the deleted file is gone, ordinals are positions in the new file table
    st.compact()
    row_doc4, ranges4, fids4 = st.row_docs()
    assert row_doc4.tolist() == [0, 0, 0, 1, 1, 1, 1, 2, 2, 4]
    assert fids4 == [ids[0], ids[2], ids[3], ids[4], ids[5]]
    assert ranges4.tolist() == [[0, 3], [3, 4], [7, 2], [9, 0], [9, 1]]
    assert reader.refresh() and reader.row_docs()[0].tolist() == row_doc4.tolist()
    assert reader.row_docs()[2] == fids4


# ---- the argument and the refusals -----------------------------------------------------------------------------------
def test_distinct_argument():
    from rfx import distinct
    assert distinct.parse_distinct(None, 5) is None and distinct.parse_distinct(False, 5) is None
    assert distinct.parse_distinct(True, 5) == 20 == distinct.default_fetch_k(5)
    assert distinct.parse_distinct(True, 1) == 16 and distinct.parse_distinct(True, 64) == 64
    assert distinct.parse_distinct({}, 10) == 40
    assert distinct.parse_distinct({"fetch_k": 10}, 10) == 10 and distinct.parse_distinct({"fetch_k": 64}, 10) == 64
    for bad in ({"fetch_k": 9}, {"fetch_k": 65}, {"fetch_k": 12.0}, {"fetch_k": True}, {"k": 3}, 1, 0.5, "yes", [1]):
        with pytest.raises(ValueError):
            distinct.parse_distinct(bad, 10)


def test_env_default(monkeypatch):
    from rfx import distinct
    monkeypatch.delenv("RFX_DISTINCT", raising=False)
    assert distinct.env_default() is None
    monkeypatch.setenv("RFX_DISTINCT", "0")
    assert distinct.env_default() is None
    monkeypatch.setenv("RFX_DISTINCT", "1")
    assert distinct.env_default() is True


class _Sharded(HostIndex):
    """Looks like a sharded index to the retriever: no search_distinct."""


def test_the_three_refusals(tmp_path):
    from rfx import store as rstore
    from rfx.distinct import DISTINCT_ERROR
    from rfx.retriever import GpuRetriever
    reg = rstore.StoreRegistry(root=str(tmp_path), device=0, index_factory=_Sharded)
    st = reg.create("demo", D, "f32")
    st.add_document(["a", "b"], vecs(2, 1), "a.md")
    ivf = reg.create("lists", D, "f32", spec={"kind": "ivf", "nlist": 4, "nprobe": 2, "train_min": 1 << 30})
    ivf.add_document(["a"], vecs(1, 2), "b.md")
    ivf.index.search_distinct = None  # (its index could run it: the store's kind is what refuses)
    ret = GpuRetriever(registry=reg, dim=D, dtype="f32")
    ret.batching = False
    for kw in ({"diversity": 0.5}, {"hybrid": 0.5}):  # together with diversity, together with hybrid
        with pytest.raises(ValueError, match=DISTINCT_ERROR):
            ret.search([st.name], "question", 2, distinct=True, **kw)
    for name in (st.name, ivf.name):  # a store whose index cannot run it (sharded), an IVF store
        with pytest.raises(ValueError, match=DISTINCT_ERROR):
            ret.search([name], "question", 2, distinct=True)
    with pytest.raises(ValueError, match=DISTINCT_ERROR):
        ret.search_store(st.name, "question", 2, diversity=(0.5, 16), distinct=16)
