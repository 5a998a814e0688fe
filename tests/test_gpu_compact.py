"""GPU: store compaction on the HIP path.

rfx_index_compact gathers the kept rows into a fresh allocation: the compacted index reads back the kept rows
bit for bit (every dtype; ranges of one row, ranges at the 32- and 128-row boundaries, a run of small ranges
that work chunks span, the last row), its counts and capacity are those of a fresh index of the kept rows, a
kept tombstone stays NaN, keep-all moves nothing and keep-none leaves a usable empty index.  Searches over
the compacted index match the f64 oracle on the kept rows and a fresh index bit for bit, on the VALU plan, the
two-pass scan's kernels 11 and 10 and an exact MFMA plan; the rebuilt int8 copy equals a fresh one, maxima
included.  At the store level: the compacted store answers like one that only ever held the live documents,
another LocalStore object follows on its own index, union views are rebuilt, device memory shrinks, and an
IVF store keeps its centroids."""
import numpy as np
import pytest
import torch

from oracle import search as osearch
from oracle import synth as osynth

pytestmark = pytest.mark.gpu

TOL, TIE = 1e-5, 2e-6  # the bars of test_gpu_parity
RANGES = ([(0, 1), (3, 1), (20, 12), (32, 40), (100, 60)] + [(300 + 4 * i, 3) for i in range(40)] +
          [(1000, 2500), (4990, 10)])
N = 5000


def keep_index(ranges):
    return np.concatenate([np.arange(f, f + n) for f, n in ranges]) if ranges else np.zeros(0, dtype=np.int64)


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.fixture(scope="module")
def rindex():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rfx.index as rindex
    return rindex


# ---- bytes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("dim", [64, 768])
def test_compacted_rows_are_the_kept_rows_bit_for_bit(rindex, dtype, dim):
    ix = rindex.DeviceIndex(dim, dtype)
    ix.add_synthetic(5, N)
    before = ix.read(0, N).clone()
    keep = keep_index(RANGES)
    assert set(ix.compact_times().values()) == {0.0}
    assert ix.compact(RANGES) == keep.size
    assert ix.rows == keep.size and ix.live_rows == keep.size
    times = ix.compact_times()
    assert times["gather"] > 0 and all(v >= 0 for v in times.values())
    got = ix.read(0, ix.rows)
    want = before[torch.from_numpy(keep).to(before.device)]
    assert torch.equal(bits(got), bits(want))
    fresh = rindex.DeviceIndex(dim, dtype)
    fresh.add(want)
    assert ix.capacity == fresh.capacity and ix.capacity >= ix.rows and ix.capacity % 128 == 0
    # the compacted index takes appends like any other
    assert ix.add(before[:7]) == keep.size
    assert torch.equal(bits(ix.read(keep.size, 7)), bits(before[:7]))
    assert torch.equal(bits(ix.read(0, keep.size)), bits(want))
    ix.close()
    fresh.close()


def test_malformed_ranges_are_refused_before_anything_moves(rindex):
    ix = rindex.DeviceIndex(64, "f32")
    ix.add_synthetic(5, 300)
    before = ix.read(0, 300).clone()
    cap = ix.capacity
    for bad in ([(50, 5), (10, 5)], [(10, 5), (14, 5)], [(296, 5)], [(-1, 5)], [(10, 0)], [(300, 1)]):
        with pytest.raises(ValueError):
            ix.compact(bad)
    assert ix.rows == 300 and ix.capacity == cap and torch.equal(bits(ix.read(0, 300)), bits(before))
    ix.close()


def test_kept_tombstone_stays_nan_and_never_ranks(rindex):
    ix = rindex.DeviceIndex(768, "bf16")
    ix.add_synthetic(5, N)
    q = ix.read(33, 1).clone()  # the question IS row 33: it would rank first
    ix.tombstone([33, 1001, 80])  # 33 and 1001 are kept rows; 80 is dropped
    keep = keep_index(RANGES)
    ix.compact(RANGES)
    assert ix.rows == keep.size and ix.live_rows == keep.size - 2
    p33, p1001 = int(np.flatnonzero(keep == 33)[0]), int(np.flatnonzero(keep == 1001)[0])
    for p in (p33, p1001):
        assert torch.isnan(ix.read(p, 1).float()).all()
    assert not torch.isnan(ix.read(p33 + 1, 1).float()).any()
    s, r = ix.search(q, 10)
    r = r.cpu().numpy()
    assert p33 not in r and p1001 not in r and (r >= 0).all()
    ix.tombstone([p33])  # already tombstoned: the host bitmap followed the rows
    assert ix.live_rows == keep.size - 2
    ix.close()


def test_keep_all_is_a_no_op_and_keep_none_leaves_a_usable_index(rindex):
    ix = rindex.DeviceIndex(768, "bf16")
    ix.add_synthetic(5, 700)
    before = ix.read(0, 700).clone()
    ptr, cap = ix.data_ptr(), ix.capacity
    assert ix.compact([(0, 700)]) == 700 and ix.compact([(0, 300), (300, 400)]) == 700
    assert ix.data_ptr() == ptr and ix.capacity == cap and ix.rows == 700
    assert ix.compact([]) == 0
    assert ix.rows == 0 and ix.live_rows == 0 and ix.capacity == 0
    q = before[:2].contiguous()
    assert ix.add(before[:300].contiguous()) == 0 and ix.rows == 300 and ix.live_rows == 300
    s, r = ix.search(q, 5)
    assert r.cpu().numpy()[:, 0].tolist() == [0, 1]
    ix.close()


# ---- search parity after compaction -----------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[768, 1024])
def compacted(request, rindex):
    """About 20,000 bf16 rows of which 8,192 are kept (128 ranges of 64 rows): the compacted index, a fresh
    index over the same rows, and the kept rows in f64 for the oracle."""
    dim, n = request.param, 20000
    ranges = [(150 * i + 7, 64) for i in range(128)]
    keep = keep_index(ranges)
    ix = rindex.DeviceIndex(dim, "bf16")
    ix.add_synthetic(11, n)
    kept_rows = ix.read(0, n)[torch.from_numpy(keep).to("cuda")].contiguous()
    assert ix.compact(ranges) == 8192
    fresh = rindex.DeviceIndex(dim, "bf16")
    fresh.add(kept_rows)
    rows64 = osynth.to_f64(osynth.synth_rows(11, 0, n, dim, "bf16")[keep], "bf16")
    yield dim, ix, fresh, rows64
    ix.close()
    fresh.close()


@pytest.mark.parametrize("nq,screen,kernel", [(1, 0, 0), (4, 1, 11), (16, 1, 10), (16, 0, None)])
def test_search_parity_after_compaction(rindex, compacted, nq, screen, kernel):
    dim, ix, fresh, rows64 = compacted
    for x in (ix, fresh):
        x.enable_screen(screen)
    if kernel is None:
        assert ix.plan(nq, 10)[0] not in (0, 10, 11), "an exact MFMA plan"
    else:
        assert ix.search_plan(nq, 10) == kernel
    q = rindex.synth_rows(12, 0, nq, dim, "bf16")
    q64 = osynth.to_f64(osynth.synth_rows(12, 0, nq, dim, "bf16"), "bf16")
    s, r = ix.search(q, 10)
    fs, fr = fresh.search(q, 10)
    torch.cuda.synchronize()
    assert torch.equal(r, fr) and torch.equal(s.view(torch.int32), fs.view(torch.int32))
    ref_s, ref_r = osearch.topk(q64, rows64, 10)
    probs = osearch.check_topk(s.cpu().numpy(), r.cpu().numpy(), ref_s, ref_r, lambda qi, rows: rows64[rows] @ q64[qi],
                               tol=TOL, tie_band=TIE)
    assert not probs, probs[:5]


# ---- the int8 copy ---------------------------------------------------------------------------------------------
def test_int8_copy_is_rebuilt_over_the_kept_rows(rindex):
    dim, n = 768, 6000
    ranges = [(0, 1000), (2000, 37), (2100, 2900)]
    keep = keep_index(ranges)
    ix = rindex.DeviceIndex(dim, "bf16")
    ix.add_synthetic(21, n)
    ix.write(1500, (ix.read(1500, 1).float() * 3).to(torch.bfloat16))  # a long row among those to be dropped
    ix.enable_screen(1)
    assert ix.screen_read(0, 1)[3][0] > 2.5  # the store-wide max row norm is that row's
    kept_rows = ix.read(0, n)[torch.from_numpy(keep).to("cuda")].contiguous()
    ix.compact(ranges)
    assert ix.screen_state()[0] == 1 and not ix.screen_state()[2]
    fresh = rindex.DeviceIndex(dim, "bf16")
    fresh.add(kept_rows)
    fresh.enable_screen(1)
    assert ix.capacity == fresh.capacity
    got, want = ix.screen_read(0, ix.capacity // 32), fresh.screen_read(0, fresh.capacity // 32)
    for g, w, what in zip(got, want, ("codes", "scales", "live words", "stats")):
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g,
                              w.view(np.uint32) if w.dtype == np.float32 else w), what
    assert got[3][0] < 1.5  # the maxima are the kept rows'
    ix.close()
    fresh.close()


# ---- store level ---------------------------------------------------------------------------------------------------
DOC = 4000


def _fill(st, rindex, which):
    fids = {}
    for i in which:
        fids[i] = st.add_document([f"d{i}-{j}" for j in range(DOC)], rindex.synth_rows(30 + i, 0, DOC, 768, "bf16"),
                                  f"d{i}.md", {"doc": str(i)})[0]
    return fids


def test_store_compaction_end_to_end(rindex, tmp_path, monkeypatch):
    from rfx import retriever as rret
    from rfx import store as rstore
    from rfx.index import DeviceIndex

    reg = rstore.StoreRegistry(root=str(tmp_path / "a"), device=0)
    st = reg.create("demo", 768, "bf16")
    fids = _fill(st, rindex, range(5))
    other_reg = rstore.StoreRegistry(root=str(tmp_path / "a"), device=0)
    sb = other_reg.get(st.name)  # another process's object, caught up
    st.delete_file(fids[1])
    st.delete_file(fids[3])
    assert sb.refresh()
    handle, cap_before = sb.index.handle, st.index.capacity

    # a union view over this store and another, built before the compaction
    two = reg.create("second", 768, "bf16")
    _fill(two, rindex, [7])
    ret = rret.GpuRetriever(registry=reg, dtype="bf16")
    ret.batching = False
    names = [st.name, two.name]

    def hits(union):
        ret.union = union
        out = [(h.store, h.file_id, h.text, round(h.score, 6)) for h in ret.search(names, "alpha gamma delta", 10)]
        assert ret.last_path == ("union" if union else "per-store")
        return out
    before_hits = hits(True)
    assert before_hits == hits(False)
    key = (tuple(names), id(reg))
    view = rret._UNIONS[key]

    syncs = []
    real_sync = DeviceIndex.rows_sync
    monkeypatch.setattr(DeviceIndex, "rows_sync", lambda self, *a, **kw: (syncs.append(a), real_sync(self, *a, **kw))[1])
    out = ret.compact_store(st.name)
    assert out["rows_before"] == 5 * DOC and out["rows"] == 3 * DOC
    assert st.index.rows == 3 * DOC and st.index.live_rows == 3 * DOC and st.dead_rows() == 0
    assert st.index.capacity < cap_before, "the smaller allocation"
    assert key not in rret._UNIONS, "the view that pinned the old allocation is evicted"

    # the same answers as a store that only ever held the three live documents
    ref = rstore.StoreRegistry(root=str(tmp_path / "b"), device=0).create("ref", 768, "bf16")
    _fill(ref, rindex, [0, 2, 4])
    for nq in (1, 16):
        q = rindex.synth_rows(40, 0, nq, 768, "bf16")
        s, r = st.search(q, 10)
        rs, rr = ref.search(q, 10)
        assert torch.equal(r, rr) and torch.equal(s.view(torch.int32), rs.view(torch.int32))
    assert [t for _, t in st.rows] == [t for _, t in ref.rows]
    assert st.row_info(DOC)[1] == "d2-0" and st.row_info(DOC)[0] == fids[2]

    # the other object follows on its own index: same handle, no row bytes from disk
    assert other_reg.get(st.name) is sb and sb.index.handle == handle and syncs == []
    assert sb.generation == st.generation and sb.index.rows == 3 * DOC
    q = rindex.synth_rows(41, 0, 4, 768, "bf16")
    s, r = st.search(q, 10)
    bs, br = sb.search(q, 10)
    assert torch.equal(r, br) and torch.equal(s.view(torch.int32), bs.view(torch.int32))

    # the union is rebuilt over the new rows and answers like the per-store path
    after = hits(True)
    assert rret._UNIONS[key] is not view
    assert after == hits(False)
    assert after == before_hits, "the deleted documents were tombstoned before: the answers do not change"
    for s_ in (sb, ref, two, st):
        s_.close()


def test_ivf_store_keeps_its_centroids(rindex, tmp_path):
    from rfx import ivf as rivf
    from rfx import store as rstore

    reg = rstore.StoreRegistry(root=str(tmp_path), device=0)
    st = reg.create("ivf-demo", 768, "bf16", spec={"kind": "ivf", "nlist": 8, "nprobe": 8, "train_min": 2000})
    fids = [st.add_document([f"d{i}-{j}" for j in range(1000)],
                            rivf.synth_clustered(7, 16, 100 + i, 1000 * i, 1000, 768, "bf16"), f"d{i}.md")[0]
            for i in range(3)]
    assert st.ivf_ready()
    cid = st.ivf_id
    st.delete_file(fids[1])
    assert st.compact()["rows"] == 2000
    assert st.ivf_ready() and st.ivf_id == cid and st.ivf_meta["id"] == cid and st.ivf.rows == 2000
    q = rivf.synth_clustered(7, 16, 999, 0, 8, 768, "bf16")
    s, r = st.search(q, 10)  # through the lists (every list probed), re-ranked exactly
    es, er = st.index.search(q, 10)
    from rfx.quality import recall_at_k
    assert recall_at_k(r.numpy().tolist(), er.cpu().numpy().tolist(), 10) >= 0.9
    assert 0 <= int(r.min()) and int(r.max()) < 2000
    fresh = rstore.StoreRegistry(root=str(tmp_path), device=0).get(st.name)
    assert fresh.ivf_ready() and fresh.ivf_id == cid
    assert np.array_equal(fresh.search(q, 10)[1].numpy(), r.numpy())
    fresh.close()
    st.close()
