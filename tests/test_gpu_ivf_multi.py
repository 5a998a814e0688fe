"""GPU parity of the IVF search of a batch under different filters (rfx_ivf_search_multi /
rfx_ivf_search_rerank_multi) against tests/ivf_multi_ref.py: ivf_mask_ref.search once per question
at that question's probe count under that question's mask, stacked.  Corpora: tests/hostile_ivf.py's edges, skew
(the 12,000-row list beside short ones) and dups.  Tables of 1, 2, 8, 9 (straddling the staged batch of 8) and nq
masks, with and without questions that take no mask, the questions in filter-group order and shuffled;
complementary masks on questions that probe the same lists in the same staged batch; identical masks under two
table indices; probe counts mixed 1 / 3 / all, all equal, and nlist 4,100 (the fallback probe merge).  The bar is
BIT-EXACT (rows equal, scores equal as uint32); the re-rank form as tests/test_gpu_ivf_masked.py holds it.
tests/test_ivf_multi_ref.py shows on the CPU that a kernel with one mask per staged batch, one probe count per
batch, or a mask applied after the top-k fails every case where it can."""
import ctypes

import numpy as np
import pytest
import torch

import hostile
import hostile_ivf as hi
import ivf_mask_ref as mr
import ivf_multi_ref as mu
from oracle import ivf as oivf

pytestmark = pytest.mark.gpu

_corpora, _indexes, _masks = {}, {}, {}


@pytest.fixture(scope="module")
def rivf():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rfx.ivf as rivf
    yield rivf
    for ix in _indexes.values():
        ix.close()
    _indexes.clear()
    _masks.clear()


def corpus(name):
    if name not in _corpora:
        c = getattr(hi, name)("bf16")
        c.rows.setflags(write=False)
        _corpora[name] = c
    return _corpora[name]


def up(x):
    t = torch.from_numpy(np.array(x, dtype=np.float32)).to(torch.bfloat16)
    assert np.array_equal(t.to(torch.float32).numpy(), x)
    return t.cuda()


def assert_same(s, r, ref_s, ref_r, what):
    s, r = s.cpu().numpy(), r.cpu().numpy()
    bad = np.flatnonzero((r != ref_r).any(axis=1) | (s.view(np.uint32) != ref_s.view(np.uint32)).any(axis=1))
    if bad.size:
        i = bad[0]
        j = np.flatnonzero((r[i] != ref_r[i]) | (s[i].view(np.uint32) != ref_s[i].view(np.uint32)))[0]
        pytest.fail(f"{what}: {bad.size} of {len(r)} queries differ; query {i} from place {j}: rows "
                    f"{r[i][j:j + 6].tolist()} scores {s[i][j:j + 6].tolist()}, reference rows "
                    f"{ref_r[i][j:j + 6].tolist()} scores {ref_s[i][j:j + 6].tolist()}")


def decidable(cand, q64, rows64, k, margin):
    """tests/test_gpu_ivf_masked.py's separation condition: among a query's k + 1 best candidates, two f64 scores
    are either more than `margin` (twice the f32 dot's error bound) apart or belong to identical rows."""
    out = np.ones(len(cand), dtype=bool)
    for i in range(len(cand)):
        rr = cand[i][cand[i] >= 0]
        sc = rows64[rr] @ q64[i]
        o = np.lexsort((rr, -sc))[:k + 1]
        for a, b in zip(o[:-1], o[1:]):
            if not (sc[a] - sc[b] > margin or np.array_equal(rows64[rr[a]], rows64[rr[b]])):
                out[i] = False
    return out


def index_of(rivf, c):
    if c.name not in _indexes:
        ix = rivf.IvfIndex(c.rows.shape[1], c.nlist)
        ix.set_centroids(torch.from_numpy(c.qc).cuda())
        ix.add(up(c.rows))
        _indexes[c.name] = ix
    return _indexes[c.name]


def device_masks(c, names, splits, nq):
    """One device tensor per table entry (the spare bits set) — a tensor of its own per entry, equal names too."""
    lab = c.quantized()[2]
    out = []
    for n in names:
        key = (c.name, n, splits if "seedless" in n else 1, nq if n.startswith("rot") else 0)
        if key not in _masks:
            _masks[key] = mr.to_words(mu.selection(n, lab, splits, nq))
        out.append(torch.from_numpy(_masks[key]).cuda())
    return out


def reference(c, q, names, mo, npr, splits, k):
    codes, inv, lab, fc = c.quantized()
    qq, qinv = oivf.quantize(q)
    sels = mu.selections(c, names, mo, splits, len(q))
    return mu.search(qq, qinv, codes, inv, lab, c.qc, fc, npr, k, sels), sels


@pytest.mark.parametrize("name,table,holes,order,splits,k,nq,probes", mu.CASES)
def test_search_multi(rivf, monkeypatch, name, table, holes, order, splits, k, nq, probes):
    c = corpus(name)
    assert c.rows.shape[0] % 32, "the last mask word must have spare bits"
    ix = index_of(rivf, c)
    q = c.queries["law"][:nq]
    names, mo, npr = mu.build(c, table, holes, order, splits, nq, probes)
    masks = device_masks(c, names, splits, nq)
    monkeypatch.setenv("RFX_IVF_SPLITS", str(splits))
    s, r = ix.search(up(q), k, None, row_masks=masks, mask_of=mo, nprobes=npr)
    (ref_s, ref_r), sels = reference(c, q, names, mo, npr, splits, k)
    assert_same(s, r, ref_s, ref_r, f"{name}/{table} holes {holes} {order} splits {splits} k {k} nq {nq} {probes}")
    r = r.cpu().numpy()
    for i in range(nq):
        assert sels[i][r[i][r[i] >= 0]].all()


def test_complementary_masks_share_lists_and_batches(rivf):
    """The case the kernel exists for, stated on the answers: 33 questions probe every list under `alt` and its
    complement in turn, so every list's staged batches of 8 hold both masks (17 and 16 pairs cannot be cut into
    eights along the mask), and a row that one question returns is one its neighbour may not."""
    c = corpus("skew")
    ix = index_of(rivf, c)
    q = c.queries["law"]
    names, mo, npr = ["alt", "~alt"], np.arange(33, dtype=np.int32) % 2, np.full(33, c.nlist, dtype=np.int32)
    s, r = ix.search(up(q), 16, None, row_masks=device_masks(c, names, 1, 33), mask_of=mo, nprobes=npr)
    (ref_s, ref_r), _ = reference(c, q, names, mo, npr, 1, 16)
    assert_same(s, r, ref_s, ref_r, "complementary masks")
    r = r.cpu().numpy()
    assert (r[0::2] % 2 == 1).all() and (r[1::2] % 2 == 0).all() and (r >= 0).all()


def test_equal_to_the_one_mask_and_unmasked_calls(rivf):
    c = corpus("dups")
    ix = index_of(rivf, c)
    q = up(c.queries["law"])
    (alt,) = device_masks(c, ["alt"], 1, 33)
    for k, nprobe in ((5, 3), (64, min(c.nlist, 64))):
        ms, mrows = ix.search(q, k, nprobe, row_mask=alt)
        s, r = ix.search(q, k, nprobe, row_masks=[alt])  # one mask, equal probe counts
        assert_same(s, r, ms.cpu().numpy(), mrows.cpu().numpy(), "one mask vs rfx_ivf_search_masked")
        us, ur = ix.search(q, k, nprobe)
        s, r = ix.search(q, k, nprobe, row_masks=[alt], mask_of=[-1] * 33)  # all -1
        assert_same(s, r, us.cpu().numpy(), ur.cpu().numpy(), "all -1 vs rfx_ivf_search")
        s, r = ix.search(q, k, nprobe, nprobes=[nprobe] * 33)  # no table at all
        assert_same(s, r, us.cpu().numpy(), ur.cpu().numpy(), "no table vs rfx_ivf_search")
    with pytest.raises(ValueError, match="exclusive"):
        ix.search(q, 5, 3, row_mask=alt, row_masks=[alt])


def test_workspace_reuse_after_a_wider_call(rivf):
    """One workspace: a call with every question at every list, then one with most questions at one probe.  The
    second call's absent pairs must read empty, not the first call's candidates."""
    c = corpus("edges")
    ix = index_of(rivf, c)
    nq, k = 33, 16
    q = c.queries["law"][:nq]
    names = ["alt", "~alt"]
    masks = device_masks(c, names, 1, nq)
    mo = mu.mask_of(2, nq, False, "shuffle")
    full = np.full(nq, c.nlist, dtype=np.int32)
    ws = torch.empty(ix.workspace_bytes(nq, k, c.nlist), dtype=torch.uint8, device="cuda")
    for npr in (full, mu.probe_counts("most1", nq, c.nlist)):
        assert npr.max() == c.nlist
        s, r = ix.search(up(q), k, None, workspace=ws, row_masks=masks, mask_of=mo, nprobes=npr)
        (ref_s, ref_r), _ = reference(c, q, names, mo, npr, 1, k)
        assert_same(s, r, ref_s, ref_r, f"workspace reuse, probe counts {sorted(set(npr.tolist()))}")


@pytest.fixture(scope="module")
def wide():
    """nlist 4,100 (> 4,096: probe selection takes the merge kernel): random int8 centroids, 3,001 rows near a
    few hundred of them."""
    d, nlist, n, nq = 256, 4100, 3001, 9
    rng = np.random.default_rng(21)
    dirs = hostile._unit(rng.standard_normal((nlist, d)))
    qc = oivf.quantize(dirs.astype(np.float32))[0]
    near = rng.integers(0, nlist, 300)
    rows = hostile.stored(hostile._unit(dirs[near[rng.integers(0, 300, n)]] + 0.3 * hostile._unit(
        rng.standard_normal((n, d)))), "bf16")
    q = hostile.stored(hostile._unit(dirs[near[:nq]] + 0.3 * hostile._unit(rng.standard_normal((nq, d)))), "bf16")
    return hi.IvfCorpus("wide", "bf16", rows, qc, {"law": q})


def test_nlist_4100_takes_the_fallback_probe_merge(rivf, wide):
    c = wide
    ix = rivf.IvfIndex(256, c.nlist)
    try:
        ix.set_centroids(torch.from_numpy(c.qc).cuda())
        ix.add(up(c.rows))
        q = c.queries["law"]
        nq = len(q)
        names = ["alt", "~alt", "wordedge"]
        lab = c.quantized()[2]
        masks = [torch.from_numpy(mr.to_words(mu.selection(n, lab))).cuda() for n in names]
        mo = np.array([0, 1, 2, -1, 0, 1, 2, -1, 0], dtype=np.int32)
        npr = mu.probe_counts("mix", nq, c.nlist)  # 1 / 3 / 64
        assert set(npr.tolist()) == {1, 3, 64}
        s, r = ix.search(up(q), 16, None, row_masks=masks, mask_of=mo, nprobes=npr)
        (ref_s, ref_r), _ = reference(c, q, names, mo, npr, 1, 16)
        assert_same(s, r, ref_s, ref_r, "nlist 4100")
        assert (ref_r >= 0).any()
    finally:
        ix.close()


# (corpus, table, mask_of pattern, k, rerank depth, probes, queries): chosen on the CPU, from the reference alone,
# so that every query decides its rows beyond the f32 dot's error bound with twice the margin to spare
# (tests/test_gpu_ivf_masked.py, decidable); mask_of and the probe counts are those of the queries listed
RERANK = [
    ("edges", ["alt", "few"], 5, 20, "mix", [0, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 18, 19, 20, 21, 23, 24, 26, 28, 29, 32]),
    ("dups", ["wordedge", "~alt"], 5, 16, mu.FULL, [0, 2, 3, 6, 7, 9, 11, 12, 13, 14, 15, 16, 17, 18, 20, 21, 22, 27, 28, 29,
                                                   30]),
    ("skew", ["ranges", "wordedge"], 5, 16, 3, [0, 2, 3, 8, 11, 12, 13, 18, 22, 23, 24, 26, 27, 28, 30, 31, 32]),
]


@pytest.mark.parametrize("name,names,k,rk,probes,queries", RERANK, ids=[f"{c[0]}-k{c[2]}-rk{c[3]}" for c in RERANK])
def test_search_rerank_multi(rivf, name, names, k, rk, probes, queries):
    c = corpus(name)
    ix = index_of(rivf, c)
    q = c.queries["law"] if queries is None else c.queries["law"][queries]
    nq = len(q)
    mo = mu.mask_of(len(names), nq, True, "shuffle")
    npr = mu.probe_counts(probes, nq, c.nlist)
    (_, cand), sels = reference(c, q, names, mo, npr, 1, rk)
    rows64, q64 = c.rows.astype(np.float64), q.astype(np.float64)
    _, ref_r = oivf.rerank(cand, q64, rows64, k)
    S = hostile.scale_bound(c.rows, q)
    sure = decidable(cand, q64, rows64, k, 2 * (c.rows.shape[1] // 64 + 7) * 2.0 ** -24 * S)
    assert sure.all(), f"queries {np.flatnonzero(~sure).tolist()} do not decide their rows: pick other queries"
    s, r = ix.search_rerank(up(q), k, None, up(c.rows), rerank_k=rk, row_masks=device_masks(c, names, 1, nq),
                            mask_of=mo, nprobes=npr)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    assert np.array_equal(r, ref_r), f"{(r != ref_r).any(axis=1).sum()} of {nq} queries differ in rows"
    for i in range(nq):
        ok = r[i] >= 0
        assert sels[i][r[i][ok]].all() and np.isneginf(s[i][~ok]).all()
        assert np.all(np.abs(s[i][ok] - rows64[r[i][ok]] @ q64[i]) <= 1e-5)


def _raw(ix, q, k, table_ptr, n_masks, words, mo, npr, nmax, host=True):
    """host: the check runs on the host copies the caller passes; False: on a read-back of the device arrays."""
    from rfx._lib import DTYPE_CODES, lib, ptr, stream_ptr
    nq = q.shape[0]
    out_s = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    out_r = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    ws = torch.empty(max(ix.workspace_bytes(nq, k, min(max(nmax, 1), ix.nlist, 64)), 1), dtype=torch.uint8, device="cuda")
    mo_h, np_h = torch.tensor(mo, dtype=torch.int32), torch.tensor(npr, dtype=torch.int32)
    mo_d, np_d = mo_h.cuda(), np_h.cuda()
    null = ctypes.c_void_p(0)
    rc = lib.rfx_ivf_search_multi(ix.handle, ptr(q), nq, DTYPE_CODES["bf16"], k, table_ptr, n_masks, words, ptr(mo_d),
                                  ptr(np_d), nmax, ptr(mo_h) if host else null, ptr(np_h) if host else null,
                                  ptr(out_s), ptr(out_r), ptr(ws), ws.numel(), stream_ptr(None))
    torch.cuda.synchronize()
    return rc, out_s, out_r


def test_einval(rivf):
    from rfx import _lib
    c = corpus("edges")
    ix = index_of(rivf, c)
    q = up(c.queries["law"][:4])
    masks = device_masks(c, ["alt", "~alt"], 1, 4)
    table = torch.tensor([m.data_ptr() for m in masks], dtype=torch.int64).cuda()
    need = (c.rows.shape[0] + 31) // 32
    ok_mo, ok_np = [0, 1, -1, 0], [1, 3, 2, 3]
    bs, br = ix.search(q, 5, None, row_masks=masks, mask_of=ok_mo, nprobes=ok_np)
    for host in (True, False):
        rc, s, r = _raw(ix, q, 5, _lib.ptr(table), 2, need, ok_mo, ok_np, 3, host)
        assert rc == _lib.RFX_OK
        assert_same(s, r, bs.cpu().numpy(), br.cpu().numpy(), f"raw call (host copies: {host}) vs binding")
    bad = [
        (_lib.ptr(table), 2, need - 1, ok_mo, ok_np, 3, b"row mask has"),       # short masks
        (_lib.ptr(table), 2, need, [0, 2, -1, 0], ok_np, 3, b"mask_of[1]"),     # index == n_masks
        (_lib.ptr(table), 2, need, [0, 1, -2, 0], ok_np, 3, b"mask_of[2]"),     # below -1
        (_lib.ptr(table), 2, need, ok_mo, [1, 3, 0, 3], 3, b"nprobe_of[2]"),    # probe count 0
        (_lib.ptr(table), 2, need, ok_mo, [1, 4, 2, 3], 3, b"nprobe_of[1]"),    # above nprobe_max
        (ctypes.c_void_p(0), 0, 0, ok_mo, ok_np, 3, b"n_masks is 0"),            # no table, yet an index >= 0
        (_lib.ptr(table), 2, need, ok_mo, ok_np, 65, b"nprobe=65"),             # nprobe_max past the ABI's 64
    ]
    for table_ptr, n_masks, words, mo, npr, nmax, msg in bad:
        for host in (True, False):  # checked on the caller's host copies, and on the read-back without them
            rc, _, _ = _raw(ix, q, 5, table_ptr, n_masks, words, mo, npr, nmax, host)
            assert rc == _lib.RFX_EINVAL and msg in _lib.lib.rfx_last_error(), (msg, host, _lib.lib.rfx_last_error())
    rc, s, r = _raw(ix, q, 5, ctypes.c_void_p(0), 0, 0, [-1] * 4, ok_np, 3)  # no table and no index: fine
    assert rc == _lib.RFX_OK
    with pytest.raises(ValueError, match="row mask has"):
        ix.search_rerank(q, 5, None, up(c.rows), row_masks=[masks[0][:need - 1].contiguous()], mask_of=[0] * 4,
                         nprobes=ok_np)


def test_sharded_multi_equals_one_device(tmp_path, monkeypatch):
    """An IVF store read through 4 logical shards answers a batch under different filters in one list search
    (search_lists_filtered_multi) bit-identically to the same store on one device."""
    from rfx import ivf as rivf_
    from rfx import store as rstore
    from rfx.sharded import ShardedIndex, ShardedIvf

    dim, spec = 768, {"kind": "ivf", "nlist": 32, "nprobe": 8, "train_min": 4000}
    root = str(tmp_path)
    st = rstore.StoreRegistry(root=root, device=0).create("ivf-sh", dim, "bf16", spec=spec)
    docs = [rivf_.synth_clustered(7, 48, 200 + i, 1500 * i, 1500, dim, "bf16") for i in range(4)]
    fids = [st.add_document([f"d{i}-{j}" for j in range(1500)], v, f"d{i}.md", {"tenant": f"t{i % 2}"})[0]
            for i, v in enumerate(docs)]
    st.delete_file(fids[2])  # tenant t0 keeps rows 0 .. 1499, t1 rows 1500 .. 2999 and 4500 .. 5999
    st.add_document([f"e-{j}" for j in range(37)], rivf_.synth_clustered(7, 48, 300, 0, 37, dim, "bf16"), "e.md",
                    {"tenant": "t1"})  # 6,037 rows: not a multiple of 32
    plain = rstore.StoreRegistry(root=root, device=0).get(st.name)
    shard = rstore.StoreRegistry(root=root, device=0, devices="0x4").get(st.name)
    assert isinstance(shard.index, ShardedIndex) and isinstance(shard.ivf, ShardedIvf)
    assert plain.ivf_ready() and shard.ivf_ready()
    monkeypatch.setenv("RFX_IVF_FILTERED", "1")
    q = rivf_.synth_clustered(7, 48, 999, 0, 33, dim, "bf16")
    filts = [{"tenant": f"t{i % 2}"} for i in range(33)]
    assert plain.filtered_nprobe(filts[0]) != plain.filtered_nprobe(filts[1])  # probe counts differ across groups
    for k in (1, 10, 20):
        a_s, a_r, a_d = plain.search_lists_filtered_multi(q, k, filts)
        b_s, b_r, b_d = shard.search_lists_filtered_multi(q, k, filts)
        assert a_d == b_d == []
        assert np.array_equal(a_r.numpy(), b_r.numpy())
        assert np.array_equal(a_s.numpy().view(np.uint32), b_s.numpy().view(np.uint32))
        r = a_r.numpy()
        assert (r[0::2] < 1500).all() and (r[1::2] >= 1500).all() and (r >= 0).all()
        for i in (0, 1):  # and each is the one-filter call's answer
            o_s, o_r = plain.search_lists_filtered(q[i::2].contiguous(), k, filts[i])
            assert np.array_equal(o_r.numpy(), r[i::2])
            assert np.array_equal(o_s.numpy().view(np.uint32), a_s.numpy()[i::2].view(np.uint32))
