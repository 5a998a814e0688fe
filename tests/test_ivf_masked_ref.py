"""CPU: the reference of the metadata-filtered IVF search and the store's rule around it.

1. tests/ivf_mask_ref.py's wrapper (oracle.ivf.search with the unselected rows' labels set to -1) equals the
   definition written out: score every row of the probed lists, drop the unselected, rank.
2. Two mutants — the mask ignored; the mask applied to the finished unmasked top-k — differ from the wrapper on
   every (corpus, mask, grid point) the GPU file runs, other than the all-ones and all-zero masks: the cases
   discriminate.
3. rfx.store.ivf_filter_nprobe: exact values, the cap, selected = 0, the three modes.
4. LocalStore.search_filtered with host stand-ins (tests/fakes.py): "ivf" at the widened nprobe with the mask
   passed through under auto; "exact" when the cap bites, when the lists are behind and under mode 0;
   LocalStore.search(row_mask=...) untouched in every mode."""
import numpy as np
import pytest

import hostile_ivf as hi
import ivf_mask_ref as mr
from fakes import HostIndex, HostIvf
from oracle import ivf as oivf
from rfx import store as rstore

_corpora = {}


def corpus(name):
    if name not in _corpora:
        c = getattr(hi, name)("bf16")
        c.rows.setflags(write=False)
        _corpora[name] = c
    return _corpora[name]


def args_of(c, nq, nprobe):
    codes, inv, lab, fc = c.quantized()
    qq, qinv = oivf.quantize(c.queries["law"][:nq])
    return qq, qinv, codes, inv, lab, c.qc, fc, nprobe or min(c.nlist, 64)


# ---- 1. the wrapper is the definition ----------------------------------------------------------------------
@pytest.mark.parametrize("name,mask,k,nq,nprobe", [("edges", "alt", 17, 5, 3), ("edges", "wordedge", 64, 4, mr.FULL),
                                                   ("dups", "ranges", 16, 7, 3), ("dups", "few", 5, 4, mr.FULL),
                                                   ("edges", "zeros", 4, 2, 1), ("dups", "ones", 64, 7, 3)])
def test_wrapper_is_the_definition(name, mask, k, nq, nprobe):
    c = corpus(name)
    a = args_of(c, nq, nprobe)
    sel = mr.selection(mask, a[4])
    s, r = mr.search(*a, k, sel)
    bs, br = mr.brute_force(*a, k, sel)
    assert hi.same_bits(s, r, bs, br)
    assert sel[r[r >= 0]].all()
    if mask == "zeros":
        assert (r == -1).all() and np.isneginf(s).all()


def test_masks_are_what_they_claim():
    for name in mr.PLAN:
        c = corpus(name)
        lab = c.quantized()[2]
        n = len(lab)
        assert n % 32, f"{name}: {n} rows, a multiple of 32 — the last mask word has no spare bits"
        sizes = np.bincount(lab, minlength=c.nlist)
        assert mr.selection("first", lab).sum() == (sizes > 0).sum() == mr.selection("last", lab).sum()
        assert mr.selection("few", lab).sum() == 3
        w = mr.selection("wordedge", lab)
        assert w[0] and w[31] and w[32] and not w[1:31].any()
        rng = mr.selection("ranges", lab)
        assert 0.25 < rng.mean() < 0.75 and np.flatnonzero(np.diff(rng.astype(int))).size >= 6
        for m in mr.PLAN[name]:
            sel = mr.selection(m, lab, 2)
            words = mr.to_words(sel)
            assert len(words) == (n + 31) // 32 and np.array_equal(mr.from_words(words, n), sel)
            assert (words[-1].view(np.uint32) >> np.uint32(n % 32)) == (1 << (32 - n % 32)) - 1  # spare bits set
    lab = corpus("skew").quantized()[2]
    pos = mr.list_positions(lab)
    for splits in (1, 2, 4):
        sel = mr.selection("seedless", lab, splits)
        long_list = np.argmax(np.bincount(lab))
        gone = np.flatnonzero(~sel)
        assert (lab[gone] == long_list).all() and sorted(pos[gone]) == list(range(512 * splits))
        assert np.bincount(lab)[long_list] > 512 * splits + 64 * 4 * splits  # every wave still has rows to offer


# ---- 2. the cases discriminate -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mr.PLAN))
def test_mutants_differ_on_every_case(name):
    c = corpus(name)
    memo = {}
    for cname, mask, splits, k, nq, nprobe in mr.CASES:
        if cname != name or mask in ("ones", "zeros"):
            continue
        a = args_of(c, nq, nprobe)
        sel = mr.selection(mask, a[4], splits)
        ref = mr.search(*a, k, sel)
        key = (k, nq, nprobe)
        if key not in memo:
            memo[key] = mr.mutant_ignored(*a, k, sel)
        for what, got in (("mask ignored", memo[key]), ("mask after the top-k", mr.mutant_after_topk(*a, k, sel))):
            assert not hi.same_bits(got[0], got[1], *ref), \
                f"{name}/{mask} splits {splits} k {k} nq {nq} nprobe {nprobe}: the mutant '{what}' passes"
        if mask == "few" and k > 3:
            assert (ref[1] == -1).any()  # fewer than k eligible rows: padding in the answer


def test_cases_cover_every_value():
    for name in mr.PLAN:
        mine = [c[2:] for c in mr.CASES if c[0] == name]
        assert {m[0] for m in mine} == {1, 2, 4} and {m[1] for m in mine} == {1, 4, 5, 16, 17, 64}
        assert {m[2] for m in mine} == {1, 9, 33} and {m[3] for m in mine} == {1, 3, mr.FULL}
    assert {corpus(n).rows.shape[1] for n in mr.PLAN} == {256, 768}
    assert {c[2] for c in mr.CASES if c[1] == "seedless"} == {1, 2, 4}


# ---- 3. the rule ---------------------------------------------------------------------------------------------
def test_ivf_filter_nprobe():
    f = rstore.ivf_filter_nprobe
    assert f(8, 1024, 6000, 6000, "auto") == 8           # f = 1
    assert f(8, 1024, 3000, 6000, "auto") == 16          # 1/2
    assert f(8, 1024, 2000, 6000, "auto") == 24          # 1/3
    assert f(8, 1024, 750, 6000, "auto") == 64           # 1/8: exactly the cap
    assert f(8, 1024, 2001, 6000, "auto") == 24 and f(8, 1024, 1999, 6000, "auto") == 25  # the ceiling, in integers
    assert f(8, 1024, 749, 6000, "auto") is None and f(8, 1024, 749, 6000, "1") == 64  # past the cap
    assert f(32, 4096, 12_500_000 // 4, 12_500_000, "auto") is None  # config 5's nprobe at f = 1/4: 128 > 64
    assert f(8, 32, 1500, 6000, "auto") == 32 and f(8, 32, 1499, 6000, "auto") is None  # cap = nlist below 64
    assert f(8, 32, 100, 6000, "1") == 32
    for mode in ("0", "auto", "1"):
        assert f(8, 1024, 0, 6000, mode) is None         # nothing selected
    assert f(8, 1024, 6000, 6000, "0") is None and f(8, 1024, 3000, 6000, "0") is None
    assert f(8, 1024, 3000, 6000, "1") == 16


def test_mode_is_read_per_call(monkeypatch):
    monkeypatch.delenv("RFX_IVF_FILTERED", raising=False)
    assert rstore.ivf_filtered_mode() == "0"
    for raw, want in (("auto", "auto"), (" AUTO ", "auto"), ("1", "1"), ("0", "0"), ("yes", "0")):
        monkeypatch.setenv("RFX_IVF_FILTERED", raw)
        assert rstore.ivf_filtered_mode() == want


# ---- 4. the store plan, host stand-ins ---------------------------------------------------------------------
SPEC = {"kind": "ivf", "nlist": 16, "nprobe": 2, "train_min": 16}


class MaskedHostIvf(HostIvf):
    """HostIvf whose search_index takes the row mask (unpacked, applied before its ranking) and logs the call."""
    calls = []

    def search_index(self, queries, k, nprobe, index, rerank_k=None, row_mask=None):
        MaskedHostIvf.calls.append({"k": k, "nprobe": nprobe, "rerank_k": rerank_k, "row_mask": row_mask})
        if row_mask is None:
            return super().search_index(queries, k, nprobe, index, rerank_k)
        sel = mr.from_words(row_mask, self.rows)

        class Masked:  # the index's rows with the unselected ones NaN: HostIvf drops NaN scores before ranking
            @staticmethod
            def read(r0, n):
                x = index.read(r0, n).copy()
                x[~sel[r0:r0 + n]] = np.nan
                return x
        return super().search_index(queries, k, nprobe, Masked, rerank_k)


def vecs(n, seed, dim=32):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


@pytest.fixture
def tenants(tmp_path):
    """64 rows: tenant t0 32 rows, t1 16, t2 8 + a deleted 8-row file of t2: live 56."""
    MaskedHostIvf.calls = []
    reg = rstore.StoreRegistry(root=str(tmp_path), device=0, index_factory=HostIndex, ivf_factory=MaskedHostIvf)
    st = reg.create("demo", 32, "f32", spec=SPEC)
    st.add_document(["a"] * 32, vecs(32, 1), "a.md", metadata={"tenant": "t0"})
    st.add_document(["b"] * 16, vecs(16, 2), "b.md", metadata={"tenant": "t1"})
    st.add_document(["c"] * 8, vecs(8, 3), "c.md", metadata={"tenant": "t2"})
    dead = st.add_document(["d"] * 8, vecs(8, 4), "d.md", metadata={"tenant": "t2"})[0]
    st.delete_file(dead)
    assert st.ivf_ready() and st.dead_rows() == 8
    return st


def exact_filtered(st, q, k, lo, hi):
    x = st.index.read(0, st.index.rows)
    out = []
    for qi in q:
        sc = x @ qi
        ok = np.array([r for r in range(lo, hi) if not np.isnan(sc[r])])
        out.append(list(ok[np.lexsort((ok, -sc[ok]))][:k]))
    return out


def test_search_filtered_takes_the_lists_under_auto(tenants, monkeypatch):
    st = tenants
    monkeypatch.setenv("RFX_IVF_FILTERED", "auto")
    q = vecs(3, 9)
    # t0: 32 of 56 live rows -> ceil(2 * 56 / 32) = 4 probes; t1: 16 of 56 -> 7; t2: 8 of 56 -> 14
    for tenant, lo, hi, nprobe in (("t0", 0, 32, 4), ("t1", 32, 48, 7), ("t2", 48, 56, 14)):
        MaskedHostIvf.calls = []
        filt = {"tenant": tenant}
        assert st.filtered_nprobe(filt) == nprobe
        assert st.search_lists_filtered(q, 5, filt) is not None
        MaskedHostIvf.calls = []
        s, r, path = st.search_filtered(q, 5, filt)
        assert path == "ivf" and len(MaskedHostIvf.calls) == 1  # the rule, the mask and the search: once
        call = MaskedHostIvf.calls[0]
        assert call["nprobe"] == nprobe and call["k"] == 5 and call["rerank_k"] == 16
        assert np.array_equal(call["row_mask"], st.row_mask(filt))
        r = r.numpy()
        assert ((r >= lo) & (r < hi) | (r == -1)).all() and (r >= 0).any()
    # every list probed (nprobe = nlist): the filtered IVF answer is the exact filtered top-k
    monkeypatch.setitem(st.spec, "nprobe", 10)  # t0: ceil(10 * 56 / 32) = 18 > cap 16 -> exact under auto, 16 under 1
    assert st.filtered_nprobe({"tenant": "t0"}) is None and st.search_lists_filtered(q, 5, {"tenant": "t0"}) is None
    monkeypatch.setenv("RFX_IVF_FILTERED", "1")
    assert st.filtered_nprobe({"tenant": "t0"}) == 16
    s, r, path = st.search_filtered(q, 5, {"tenant": "t0"})
    assert path == "ivf" and [list(x) for x in r.numpy()] == exact_filtered(st, q, 5, 0, 32)


def test_search_filtered_exact_paths(tenants, monkeypatch):
    st = tenants
    q = vecs(2, 9)
    import torch
    scans = []
    scan_s, scan_r = torch.tensor([[0.5]]), torch.tensor([[7]])
    monkeypatch.setattr(HostIndex, "search", lambda self, q, k, row_mask=None: scans.append(row_mask) or (scan_s, scan_r),
                        raising=False)
    t2 = {"tenant": "t2"}

    def expect_exact(filt):
        MaskedHostIvf.calls, n = [], len(scans)
        s, r, path = st.search_filtered(q, 5, filt)
        assert path == "exact" and torch.equal(s, scan_s) and torch.equal(r, scan_r)
        assert not MaskedHostIvf.calls and len(scans) == n + 1 and np.array_equal(scans[-1], st.row_mask(filt))

    monkeypatch.setenv("RFX_IVF_FILTERED", "0")  # mode 0
    expect_exact(t2)
    monkeypatch.delenv("RFX_IVF_FILTERED")  # the default is mode 0
    expect_exact(t2)
    monkeypatch.setenv("RFX_IVF_FILTERED", "auto")
    monkeypatch.setitem(st.spec, "nprobe", 3)  # t2: ceil(3 * 56 / 8) = 21 > cap 16: the cap bites
    expect_exact(t2)
    monkeypatch.setitem(st.spec, "nprobe", 2)
    assert st.filtered_nprobe(t2) == 14
    monkeypatch.setattr(type(st), "ivf_ready", lambda self: False)  # the lists are behind
    expect_exact(t2)
    monkeypatch.undo()
    monkeypatch.setenv("RFX_IVF_FILTERED", "auto")
    MaskedHostIvf.calls = []
    s, r, path = st.search_filtered(q, 5, {"tenant": "nobody"})  # no file matches: padding, no search at all
    assert path == "exact" and (r.numpy() == -1).all() and np.isneginf(s.numpy()).all() and not MaskedHostIvf.calls


@pytest.mark.parametrize("mode", [None, "0", "auto", "1"])
def test_store_search_with_a_mask_is_untouched(tenants, monkeypatch, mode):
    st = tenants
    if mode is None:
        monkeypatch.delenv("RFX_IVF_FILTERED", raising=False)
    else:
        monkeypatch.setenv("RFX_IVF_FILTERED", mode)
    scans = []
    monkeypatch.setattr(HostIndex, "search", lambda self, q, k, row_mask=None: scans.append(row_mask) or "scan",
                        raising=False)
    MaskedHostIvf.calls = []
    assert st.search(vecs(1, 5), 3, row_mask="mask") == "scan" and scans == ["mask"] and not MaskedHostIvf.calls
    st.search(vecs(1, 5), 3)  # unfiltered: the lists, at the store's own nprobe, no mask
    assert [(c["nprobe"], c["row_mask"]) for c in MaskedHostIvf.calls] == [(2, None)]
