"""CPU: the reference of the IVF search of a batch under different filters, and the store's plan around it
(DESIGN §4.16).

1. tests/ivf_multi_ref.py's reference (ivf_mask_ref.search once per question) equals the definition written out.
2. Three mutants — every question under question 0's mask; every question at the batch's largest probe count; the
   mask applied to a finished top-k — differ from the reference on every case of the GPU grid where they can: more
   than one distinct selection in use, more than one probe count in use, a selection that is not all ones.  Every
   case is non-trivial for at least one mutant but the all-equal one-question cases: the grid discriminates.
3. LocalStore.search_lists_filtered_multi with host stand-ins (tests/fakes.py): equal filters share a mask, each
   filter gets its own rule value, one search_index call; the declined set under auto at the cap.
4. The built library exports the new symbols."""
import numpy as np
import pytest

import hostile_ivf as hi
import ivf_mask_ref as mr
import ivf_multi_ref as mu
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


def args_of(c, nq):
    codes, inv, lab, fc = c.quantized()
    qq, qinv = oivf.quantize(c.queries["law"][:nq])
    return qq, qinv, codes, inv, lab, c.qc, fc


# ---- 1. the reference is the definition --------------------------------------------------------------------
@pytest.mark.parametrize("name,table,holes,order,k,nq,probes", [("edges", "comp", False, "shuffle", 17, 5, "mix"),
                                                                ("dups", "nine", True, "group", 5, 9, "mix"),
                                                                ("edges", "perq", False, "shuffle", 64, 4, 3)])
def test_reference_is_the_definition(name, table, holes, order, k, nq, probes):
    c = corpus(name)
    a = args_of(c, nq)
    names, mo, npr = mu.build(c, table, holes, order, 1, nq, probes)
    sels = mu.selections(c, names, mo, 1, nq)
    s, r = mu.search(*a, npr, k, sels)
    bs, br = mu.brute_force(*a, npr, k, sels)
    assert hi.same_bits(s, r, bs, br)
    for i in range(nq):
        assert sels[i][r[i][r[i] >= 0]].all()


def test_builders():
    lab = corpus("edges").quantized()[2]
    for nq in (9, 33):
        rot = [mu.selection(f"rot{i}", lab, 1, nq) for i in range(nq)]
        assert len({x.tobytes() for x in rot}) == nq  # nq distinct masks
    assert np.array_equal(mu.selection("~alt", lab), ~mr.selection("alt", lab))
    assert mu.mask_of(0, 9, True, "group").tolist() == [-1] * 9
    g = mu.mask_of(8, 33, False, "group")
    assert (np.diff(g) >= 0).all() and set(g) == set(range(8))
    s = mu.mask_of(8, 33, False, "shuffle")
    assert sorted(s) == sorted(g) and (np.diff(s) < 0).any()
    assert (mu.mask_of(2, 33, True, "group")[1::4] == -1).all()
    assert set(mu.probe_counts("mix", 9, 24)) == {1, 3, 24} and set(mu.probe_counts("most1", 9, 100)) == {1, 64}


# ---- 2. the cases discriminate -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges", "skew", "dups"])
def test_mutants_differ_on_every_case(name):
    c = corpus(name)
    lab = c.quantized()[2]
    for case in mu.CASES:
        cname, table, holes, order, splits, k, nq, probes = case
        if cname != name:
            continue
        a = args_of(c, nq)
        names, mo, npr = mu.build(c, table, holes, order, splits, nq, probes)
        sels = mu.selections(c, names, mo, splits, nq)
        ref = mu.search(*a, npr, k, sels)
        applicable = {
            "first mask": len({x.tobytes() for x in sels}) > 1,
            "largest nprobe": len(set(npr.tolist())) > 1,
            "mask after the top-k": any(not x.all() and x.any() for x in sels),
        }
        fns = {"first mask": mu.mutant_first_mask, "largest nprobe": mu.mutant_max_nprobe,
               "mask after the top-k": mu.mutant_after_topk}
        assert any(applicable.values()) or nq == 1, f"{case}: no mutant applies"
        for what, on in applicable.items():
            if on:
                got = fns[what](*a, npr, k, sels)
                assert not hi.same_bits(got[0], got[1], *ref), f"{case}: the mutant '{what}' passes"
        assert len(lab) % 32


def test_cases_cover_every_value():
    for name in ("edges", "skew", "dups"):
        mine = [c for c in mu.CASES if c[0] == name]
        assert {m[4] for m in mine} == {1, 2, 4}, name
        assert {m[5] for m in mine} >= {1, 4, 5, 16, 17, 64}, name
        assert {m[6] for m in mine} == {1, 9, 33}, name
        assert {m[2] for m in mine} == {True, False} and {m[3] for m in mine} == {"group", "shuffle"}
        assert {len(mu.table_names(m[1], m[6])) for m in mine} >= {1, 2, 8, 9, 33}, name
        assert {"mix"} <= {m[7] for m in mine} and any(isinstance(m[7], int) for m in mine)
    assert {corpus(n).rows.shape[1] for n in ("edges", "skew", "dups")} == {256, 768}
    assert any(c[1] == "comp" and c[3] == "shuffle" and c[7] == mu.FULL and c[6] == 33 for c in mu.CASES)
    assert any(c[1] == "same" for c in mu.CASES)


# ---- 3. the store plan, host stand-ins ---------------------------------------------------------------------
SPEC = {"kind": "ivf", "nlist": 16, "nprobe": 2, "train_min": 16}


class MultiHostIvf(HostIvf):
    """HostIvf whose search_index takes the per-question form: one question at a time at its own probe count over
    the rows its own mask selects (unselected rows NaN: HostIvf drops NaN scores before ranking)."""
    calls = []

    def search_index(self, queries, k, nprobe, index, rerank_k=None, row_mask=None, row_masks=None, mask_of=None,
                     nprobes=None):
        import torch
        MultiHostIvf.calls.append({"k": k, "nprobe": nprobe, "rerank_k": rerank_k, "row_mask": row_mask,
                                   "row_masks": row_masks, "mask_of": mask_of, "nprobes": nprobes, "nq": len(queries)})
        if row_masks is None and row_mask is None:
            return super().search_index(queries, k, nprobe, index, rerank_k)
        if row_masks is None:  # the one-mask form
            row_masks, mask_of, nprobes = [row_mask], [0] * len(queries), [nprobe] * len(queries)
        out = []
        for i, q in enumerate(np.asarray(queries)):
            sel = mr.from_words(row_masks[mask_of[i]], self.rows)

            class Masked:
                @staticmethod
                def read(r0, n, sel=sel):
                    x = index.read(r0, n).copy()
                    x[~sel[r0:r0 + n]] = np.nan
                    return x
            out.append(super().search_index(q[None], k, nprobes[i], Masked, rerank_k))
        return torch.cat([s for s, _ in out]), torch.cat([r for _, r in out])


def vecs(n, seed, dim=32):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


@pytest.fixture
def tenants(tmp_path):
    """64 rows: tenant t0 32 rows, t1 16, t2 8 + a deleted 8-row file of t2: live 56."""
    MultiHostIvf.calls = []
    reg = rstore.StoreRegistry(root=str(tmp_path), device=0, index_factory=HostIndex, ivf_factory=MultiHostIvf)
    st = reg.create("demo", 32, "f32", spec=SPEC)
    st.add_document(["a"] * 32, vecs(32, 1), "a.md", metadata={"tenant": "t0"})
    st.add_document(["b"] * 16, vecs(16, 2), "b.md", metadata={"tenant": "t1"})
    st.add_document(["c"] * 8, vecs(8, 3), "c.md", metadata={"tenant": "t2"})
    dead = st.add_document(["d"] * 8, vecs(8, 4), "d.md", metadata={"tenant": "t2"})[0]
    st.delete_file(dead)
    assert st.ivf_ready() and st.dead_rows() == 8
    return st


T = [{"tenant": f"t{i}"} for i in range(3)]
SPAN = {0: (0, 32), 1: (32, 48), 2: (48, 56)}


def test_one_search_for_all_filters(tenants, monkeypatch):
    st = tenants
    monkeypatch.setenv("RFX_IVF_FILTERED", "auto")
    q = vecs(7, 9)
    who = [1, 0, 2, 0, 1, 1, 2]
    MultiHostIvf.calls = []
    s, r, declined = st.search_lists_filtered_multi(q, 5, [T[w] for w in who])
    assert declined == [] and len(MultiHostIvf.calls) == 1  # the rules, the masks and the search: once
    call = MultiHostIvf.calls[0]
    # t0: 32 of 56 live rows -> ceil(2 * 56 / 32) = 4 probes; t1: 16 of 56 -> 7; t2: 8 of 56 -> 14
    assert len(call["row_masks"]) == 3 and call["nq"] == 7  # equal filters share a mask
    assert call["nprobe"] == 14 and call["k"] == 5 and call["rerank_k"] == 16 and call["row_mask"] is None
    assert sorted(call["nprobes"]) == sorted({0: 4, 1: 7, 2: 14}[w] for w in who)
    assert list(call["mask_of"]) == sorted(call["mask_of"])  # the questions go out in filter-group order
    for m, npb in zip(call["mask_of"], call["nprobes"]):
        w = [t for t in range(3) if call["row_masks"][m] is st.row_mask(T[t])]
        assert len(w) == 1 and npb == {0: 4, 1: 7, 2: 14}[w[0]]
    r = r.numpy()
    for i, w in enumerate(who):  # each answer is the one-filter call's, in the caller's order
        lo, hi_ = SPAN[w]
        assert ((r[i] >= lo) & (r[i] < hi_) | (r[i] == -1)).all() and (r[i] >= 0).any()
        one_s, one_r = st.search_lists_filtered(q[i:i + 1], 5, T[w])
        assert np.array_equal(one_r.numpy()[0], r[i]) and np.array_equal(one_s.numpy()[0], s.numpy()[i])


def test_declined_under_auto_at_the_cap(tenants, monkeypatch):
    st = tenants
    monkeypatch.setenv("RFX_IVF_FILTERED", "auto")
    monkeypatch.setitem(st.spec, "nprobe", 3)  # t0: ceil(3 * 56 / 32) = 6, t1: 11, t2: 21 > cap 16: declined
    q = vecs(5, 9)
    who = [2, 0, 1, 2, 0]
    MultiHostIvf.calls = []
    s, r, declined = st.search_lists_filtered_multi(q, 4, [T[w] for w in who] )
    assert declined == [0, 3] and len(MultiHostIvf.calls) == 1
    call = MultiHostIvf.calls[0]
    assert call["nq"] == 3 and len(call["row_masks"]) == 2 and sorted(call["nprobes"]) == [6, 6, 11]
    assert call["nprobe"] == 11
    assert (r.numpy()[declined] == -1).all() and np.isneginf(s.numpy()[declined]).all()
    assert (r.numpy()[[1, 2, 4]] >= 0).any(axis=1).all()
    nobody = {"tenant": "nobody"}  # a filter that matches no file is declined too (the caller answers None)
    out = st.search_lists_filtered_multi(q[:2], 4, [nobody, T[0]])
    assert out[2] == [0]
    monkeypatch.setenv("RFX_IVF_FILTERED", "1")  # mode 1: t2 at the cap
    MultiHostIvf.calls = []
    s, r, declined = st.search_lists_filtered_multi(q, 4, [T[w] for w in who])
    assert declined == [] and sorted(MultiHostIvf.calls[0]["nprobes"]) == [6, 6, 11, 16, 16]
    monkeypatch.setenv("RFX_IVF_FILTERED", "auto")
    monkeypatch.setitem(st.spec, "nprobe", 10)  # every filter past the cap: nothing takes the lists
    MultiHostIvf.calls = []
    assert st.search_lists_filtered_multi(q, 4, [T[w] for w in who]) is None and not MultiHostIvf.calls
    monkeypatch.setenv("RFX_IVF_FILTERED", "0")
    monkeypatch.setitem(st.spec, "nprobe", 2)
    assert st.search_lists_filtered_multi(q, 4, [T[w] for w in who]) is None and not MultiHostIvf.calls
    with pytest.raises(ValueError):
        st.search_lists_filtered_multi(q, 4, [T[0]])


def test_multi_mode_switch(monkeypatch):
    monkeypatch.delenv("RFX_IVF_MULTI", raising=False)
    assert rstore.ivf_multi_mode() is True
    monkeypatch.setenv("RFX_IVF_MULTI", "0")
    assert rstore.ivf_multi_mode() is False
    monkeypatch.setenv("RFX_IVF_MULTI", "1")
    assert rstore.ivf_multi_mode() is True


# ---- 4. the library ------------------------------------------------------------------------------------------
def test_new_symbols_are_exported():
    from rfx import _lib
    for name in ("rfx_ivf_search_multi", "rfx_ivf_search_rerank_multi"):
        assert name in _lib.SIGNATURES and getattr(_lib.lib, name) is not None
    assert len(_lib.SIGNATURES["rfx_ivf_search_multi"][0]) == 18
    assert len(_lib.SIGNATURES["rfx_ivf_search_rerank_multi"][0]) == 21
