"""CPU: the corpora of tests/hostile_ivf.py hold what they promise, checked against oracle/ivf.py alone — a corpus
that has lost its edge fails here, not silently on the GPU (tests/test_gpu_ivf_hostile.py).  Also here: the
sub-scale rule of the quantiser, the tie rule restated in plain Python, and two mutants of oracle.ivf.search
(ranked by ord_f32 keys; ties by row descending) that must differ from it on the dups and "tiny" cases."""
import warnings

import numpy as np
import pytest

import hostile_ivf as hi
from oracle import ivf as oivf

_built = {}


def corpus(name, dtype="bf16"):
    if (name, dtype) not in _built:
        c = getattr(hi, name)(dtype)
        c.rows.setflags(write=False)
        _built[name, dtype] = c
    return _built[name, dtype]


def oracle_search(c, qset, nprobe, k, nq=None, rule=None):
    codes, inv, lab, fc = c.quantized()
    qq, qinv = oivf.quantize(c.queries[qset][:nq])
    if rule:
        return hi.search_by(rule, qq, qinv, codes, inv, lab, c.qc, fc, nprobe, k)
    return oivf.search(qq, qinv, codes, inv, lab, c.qc, fc, nprobe, k)


@pytest.mark.parametrize("name", ["edges", "skew", "neg", "scales"])
def test_planted_list_sizes(name):
    c = corpus(name)
    lab = c.quantized()[2]
    cnt = np.bincount(lab, minlength=c.nlist)
    if name == "scales":  # the six planted rows left their lists: the zero rows go to list 0
        assert np.abs(cnt - np.array(c.notes["sizes"])).sum() <= 12 and (lab[c.notes["zero_rows"]] == 0).all()
    else:
        assert cnt.tolist() == list(c.notes["sizes"])
    assert c.rows.shape[0] <= 16384
    # the row ids of a list are scattered: no list of 3+ rows is a run of consecutive ids
    for l in np.flatnonzero(cnt >= 3):
        m = np.flatnonzero(lab == l)
        assert m[-1] - m[0] >= len(m)
    if name == "skew":
        assert cnt.max() == 12000 and np.sort(cnt)[-2] <= 40 and (cnt == 0).sum() >= 2


def test_dups_blocks_tie_at_the_cut():
    c = corpus("dups")
    codes, inv, lab, fc = c.quantized()
    qo = c.notes["query_of"]
    s, r = oracle_search(c, "law", 3, 64)
    # A: 300 copies past the list's first 128 places, in every wave's share of the 1025-row list
    a = c.notes["block_a"]
    members = np.flatnonzero(lab == lab[a[0]])
    pos = np.searchsorted(members, a)
    assert len(a) == 300 and pos.min() >= 128 and len(set((pos // 64) % 4)) == 4 and len(members) == 1025
    assert (s[qo["a"]] == s[qo["a"], 0]).all() and np.isin(r[qo["a"]], a).all()
    # the tie rule in plain Python: the 64 lowest ids of the block
    assert r[qo["a"]].tolist() == sorted(int(x) for x in a)[:64]
    # B: 70 copies, 64 of them returned, the cut inside the tie
    b = c.notes["block_b"]
    assert len(b) == 70 and (lab[b] == hi.EDGE_SIZES.index(257)).all()
    assert (s[qo["b"]] == s[qo["b"], 0]).all() and r[qo["b"]].tolist() == sorted(int(x) for x in b)[:64]
    # C: five equal scores over two lists probed together, on top of the answer; cut them at k = 4
    cc = c.notes["block_c"]
    assert set(lab[cc].tolist()) == set(c.notes["lists_c"])
    assert r[qo["c"], :5].tolist() == cc.tolist() and (s[qo["c"], :5] == s[qo["c"], 0]).all()
    assert s[qo["c"], 5] < s[qo["c"], 4]
    s4, r4 = oracle_search(c, "law", 3, 4)
    assert r4[qo["c"]].tolist() == cc[:4].tolist() and s4[qo["c"], 3] == s[qo["c"], 4]
    qq = oivf.quantize(c.queries["law"])[0]
    assert set(c.notes["lists_c"]) <= set(oivf.probes(qq, c.qc, fc, 3)[qo["c"]].tolist())


def test_dup_centroids_tie_everywhere():
    c = corpus("dup_centroids")
    codes, inv, lab, fc = c.quantized()
    assert c.nlist == 260 and fc[c.notes["zero_centroid"]] == 0 and not c.qc[c.notes["zero_centroid"]].any()
    cs = oivf.coarse_scores(codes, c.qc, fc)
    deltas = set()
    for a, b in c.notes["pairs"]:
        assert np.array_equal(c.qc[a], c.qc[b]) and np.array_equal(cs[:, a], cs[:, b])
        assert (lab == b).sum() == 0 and (lab == a).sum() > 0  # the lower id wins every row's argmax tie
        deltas.add(b - a)
    assert deltas == {4, 32, 64, 128}
    qq = oivf.quantize(c.queries["law"])[0]
    qs = -np.sort(-oivf.coarse_scores(qq, c.qc, fc), axis=1)
    for nprobe in (1, 3):
        assert (qs[:, nprobe - 1] == qs[:, nprobe]).sum() >= len(c.notes["pairs"]), nprobe
    pr = oivf.probes(qq, c.qc, fc, 1)
    assert not np.isin(pr, [b for _, b in c.notes["pairs"]]).any()


def test_dup_sample_empties_a_list():
    c = corpus("dup_sample")
    nlist, step = c.notes["nlist"], c.notes["step"]
    xq = oivf.quantize(c.rows)[0]
    assert np.array_equal(xq[0], xq[step]) and np.array_equal(xq[0], xq[2 * step])
    qc0 = xq[np.arange(nlist) * step]
    lab = oivf.assign(xq, qc0, oivf.centroid_factor(qc0))
    cnt = np.bincount(lab, minlength=nlist)
    assert cnt[1] == 0 and cnt[2] == 0 and cnt[0] > 0 and lab[step] == 0 and lab[2 * step] == 0
    for iters in (1, 3):
        qc, _ = oivf.train(xq, nlist, iters)
        assert np.array_equal(qc[2], qc0[2])  # the empty list's centroid never moves


def test_scales_plants():
    c = corpus("scales")
    codes, inv, lab, fc = c.quantized()
    e = c.notes["exponents"]
    assert set(e.tolist()) >= set(range(-100, 101))
    small = (lab < hi.SMALL_LISTS) & (inv > 0)
    small[[c.notes["onehot_row"], c.notes["tie_row"]]] = False  # (planted at scale 1; the oracle puts them in list 0)
    assert (e[small] <= -60).all() and small.sum() > 700
    z = c.notes["zero_rows"]
    assert len(z) == 4 and not codes[z].any() and (inv[z] == 0).all()
    o = c.notes["onehot_row"]
    assert codes[o].min() == -127 and np.count_nonzero(codes[o]) == 1 and inv[o] == np.float32(1 / 127)
    t = codes[c.notes["tie_row"]].astype(np.int64)
    assert inv[c.notes["tie_row"]] == np.float32(2.0 ** -7) and t.max() == 127
    assert (t[t != 127] % 2 == 0).all()  # every rint tie went to the even neighbour
    f16 = corpus("scales", "f16")
    assert np.array_equal(f16.rows.astype(np.float16).astype(np.float32), f16.rows) and np.abs(f16.rows).max() < 65504


def test_scales_tiny_holds_both_zeros():
    c = corpus("scales")
    codes, inv, lab, fc = c.quantized()
    qq, qinv = oivf.quantize(c.queries["tiny"])
    with np.errstate(under="ignore"):
        p = (inv[:, None] * qinv[None, :]).astype(np.float32)
    tiny_min = np.float32(2.0 ** -126)
    assert ((p > 0) & (p < tiny_min)).any() and ((p == 0) & (inv[:, None] > 0)).any() and (p >= tiny_min).any()
    s, r = oracle_search(c, "tiny", 3, 64)
    both = [(s[i] == 0).any() and np.signbit(s[i][s[i] == 0]).any() and (~np.signbit(s[i][s[i] == 0])).any()
            for i in range(len(s))]
    assert sum(both) >= 4
    # a -0.0 stands in front of a +0.0 with a higher row id: the order ord_f32 keys would not give
    i = both.index(True)
    zs = np.flatnonzero(s[i] == 0)
    assert (np.diff(r[i][zs]) > 0).all()
    sb = np.signbit(s[i][zs])
    assert (sb[:-1] & ~sb[1:]).any()


def test_scales_zero_query_answer_is_known():
    c = corpus("scales")
    lab = c.quantized()[2]
    for nprobe, k in ((1, 5), (3, 64), (16, 17)):
        s, r = oracle_search(c, "zero", nprobe, k, nq=2)
        want = np.flatnonzero(lab < nprobe)[:k]
        assert (r[:, :len(want)] == want).all() and (r[:, len(want):] == -1).all()
        assert np.array_equal(s[:, :len(want)].view(np.uint32), np.zeros((2, len(want)), np.uint32))  # +0.0


def test_neg_scores_are_negative():
    c = corpus("neg")
    codes, inv, lab, fc = c.quantized()
    qq, qinv = oivf.quantize(c.queries["neg"])
    d = oivf.int_dot(qq, codes).astype(np.float32)
    s = d * (inv[None, :] * qinv[:, None])
    assert (s < 0).all()
    s, r = oracle_search(c, "neg", 3, 16)
    assert (s[r >= 0] < 0).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_subscale_rule(dtype):
    c = corpus("subscale", dtype)
    sub = c.notes["sub"]
    assert sub.tolist() == [True] * len(hi.SUB_AMAX) + [False] * len(hi.NEAR_AMAX)
    assert (c.rows == 0).any(axis=1).all() and (c.notes["amax"] > 0).all()
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no numpy warning left
        codes, inv = oivf.quantize(c.rows)
    assert not codes[sub].any() and (inv[sub] == 0).all()
    assert (np.abs(codes[~sub]).max(axis=1) == 127).all() and (inv[~sub] > 0).all()
    assert (codes[~sub][:, 7] == -127).all()
    # the rule changes no row in the quantiser's ordinary domain
    x = oivf.clustered_rows(5, 16, 9, 0, 64, 256, "f32")
    q, v = oivf.quantize(x)
    am = np.abs(x).max(axis=1)
    assert np.array_equal(v, am / np.float32(127)) and np.array_equal(
        q, np.rint(x * (np.float32(127) / am)[:, None]).astype(np.int8))


def test_padded_tail_case_exists():
    c = corpus("edges")
    s, r = oracle_search(c, "law", 1, 64, nq=33)
    assert (r == -1).any() and np.isneginf(s[r == -1]).all()


# ---- sensitivity: mutants of the ranking rule must fail the GPU tests' comparison --------------------------
def test_restated_search_is_the_oracle():
    for name, qset in (("dups", "law"), ("scales", "tiny")):
        c = corpus(name)
        assert hi.same_bits(*oracle_search(c, qset, 3, 64, rule="oracle"), *oracle_search(c, qset, 3, 64))


@pytest.mark.parametrize("rule,name,qset,differs", [
    ("ord", "scales", "tiny", True), ("row_desc", "scales", "tiny", True), ("row_desc", "dups", "law", True),
    ("ord", "dups", "law", False)])  # (no zero scores in dups: the ord_f32 order is the oracle's there)
@pytest.mark.parametrize("k", [4, 16, 64])
def test_mutants_fail_the_comparison(rule, name, qset, differs, k):
    c = corpus(name)
    ref = oracle_search(c, qset, 3, k)
    got = oracle_search(c, qset, 3, k, rule=rule)
    assert hi.same_bits(*got, *ref) != differs
