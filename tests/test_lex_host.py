"""CPU: the lexical index's exports, the numpy reference's own properties (tests/lex_ref.py), and the
sanitized stand-alone program over csrc/lex_host.h."""
import os
import re
import subprocess

import numpy as np
import lex_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEX_SYMBOLS = ("rfx_lex_create", "rfx_lex_destroy", "rfx_lex_add", "rfx_lex_tombstone", "rfx_lex_info", "rfx_lex_df",
               "rfx_lex_search_workspace_bytes", "rfx_lex_search", "rfx_lex_fuse")


def test_exports_exist():
    from rfx import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rfx_\w+)", out))
    header = open(os.path.join(ROOT, "include", "rfx.h")).read()
    for s in LEX_SYMBOLS:
        assert s in exported and s in _lib.SIGNATURES and re.search(r"^int %s\(" % s, header, re.M), s
    from rfx import lexical
    for m in ("add_csr", "add_texts", "tombstone", "df", "search", "fuse", "close"):
        assert callable(getattr(lexical.LexIndex, m))


def test_build_id_covers_the_new_sources():
    from rfx import _lib
    names = sorted(f for f in os.listdir(_lib.CSRC) if f.endswith((".hip", ".h", ".cpp")))
    for f in ("k_lex.h", "k_lex.hip", "k_fuse.h", "k_fuse.hip", "lex_api.hip", "lex_host.h"):
        assert f in names
    assert _lib.BUILD_ID == _lib.SOURCE_HASH
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    for f in ("k_lex.hip", "k_fuse.hip", "lex_api.hip"):
        assert f in mk


def test_rrf_alpha_one_is_the_dense_prefix_and_zero_the_lexical_prefix():
    dense = [5, 9, 2, 7, 11, 3]
    lex = [7, 40, 5, 41, 42, 43]
    for k in (1, 3, 6):
        assert lex_ref.rrf(dense, lex, k, 1.0)[1].tolist() == dense[:k]
        assert lex_ref.rrf(dense, lex, k, 0.0)[1].tolist() == lex[:k]
    # padding inside a list does not count as a rank
    s, r, kk = lex_ref.rrf([5, -1, 9], [-1, 9], 3, 0.5)
    assert r.tolist() == [9, 5, -1] and kk.tolist() == [[2, 1], [1, 0], [0, 0]] and np.isneginf(s[2])


def test_rrf_is_prefix_stable_and_rewards_agreement():
    rng = np.random.default_rng(3)
    for _ in range(50):
        dense = rng.permutation(200)[:40]
        lex = rng.permutation(200)[:40]
        a = float(rng.random())
        s64, r64, k64 = lex_ref.rrf(dense, lex, 64, a)
        s10, r10, k10 = lex_ref.rrf(dense, lex, 10, a)
        assert np.array_equal(r64[:10], r10) and np.array_equal(s64[:10], s10) and np.array_equal(k64[:10], k10)
    # a row in both lists beats a row at the same rank in one only
    s, r, _ = lex_ref.rrf([1, 2, 3], [4, 2, 5], 5, 0.5)
    assert r[0] == 2 and s[0] > s[1]
    # exact f64 tie (ranks (1, 2) and (2, 1) at alpha 0.5): the lower row first
    s, r, kk = lex_ref.rrf([8, 3], [3, 8], 2, 0.5)
    assert r.tolist() == [3, 8] and s[0] == s[1] and kk.tolist() == [[2, 1], [1, 2]]


def test_statistics_after_add_and_tombstone_equal_a_fresh_build():
    csr = lex_ref.gen_csr(21, 600, V=512, max_len=60)
    ref = lex_ref.RefIndex(512)
    ref.add(*lex_ref.slice_csr(csr, 0, 250))
    ref.add(*lex_ref.slice_csr(csr, 250, 600))
    dead = np.arange(0, 600, 7)
    ref.tombstone(dead)
    fresh, old = ref.fresh()
    N, df, total = ref.stats()
    N2, df2, total2 = fresh.stats()
    assert (N, total) == (N2, total2) and np.array_equal(df, df2) and N == 600 - dead.size
    # ... and so are the scores, row for row
    for qb, qc in lex_ref.gen_questions(4, 5, V=512):
        s, ranks = ref.scores(qb, qc)
        s2, ranks2 = fresh.scores(qb, qc)
        assert np.array_equal(s[old], s2) and np.array_equal(ranks[old], ranks2) and not ranks[dead].any()


def test_reference_topk_order_and_padding():
    ref = lex_ref.RefIndex(64)
    # rows 0 and 2 are identical (an exact tie), row 1 shares nothing with the question
    ref.add(*lex_ref.question_csr([([3, 9], [2, -1]), ([5], [1]), ([3, 9], [2, -1]), ([9], [4]), ([], [])]))
    s, r, _ = ref.topk([3, 9], [1, 3], 5)
    assert r[:2].tolist() == [0, 2] and s[0] == s[1] and r[2] == 3 and r[3:].tolist() == [-1, -1]
    assert np.all(s[:3] > 0) and np.all(np.isneginf(s[3:]))
    assert ref.topk([7], [1], 3)[1].tolist() == [-1, -1, -1]  # a bucket no row holds


def test_generator_seeds_keep_near_ties_rare():
    """The GPU tests leave a question out of the row comparison when the reference's own scores hold two
    neighbours within one f32 ulp; with their seeds the reference alone stays under 2 % of the questions."""
    csr = lex_ref.gpu_corpus()
    ref = lex_ref.RefIndex(lex_ref.GPU_V)
    ref.add(*csr)
    _, allowed = lex_ref.gpu_mask_words()
    for name, (qs, ks, params, masked) in lex_ref.gpu_question_sets(csr).items():
        for k1, b in params:
            # (the positions 1..k+1 of a smaller k are a prefix of the largest k's: one pass covers them)
            close = sum(ref.topk(qb, qc, max(ks), k1, b, allowed if masked else None)[2] for qb, qc in qs)
            assert close <= 0.02 * len(qs), (name, k1, b, close)


def test_lex_host_check_under_sanitizers(tmp_path):
    """tools/lex_host_check.cpp: the append / tombstone / statistics / weight-table / argument logic of
    csrc/lex_host.h in a stand-alone host program under AddressSanitizer and UBSan (no device, no preload)."""
    exe = str(tmp_path / "lex_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "rag-foundation_amd", "csrc"),
                    os.path.join(ROOT, "tools", "lex_host_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "lex_host_check: ok" in p.stdout, p.stdout + p.stderr


def test_parse_hybrid_argument():
    import pytest
    from rfx.retriever import default_fetch_k, parse_hybrid
    assert parse_hybrid(None, 5) is None
    assert parse_hybrid(0.25, 10) == (0.25, default_fetch_k(10), 60, 1.2, 0.75)
    assert parse_hybrid(1, 3) == (1.0, 16, 60, 1.2, 0.75) and parse_hybrid(0, 64)[1] == 64
    assert parse_hybrid({"alpha": 0.5, "fetch_k": 12, "rrf_c": 1, "k1": 0.0, "b": 1.0}, 12) == (0.5, 12, 1, 0.0, 1.0)
    for bad in (1.5, -0.1, float("nan"), True, "0.5", {"fetch_k": 8}, {"alpha": 0.5, "fetch_k": 4},
                {"alpha": 0.5, "fetch_k": 65}, {"alpha": 0.5, "fetch_k": 8.5}, {"alpha": 0.5, "rrf_c": 0},
                {"alpha": 0.5, "b": 1.5}, {"alpha": 0.5, "k1": -1.0}, {"alpha": 0.5, "k1": float("nan")},
                {"alpha": 0.5, "lambda": 0.5}):
        with pytest.raises(ValueError):
            parse_hybrid(bad, 5)


def test_hybrid_refusals_on_stand_in_stores(tmp_path):
    """hybrid= together with diversity=, on a store whose index is not a flat single-device one (the host
    stand-in has no device selection, as a sharded index has none), and on an IVF store: one fixed message."""
    import pytest
    from fakes import HostIndex, HostIvf
    from rfx import store as rstore
    from rfx.retriever import HYBRID_ERROR, GpuRetriever
    reg = rstore.StoreRegistry(root=str(tmp_path / "root"), device=0, index_factory=HostIndex, ivf_factory=HostIvf)
    ret = GpuRetriever(registry=reg, dim=64, dtype="f32")
    ret.batching = False
    flat = reg.create("flat", 64, "f32")
    ivf = reg.create("lists", 64, "f32", spec={"kind": "ivf", "nlist": 4, "nprobe": 2, "train_min": 1000})
    vecs = np.eye(64, dtype=np.float32)[:3]
    for st in (flat, ivf):
        st.add_document(["a b", "c d", "e f"], vecs, "doc")
    with pytest.raises(ValueError, match=HYBRID_ERROR):
        ret.search([flat.name], "a b", 2, hybrid=0.5, diversity=0.5)
    with pytest.raises(ValueError, match=HYBRID_ERROR):
        ret.search([flat.name], "a b", 2, hybrid=0.5)
    with pytest.raises(ValueError, match=HYBRID_ERROR):
        ret.search([ivf.name], "a b", 2, hybrid={"alpha": 0.0})
    with pytest.raises(ValueError, match=HYBRID_ERROR):
        ret.search_store(flat.name, "a b", 2, hybrid=(0.5, 16, 60, 1.2, 0.75))
    assert ret.last_hybrid is None and flat._lex is None and ivf._lex is None  # nothing lexical was built
