"""GPU: the exact two-pass scan (kernel 10 in its 8-wave and 2-wave forms, kernel 11, the quantiser of
k_screen.hip and the select) on the hostile corpora of tests/hostile.py — what oracle.synth's
isotropic unit rows never reach: tile scales 2^30 apart and live all-zero tiles (fold_mask_int's zero-scale
branch, its +-2^30 clamps, rcp of a tiny scale), negative k-th scores (the `tf <= 0` side of the integer
bound, orderable thresholds of negative floats beside the "0 = no bound yet" code), rint ties and codes at
+-127, a tombstone that collapses a tile's scale, and a shared-mean corpus whose thousands of survivors send
the batch to the gated exact pass without being forced to.

Bars as tests/test_gpu_screen.py: oracle/search.py's brute-force f64 top-k over the same stored bits, compared
through check_topk; the unit-norm tolerances scaled by the data, tol = 1e-5 S and tie band = 2e-6 S with
S = max(1, max ||x|| max ||q||) (scores are fl32 of the f64 dot: `mixed` reaches ~150).  tests/
test_screen_hostile_oracle.py shows on the CPU that the rule itself is exact on these corpora.

Forms (search_plan asserted): 8-wave kernel 10 at nq 256 and 100, 2-wave kernel 10 at nq 32, kernel 11 at nq 1
(k 1, 10, 64), 4 and 8.  Every kernel-10 case also runs through rfx_search_staged on 8 workgroups (> 64 tiles
a workgroup: the threshold tightens again and again).  Each search prints its fallback flag and survivors
("hostile: ..." lines, quoted in DESIGN §4.10); OWN lists the (corpus, type) pairs whose answer must be the
screen's own (fallback clear, >= k survivors a query): a green run is not the exact kernel's alone.  Kernel
11's gate word (no survivor counts) is read through rfx_screen_valu_diag and asserted clear for the same corpora.
"""
import numpy as np
import pytest
import torch

import hostile
from oracle import screen as oscreen
from oracle import search as osearch
from test_gpu_screen_lean import _assert_own_answer, _staged

pytestmark = pytest.mark.gpu

NQ = 256
# rows: 751 tiles (bf16 d 768) and 626 tiles (the other types), the last tile ragged; 8 workgroups: 78 .. 94 tiles each
SIZES = {("bf16", 768): 24_017, ("f16", 1024): 20_011, ("f32", 768): 20_011}
TORCH = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
W8, W2, K11 = "8-wave", "2-wave", "kernel 11"
FORMS = [(W8, 256, 10), (W8, 100, 10), (W2, 32, 10), (K11, 1, 1), (K11, 1, 10), (K11, 1, 64), (K11, 4, 10), (K11, 8, 10)]
PLAN = {W8: 10, W2: 10, K11: 11}
# (corpus, type) pairs whose answer must be the screen's own on both kernel-10 forms, at the plan's own workgroups
# (the flag was clear for them on the first GPU run of these corpora; profiles/r11/screen_hostile.txt).  Not listed: aniso (thousands
# of survivors: the natural fallback, test_natural_fallback); zeros_a, whose 32 zero rows put 16 equal scores into
# each of two lanes' lists of 10 (the duplicate-heavy case); mixed at f16 and f32, 20,011 rows: the survivors sit in
# the ~20 tiles of the largest scale, three of them in one workgroup's share overflow a lane's list inside the band.
OWN = {("mixed", "bf16"), ("shifted", "bf16"), ("zeros_b", "bf16"), ("zeros_b", "f16"), ("zeros_b", "f32"),
       ("zeros_c", "bf16"), ("zeros_d", "bf16")}
# kernel 11 (its gate word through rfx_screen_valu_diag) must answer the OWN corpora and `mixed` at f32 itself, at every
# (nq, k) but these of `mixed`: a block's list of 16 (64 for k > 16) overflows inside the band where tiles of the
# largest scale stand side by side in its share (the flags of the GPU run, profiles/r11/screen_hostile.txt)
OWN_K11 = OWN | {("mixed", "f32")}
K11_FALLS_BACK = {("mixed", "bf16", 1, 10), ("mixed", "bf16", 1, 64), ("mixed", "bf16", 4, 10), ("mixed", "bf16", 8, 10),
                  ("mixed", "f32", 1, 64), ("mixed", "f32", 8, 10)}
# corpora whose search cut into 8 workgroups (16 lists of 10 a query) must answer itself too: zeros (d), 15 rows
# inside the band, all over the store
OWN8 = {"zeros_d"}


@pytest.fixture(scope="module")
def rindex():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rfx.index as ri
    return ri


_corpora, _indexes, _refs = {}, {}, {}


def _corpus(name, dtype="bf16", d=768):
    key = (name, dtype, d)
    if key not in _corpora:
        n = SIZES[(dtype, d)]
        if name in ("aniso", "shifted", "mixed"):
            c = getattr(hostile, name)(n, d, dtype, NQ)
        else:
            c = hostile.zeros(n, d, dtype, NQ, name[-1])
        c.rows.setflags(write=False)
        live = hostile.live_rows(c).astype(np.float64)
        live.setflags(write=False)
        _corpora[key] = (c, live)
    return _corpora[key]


def _dev(x32, dtype):
    t = torch.from_numpy(np.array(x32, dtype=np.float32)).to(TORCH[dtype])  # (a copy: the corpora are read-only)
    assert np.array_equal(t.float().numpy(), x32)  # the upload holds the oracle's bits
    return t.cuda()


def _index(rindex, name, dtype="bf16", d=768, shared=True):
    """The screened store of a corpus, built once per module (never written to by the tests that share it)."""
    key = (name, dtype, d)
    if not shared or key not in _indexes:
        c, _ = _corpus(name, dtype, d)
        ix = rindex.DeviceIndex(d, dtype)
        ix.add(_dev(c.rows, dtype))
        ix.enable_screen(1)
        if c.dead:
            ix.tombstone(c.dead)
        if not shared:
            return ix
        _indexes[key] = ix
    return _indexes[key]


def _queries(name, qset, nq, dtype="bf16", d=768):
    c, _ = _corpus(name, dtype, d)
    q32 = c.queries[qset][:nq]
    return _dev(q32, dtype), q32.astype(np.float64)


def _reference(key, q64, rows64, k):
    """osearch.topk over the live rows, computed once per (corpus, queries, k, mask)."""
    if key not in _refs:
        _refs[key] = osearch.topk(q64, rows64, k)
    return _refs[key]


def _verify(s, r, ref, rows64, q64):
    S = hostile.scale_bound(rows64, q64)
    probs = osearch.check_topk(s.cpu().numpy(), r.cpu().numpy(), ref[0], ref[1], lambda qi, rr: rows64[rr] @ q64[qi],
                               tol=1e-5 * S, tie_band=2e-6 * S)
    assert not probs, probs[:5]


def _diag(ix, nq, k, ws, tag):
    diag, fb = ix.screen_diag(nq, k, ws)
    sv = diag[:, 1]
    print(f"hostile: {tag}: fallback {int(fb)}, survivors min {sv.min()} mean {sv.mean():.0f} max {sv.max()}, "
          f"kept candidates max {diag[:, 0].max()}")
    return fb


def _mask(allowed):
    words = np.zeros((allowed.size + 31) // 32, dtype=np.uint32)
    idx = np.nonzero(allowed)[0]
    np.bitwise_or.at(words, idx >> 5, (np.uint64(1) << (idx & 31).astype(np.uint64)).astype(np.uint32))
    return torch.from_numpy(words.view(np.int32)).cuda()


def _search_and_check(ix, name, qset, dtype, d, form, nq, k, allowed=None):
    """One form's search (and, for kernel 10, the same search on 8 workgroups) against the oracle; returns the
    answer of the plan's own layout."""
    _, live = _corpus(name, dtype, d)
    rows64 = live
    if allowed is not None:
        rows64 = live.copy()
        rows64[~allowed] = np.nan
    m = _mask(allowed) if allowed is not None else None
    q, q64 = _queries(name, qset, nq, dtype, d)
    assert ix.search_plan(nq, k) == PLAN[form], (form, ix.search_plan(nq, k))
    ref = _reference((name, qset, dtype, d, nq, k, allowed is not None), q64, rows64, k)
    tag = f"{name}/{qset} {dtype} d {d}{' masked' if m is not None else ''}, {form} nq {nq} k {k}"
    ws = torch.empty(ix.workspace_bytes(nq, k), dtype=torch.uint8, device="cuda")
    s, r = ix.search(q, k, workspace=ws, row_mask=m)
    torch.cuda.synchronize()
    if form == K11:
        fb = ix.screen_valu_diag()  # kernel 11's gate word: no survivor counts
        print(f"hostile: {tag}: fallback {int(fb)}")
    else:
        _diag(ix, nq, k, ws, tag)
    _verify(s, r, ref, rows64, q64)
    own = allowed is None and (name, dtype) in OWN
    if form == K11:
        if allowed is None and (name, dtype) in OWN_K11 and (name, dtype, nq, k) not in K11_FALLS_BACK:
            assert not fb  # the answer checked above was kernel 11's screen's own
    else:
        s8, r8, ws8 = _staged(ix, q, k, 8, row_mask=m)
        _diag(ix, nq, k, ws8, tag + ", 8 workgroups")
        _verify(s8, r8, ref, rows64, q64)
        # one score rule: whichever of the screen and the gated exact pass answered, the same bits
        assert torch.equal(r8, r) and torch.equal(s8, s)
        if own:
            _assert_own_answer(ix, nq, k, ws)  # the answer checked above was the screen's own
        if name in OWN8:
            _assert_own_answer(ix, nq, k, ws8)  # and so was the 8-workgroup one: a long-running screen's
    return s, r


# ---- 1. the int8 copy -----------------------------------------------------------------------------------------
def _copy_equals_oracle(ix, rows32, stats_too):
    nt = (rows32.shape[0] + 31) // 32
    codes, scales, live, stats = ix.screen_read(0, nt)
    rc, rs, rl, rst = oscreen.quantize_tiles(rows32)
    assert codes.tobytes() == rc.tobytes()
    assert scales.tobytes() == rs.tobytes()
    assert live.tobytes() == rl.tobytes()
    if stats_too:
        assert np.allclose(stats[:2], rst[:2], rtol=2e-7, atol=0) and stats[2] == rst[2] == scales.max()
    return scales


@pytest.mark.parametrize("name,dtype,d", [("mixed", "bf16", 768), ("aniso", "bf16", 768), ("mixed", "f16", 1024),
                                          ("mixed", "f32", 768)])
def test_int8_copy_bit_exact(rindex, name, dtype, d):
    c, _ = _corpus(name, dtype, d)
    _copy_equals_oracle(_index(rindex, name, dtype, d), hostile.live_rows(c), True)


def test_tombstones_that_collapse_a_tile_scale(rindex):
    """The row holding a tile's largest element goes: of the tile with the store's largest scale (max s_t is then
    a stale upper bound, which is legal: the stats are not compared), of the one-hot tile (scale 1/127 -> 0: a live
    all-zero tile) and of the tie tile (2^-7 -> 126.5 / 127 2^-7: no element sits on a tie any more)."""
    c, _ = _corpus("mixed")
    ix = _index(rindex, "mixed", shared=False)
    scales = oscreen.quantize_tiles(c.rows)[1]
    top = int(np.argmax(scales))
    blk = np.abs(c.rows[top * 32:(top + 1) * 32])
    dead = [top * 32 + int(np.unravel_index(np.argmax(blk), blk.shape)[0]), c.notes["onehot_row"], c.notes["tie_row"]]
    ix.tombstone(dead)
    rows32 = c.rows.copy()
    rows32[dead] = np.nan
    after = _copy_equals_oracle(ix, rows32, False)
    assert after[top] < scales[top] and after[c.notes["onehot_tile"]] == 0 and after[c.notes["tie_tile"]] < 2.0 ** -7
    rows64 = rows32.astype(np.float64)
    for form, nq, k in ((W8, 256, 10), (W2, 32, 10), (K11, 1, 10)):
        q, q64 = _queries("mixed", "iso", nq)
        assert ix.search_plan(nq, k) == PLAN[form]
        s, r = ix.search(q, k)
        torch.cuda.synchronize()
        _verify(s, r, osearch.topk(q64, rows64, k), rows64, q64)
    ix.close()


# ---- 2. answers against the oracle ------------------------------------------------------------------------------
BF16 = [("aniso", "same"), ("aniso", "neg"), ("shifted", "lean"), ("mixed", "iso"), ("zeros_a", "lean"),
        ("zeros_b", "lean")]
CASES = [(n, qs, "bf16", 768, f, nq, k) for n, qs in BF16 for f, nq, k in FORMS]
# zeros (c): the -2^30 clamp (a negative bound over a tile of scale 2^-30), one case a form
CASES += [("zeros_c", "lean", "bf16", 768, f, nq, 10) for f, nq in ((W8, 256), (W2, 32), (K11, 1), (K11, 8))]
# zeros (d): few survivors, so that the search on 8 workgroups (> 64 tiles each, thresholds below zero that
# tighten from tile to tile) answers itself
CASES += [("zeros_d", "lean", "bf16", 768, f, nq, 10) for f, nq in ((W8, 256), (W2, 32), (K11, 1), (K11, 8))]
CASES += [(n, qs, "f16", 1024, f, nq, k) for n, qs in BF16[3:] for f, nq, k in FORMS if f != K11]
CASES += [(n, qs, "f32", 768, f, nq, k) for n, qs in BF16[3:] for f, nq, k in FORMS if f != W8]


@pytest.mark.parametrize("name,qset,dtype,d,form,nq,k", CASES)
def test_answers_match_oracle(rindex, name, qset, dtype, d, form, nq, k):
    _search_and_check(_index(rindex, name, dtype, d), name, qset, dtype, d, form, nq, k)


@pytest.mark.parametrize("form,nq,k", [(W8, 256, 10), (W2, 32, 10), (K11, 1, 10), (K11, 8, 10)])
@pytest.mark.parametrize("name,qset", [("aniso", "same"), ("mixed", "iso")])
def test_row_mask(rindex, name, qset, form, nq, k):
    allowed = np.random.default_rng(3).random(SIZES[("bf16", 768)]) < 0.3
    _search_and_check(_index(rindex, name), name, qset, "bf16", 768, form, nq, k, allowed=allowed)


# ---- 3. exactly known answers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,nq", [(W8, 256), (W2, 32), (K11, 8)])
@pytest.mark.parametrize("variant", ["a", "b"])
def test_zero_rows_come_first_in_row_order(rindex, variant, form, nq):
    """Every other score is negative: the zero rows lead in row order with score exactly 0.0 (the tie rule of
    test_appends_tombstones_and_ties), then the best negatives under the score rule (fl32 of the f64 dot
    descending, row ascending)."""
    name = "zeros_" + variant
    c, _ = _corpus(name)
    ix = _index(rindex, name)
    assert ix.search_plan(nq, 10) == PLAN[form]
    q, _ = _queries(name, "lean", nq)
    s, r = ix.search(q, 10)
    torch.cuda.synchronize()
    s, r = s.cpu().numpy(), r.cpu().numpy()
    want, nz = hostile.known_zero_answer(c, 10, f32_rule=True)
    assert nz == (10 if variant == "a" else 4)
    assert np.array_equal(r, want[:nq])
    assert (s[:, :nz] == 0.0).all() and (s[:, nz:] < 0).all()


# ---- 4. three routes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,nq", [(W8, 256), (W2, 32), (K11, 1), (K11, 8)])
@pytest.mark.parametrize("name,qset", [("aniso", "neg"), ("mixed", "iso")])
def test_screen_forced_fallback_and_exact_scan_agree(rindex, name, qset, form, nq):
    ix = _index(rindex, name)
    _, live = _corpus(name)
    q, q64 = _queries(name, qset, nq)
    ref = _reference((name, qset, "bf16", 768, nq, 10, False), q64, live, 10)
    got = {}
    try:
        for mode in (1, 2, 0):
            ix.enable_screen(mode)
            assert (ix.search_plan(nq, 10) == PLAN[form]) if mode else (ix.search_plan(nq, 10) not in (10, 11))
            ws = torch.empty(ix.workspace_bytes(nq, 10), dtype=torch.uint8, device="cuda")
            s, r = ix.search(q, 10, workspace=ws)
            torch.cuda.synchronize()
            if mode == 2:
                assert ix.screen_valu_diag() if form == K11 else ix.screen_diag(nq, 10, ws)[1]
            elif mode == 1 and form == K11:
                print(f"hostile: three routes {name}/{qset}, {form} nq {nq}: fallback {int(ix.screen_valu_diag())}")
            _verify(s, r, ref, live, q64)
            got[mode] = (s, r)
    finally:
        ix.enable_screen(1)
    assert torch.equal(got[1][1], got[2][1]) and torch.equal(got[1][1], got[0][1])
    assert torch.equal(got[1][0].view(torch.int32), got[2][0].view(torch.int32))


# ---- 5. the natural fallback ----------------------------------------------------------------------------------------
NATURAL_OWN = set()  # forms that answered aniso/neg themselves on the GPU run (none of kernel 10's)
@pytest.mark.parametrize("form,nq", [(W8, 256), (W2, 32), (K11, 1), (K11, 8)])
def test_natural_fallback(rindex, form, nq):
    """aniso with the all-negative queries: the CPU rule keeps up to 95 % of the rows of a query, far more than
    the select holds (2,048 kept candidates) or the lanes' lists keep inside the band, so the batch goes to the
    gated exact pass without mode 2 — and answers with the oracle's rows."""
    ix = _index(rindex, "aniso")
    _, live = _corpus("aniso")
    q, q64 = _queries("aniso", "neg", nq)
    assert ix.search_plan(nq, 10) == PLAN[form]
    ws = torch.empty(ix.workspace_bytes(nq, 10), dtype=torch.uint8, device="cuda")
    s, r = ix.search(q, 10, workspace=ws)
    torch.cuda.synchronize()
    tag = f"aniso/neg natural fallback, {form} nq {nq}"
    if form == K11:
        fb = ix.screen_valu_diag()
        print(f"hostile: {tag}: fallback {int(fb)}")
    else:
        fb = _diag(ix, nq, 10, ws, tag)
    assert fb or (form, nq) in NATURAL_OWN
    _verify(s, r, _reference(("aniso", "neg", "bf16", 768, nq, 10, False), q64, live, 10), live, q64)


# ---- 6. a union of unlike stores --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [256, 1])
def test_union_of_unlike_stores(tmp_path, monkeypatch, nq):
    """One store of `mixed` rows scaled by 2^-12 (tile scales 2^-32 .. 2^-2) and one of plain synthetic unit rows,
    searched as one union view: the view's stats are the maxima over its members, the answer the oracle's over
    the rows side by side (the view's row ids)."""
    from oracle import synth as osynth
    from rfx import retriever as rret
    from rfx import store as rstore
    from rfx.index import synth_rows
    from rfx.retriever import GpuRetriever

    monkeypatch.setenv("RFX_SCREEN", "1")
    reg = rstore.StoreRegistry(root=str(tmp_path), device=0)
    ret = GpuRetriever(registry=reg, dtype="bf16")
    c, _ = _corpus("mixed")
    small = c.rows * np.float32(2.0 ** -12)
    assert np.array_equal(hostile.stored(small, "bf16"), small)  # a power of two: still stored values
    n_b = 20_000
    parts = [small, osynth.to_f64(osynth.synth_rows(71, 0, n_b, 768, "bf16"), "bf16").astype(np.float32)]
    stores = [reg.create("tiny", 768, "bf16"), reg.create("unit", 768, "bf16")]
    stores[0].add_document([f"t{i}" for i in range(small.shape[0])], _dev(small, "bf16"), "tiny.md", {})
    stores[1].add_document([f"u{i}" for i in range(n_b)], synth_rows(71, 0, n_b, 768, "bf16"), "unit.md", {})
    assert all(st._screen_on is True for st in stores)
    names = [st.name for st in stores]
    view = ret._union_view(names, stores)
    try:
        assert view.screened
        member = [st.index.screen_read(0, 1)[3] for st in stores]
        assert np.array_equal(view.index.screen_read(0, 1)[3], np.maximum(member[0], member[1]))
        total = max(view.index.rows, view.bases[-1] + n_b)
        rows64 = np.full((total, 768), np.nan)
        for base, p in zip(view.bases, parts):
            rows64[base:base + p.shape[0]] = p
        q32 = c.queries["iso"][:nq]
        q64 = q32.astype(np.float64)
        k = 10
        assert view.index.search_plan(nq, k) == (10 if nq > 8 else 11)
        s, r = view.index.search(_dev(q32, "bf16"), k)
        torch.cuda.synchronize()
        _verify(s, r, osearch.topk(q64, rows64, k), rows64, q64)
    finally:
        rret._release_union(view)
        for st in stores:
            reg.drop(st.name)
