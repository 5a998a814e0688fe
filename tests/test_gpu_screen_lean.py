"""GPU: kernel 10's lean issue stream (DESIGN §4.10 "Round 8"): the corpus stream's source, ring slot and
tile record advance as running state (csrc/k10_stream.h), the fragment reads take the slot's position from
a running value, and beyond tile 64 of a block the slot table is re-read only every 16th tile.

What can go wrong is in the addressing, so the shapes are small stores cut into few workgroups
(rfx_search_staged's scan_blocks), where a block runs many tiles: past the thinned cadence's start plus
twice its interval (64 + 32 tiles), tile counts that are odd, no multiple of the ring size (10; 8 in the
2-wave kernel) and below it, a block with one tile, and more tiles than a block's share in the tail's
clamped loads.  With 8 or 16 lists per query instead of the plan's 512, a plain synthetic store sends the batch
to the gated exact pass (some list drops a row inside the e2 band), which would hide kernel 10's answer.  So
every store carries kPlant planted rows per query, a_j q + sqrt(1 - a_j^2) r with a_j from 0.90 down to 0.45
(r the synthetic row they replace), at random positions over the whole store: they lie far above every
other row's score (|q . r| < 0.2 for unit vectors at d >= 768, the band 2 E_q is a few hundredths), a list
never holds more than its KL = 10 entries of them inside the band unless 11 of a query's 16 fall into one of
the lists, and every case asserts that the fallback did not run and that each query kept >= k survivors:
what is compared is kernel 10's own answer.  Bars as tests/test_gpu_screen.py: the brute-force top-k of oracle/search.py under check_topk
(rows identical outside the 2e-6 tie band, scores within 1e-5 of the f64 score), and the exact scan's rows
and scores bit for bit (torch.equal)."""
import numpy as np
import pytest
import torch

from oracle import search as osearch
from oracle import synth as osynth

pytestmark = pytest.mark.gpu

TOL, TIE = 1e-5, 2e-6
K = 10


@pytest.fixture(scope="module")
def rindex():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rfx.index as ri
    return ri


kPlant = 16
_store_cache = {}


def _store(rindex, n, d, dtype, nq, seed_q):
    """(rows on the device, the same rows in f64, queries on the device, queries in f64) of a synthetic store
    with kPlant planted rows per query; built once per shape and never written to."""
    key = (n, d, dtype, nq, seed_q)
    if key not in _store_cache:
        rows = rindex.synth_rows(41, 0, n, d, dtype).clone()
        q = rindex.synth_rows(seed_q, 0, nq, d, dtype)
        g = torch.Generator().manual_seed(7)
        # (the two stores of a few tiles keep their plain rows: with 5-6 tiles or one tile per list nothing is
        # dropped inside the band, and there is no room for 16 planted rows per query)
        np_ = kPlant if nq * kPlant * 4 <= n else 0
        pos = torch.randperm(n, generator=g)[:nq * np_].reshape(nq, np_).to(rows.device)
        if np_:
            a = (0.90 - 0.03 * torch.arange(kPlant, dtype=torch.float32, device=rows.device)).reshape(1, kPlant, 1)
            mix = a * q.float().unsqueeze(1) + torch.sqrt(1 - a * a) * rows[pos].float()
            rows[pos] = mix.to(rows.dtype)
        r64 = rows.double().cpu().numpy()
        r64.setflags(write=False)
        _store_cache[key] = (rows, r64, q, q.double().cpu().numpy(), pos.cpu().numpy())
    return _store_cache[key]


def _assert_own_answer(ix, nq, k, ws):
    diag, fb = ix.screen_diag(nq, k, ws)
    print(f"fallback {fb}, survivors min {diag[:, 1].min()} max {diag[:, 1].max()}")
    assert not fb and (diag[:, 1] >= min(k, ix.rows)).all(), (fb, diag[:, 1].min())  # kernel 10's answer, not the fallback's


def _staged(ix, q, k, scan_blocks, row_mask=None):
    """The two-pass search through rfx_search_staged (both stages in one call) with the screen limited to
    scan_blocks workgroups; returns (scores, rows, workspace)."""
    from rfx import _lib
    nq = q.shape[0]
    s = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    r = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    ws = torch.empty(ix.workspace_bytes(nq, k), dtype=torch.uint8, device=q.device)
    m = _lib.ptr(row_mask) if row_mask is not None else None
    mw = row_mask.numel() if row_mask is not None else 0
    _lib.check(_lib.lib.rfx_search_staged(ix.handle, _lib.ptr(q), nq, k, m, mw, 0, _lib.ptr(s), _lib.ptr(r), None,
                                          _lib.ptr(ws), ws.numel(), 3, scan_blocks, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return s, r, ws


def _oracle_check(s, r, rows64, q64, k):
    ref_s, ref_r = osearch.topk(q64, rows64, k)
    probs = osearch.check_topk(s.cpu().numpy(), r.cpu().numpy(), ref_s, ref_r, lambda qi, rr: rows64[rr] @ q64[qi],
                               tol=TOL, tie_band=TIE)
    assert not probs, probs[:5]


def _exact(ix, q, k, row_mask=None):
    """The exact scan on the same index (the screen switched off for the call)."""
    ix.enable_screen(0)
    assert ix.search_plan(q.shape[0], k) not in (10, 11)
    s, r = ix.search(q, k, row_mask=row_mask)
    torch.cuda.synchronize()
    ix.enable_screen(1)
    return s, r


# (dtype, d, rows, nq, scan_blocks) -> tiles per workgroup of the screen:
#   63,000 rows, 8 blocks: 1,969 tiles, XCD-balanced split: 246 and 247 tiles (odd, no multiple of 10), the last
#     tile 24 rows short (the NaN tail); 64 + 11 intervals of the thinned cadence
#   40,000 rows, nq 100: 1,250 tiles: 156 and 157
#   20,000 rows, nq 300: two query groups share the 8 workgroups: 4 blocks, static split: 157, 156, 156, 156
#   1,287 rows, 8 blocks: 41 tiles, static split: 6 and 5 tiles (below the ring size, below AHEAD / NST + 1)
#   300 rows, the plan's own blocks: 10 blocks of one tile
#   30,000 x 1024 f16: 938 tiles: 117 and 118 (four stages per tile)
#   60,000 rows, nq 32: the 2-wave kernel (8-slot ring): 1,875 tiles: 234 and 235
CASES = [("bf16", 768, 63_000, 256, 8), ("bf16", 768, 40_000, 100, 8), ("bf16", 768, 20_000, 300, 8),
         ("bf16", 768, 1_287, 256, 8), ("bf16", 768, 300, 256, 0), ("f16", 1024, 30_000, 256, 8),
         ("bf16", 768, 60_000, 32, 8)]


@pytest.mark.parametrize("dtype,d,n,nq,blocks", CASES)
def test_lean_stream_matches_oracle_and_exact_scan(rindex, dtype, d, n, nq, blocks):
    rows, rows64, q, q64, _ = _store(rindex, n, d, dtype, nq, 42)
    ix = rindex.DeviceIndex(d, dtype)
    ix.add(rows)
    ix.enable_screen(1)
    assert ix.search_plan(nq, K) == 10
    s, r, ws = _staged(ix, q, K, blocks)
    _assert_own_answer(ix, nq, K, ws)
    _oracle_check(s, r, rows64, q64, K)
    # a second launch (the XCD weights have moved: another split of the same tiles) answers the same
    s2, r2, ws2 = _staged(ix, q, K, blocks)
    _assert_own_answer(ix, nq, K, ws2)
    assert torch.equal(r2, r) and torch.equal(s2, s)
    se, re_ = _exact(ix, q, K)
    assert torch.equal(r, re_) and torch.equal(s, se)
    ix.close()


@pytest.mark.parametrize("nq", [256, 32])
def test_lean_stream_row_states(rindex, nq):
    """Tombstoned rows, appended rows (the last tile re-quantised), the NaN tail of the last tile and a row
    mask (the MASK = true kernels), in blocks of 156 / 157 tiles.  The mask admits 30 % of the rows and every
    planted row but each query's best and fourth; the tombstones take each query's second planted row and
    rows at tile and block edges: 13 planted rows per query stay, so kernel 10 still proves its answer."""
    n0, n1 = 37_000, 3_011
    n = n0 + n1
    rows, rows64, q, q64, pos = _store(rindex, n, 768, "bf16", nq, 43)
    ix = rindex.DeviceIndex(768, "bf16")
    ix.add(rows[:n0].contiguous())
    ix.enable_screen(1)
    ix.add(rows[n0:].contiguous())
    planted = set(pos.ravel().tolist())
    dead = sorted(set(pos[:, 1].tolist()) | {e for e in (0, 31, 32, 5_000, 20_017, n0 - 1, n0, n - 1) if e not in planted})
    ix.tombstone(dead)
    live64 = rows64.copy()
    live64[dead] = np.nan
    rng = np.random.default_rng(5)
    allowed = rng.random(n) < 0.3
    allowed[pos.ravel()] = True
    allowed[pos[:, 0]] = False
    allowed[pos[:, 3]] = False
    words = np.zeros((n + 31) // 32, dtype=np.uint32)
    idx = np.nonzero(allowed)[0]
    np.bitwise_or.at(words, idx >> 5, (np.uint64(1) << (idx & 31).astype(np.uint64)).astype(np.uint32))
    m = torch.from_numpy(words.view(np.int32)).cuda()
    masked = live64.copy()
    masked[~allowed] = np.nan
    for mask, ref in ((m, masked), (None, live64)):
        s, r, ws = _staged(ix, q, K, 8, row_mask=mask)
        _assert_own_answer(ix, nq, K, ws)
        _oracle_check(s, r, ref, q64, K)
        se, re_ = _exact(ix, q, K, row_mask=mask)
        assert torch.equal(r, re_) and torch.equal(s, se)
    ix.close()
