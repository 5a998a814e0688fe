"""GPU: the wide form of the two-pass scan (plan 12): batches of 9 or more questions at
top_k 11..64 — what the retriever's fetch_k = min(64, max(4k, 16)) searches are — screened by kernel 10 with
lists of 16 and the bound of k_scan_screen.h "the wide form", selected at k <= 64, with the exact plan of the same
search (kernels 1 / 2 / 3 at k <= 16, the VALU scan above) as the gated exact pass.

Bars as tests/test_gpu_screen_w2.py: the brute-force top-k of oracle/search.py under check_topk (rows identical
outside the 2e-6 tie band, scores within 1e-5 of the f64 score); screen, forced fallback and exact search the
same bits."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import search as osearch
from test_gpu_screen_w2 import _check, _make, _queries, rindex  # noqa: F401  (the idiom, and its fixture)

pytestmark = pytest.mark.gpu


# both kernel forms (2 waves up to 64 questions, 8 waves above at d 768; d 1024: 2 waves per 64 questions), the
# list-length edge 16 / 17 (the own-list term and m = 1 end at 16), every m = ceil(k / 16) in 1..4, k 64
@pytest.mark.parametrize("dtype,d,n,nq,k", [
    ("bf16", 768, 60_000, 9, 11), ("bf16", 768, 60_000, 33, 16), ("bf16", 768, 60_000, 64, 17),
    ("bf16", 768, 60_000, 65, 40), ("bf16", 768, 60_000, 300, 64), ("bf16", 768, 60_000, 100, 63),
    ("f16", 1024, 30_000, 33, 40), ("f16", 1024, 30_000, 100, 17), ("f16", 1024, 30_000, 64, 64),
    ("f32", 768, 40_000, 9, 64), ("f32", 768, 40_000, 65, 16), ("f32", 768, 40_000, 300, 40)])
def test_wide_plan_and_oracle(rindex, dtype, d, n, nq, k):
    ix, rows32 = _make(rindex, n, d, dtype)
    assert ix.search_plan(nq, k) == 12, ix.search_plan(nq, k)
    q, q32 = _queries(rindex, nq, d, dtype)
    ws = torch.empty(ix.workspace_bytes(nq, k), dtype=torch.uint8, device="cuda")
    _check(ix, rows32, q, q32, k, workspace=ws)
    diag, fb = ix.screen_diag(nq, k, ws)
    print("kept / survivors per query:", diag[:, 0].mean(), diag[:, 1].mean())
    assert not fb and (diag[:, 1] >= min(k, n)).all(), (fb, diag[:, 1].min())  # the screen itself answered
    ix.close()


_CHILD = """
import sys, torch, numpy as np
sys.path[:0] = {path!r}
import rfx.index as ri
ix = ri.DeviceIndex(768, "bf16"); ix.add_synthetic(21, 40000); ix.enable_screen(1)
assert ix.search_plan({nq}, {k}) != 12, ix.search_plan({nq}, {k})
s, r = ix.search(ri.synth_rows(22, 0, {nq}, 768, "bf16"), {k}); torch.cuda.synchronize()
np.save(sys.argv[1], np.concatenate([s.cpu().numpy().view(np.int32).astype(np.int64), r.cpu().numpy()]))
"""


@pytest.mark.parametrize("nq,k", [(32, 40), (100, 40), (32, 16), (100, 16)])  # k 16: kernels 1 / 3 as the gated pass
def test_wide_one_score_rule(rindex, nq, k, tmp_path):
    """Screen (mode 1), forced fallback (mode 2), exact search (mode 0) and the parent's plan (RFX_SCREEN_WIDE=0 in
    a fresh process): the same rows and the same score bits."""
    ix, rows32 = _make(rindex, 40_000, 768, "bf16")
    q, q32 = _queries(rindex, nq, 768, "bf16")
    ws = torch.empty(ix.workspace_bytes(nq, k), dtype=torch.uint8, device="cuda")
    s1, r1 = _check(ix, rows32, q, q32, k, workspace=ws)
    assert ix.search_plan(nq, k) == 12 and not ix.screen_diag(nq, k, ws)[1]
    ix.enable_screen(2)
    s2, r2 = _check(ix, rows32, q, q32, k, workspace=ws)
    assert ix.search_plan(nq, k) == 12 and ix.screen_diag(nq, k, ws)[1]
    ix.enable_screen(0)
    assert ix.search_plan(nq, k) != 12
    s3, r3 = _check(ix, rows32, q, q32, k)
    ix.close()
    out = str(tmp_path / "off.npy")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", _CHILD.format(path=[os.path.join(root, "rag-foundation_amd")], nq=nq, k=k), out], check=True,
                   env=dict(os.environ, RFX_SCREEN_WIDE="0"))
    off = np.load(out)
    for s, r in ((s2, r2), (s3, r3), (off[:nq].astype(np.int32).view(np.float32), off[nq:])):
        assert np.array_equal(r1, r) and np.array_equal(s1.view(np.uint32), s.view(np.uint32))


@pytest.mark.parametrize("case", ["duplicates", "duplicates_overflow", "mask_below_k", "tombstones", "k_above_live"])
def test_wide_hostile(rindex, case):
    n, nq, k = 30_000, 24, 40
    ix, rows32 = _make(rindex, n, 768, "bf16", screen=0)
    q, q32 = _queries(rindex, nq, 768, "bf16")
    ref_r = osearch.topk(q32.astype(np.float64), rows32.astype(np.float64), 64)[1]
    row_mask = allowed = None
    if case.startswith("duplicates"):
        # copies of one query's best row appended: ties by row.  A lane's list takes 16 rows of a tile and
        # consecutive tiles go to different workgroups, so 80 adjacent copies fit the lists of 16 and the screen
        # answers; 4,000 span more tiles than there are workgroups, lists overflow: the natural fallback
        copies = 80 if case == "duplicates" else 4000
        top = int(ref_r[0, 0])
        first = ix.add(ix.read(top, 1).repeat(copies, 1))
        rows32 = np.concatenate([rows32, np.repeat(rows32[top:top + 1], copies, axis=0)])
    elif case == "mask_below_k":  # 30 live rows under the mask, 20 of them query 0's best
        allowed = np.zeros(n, dtype=bool)
        allowed[ref_r[0, :20]] = True
        allowed[1000:1010] = True
        row_mask = torch.from_numpy(np.packbits(np.pad(allowed, (0, -n % 32)), bitorder="little").view(np.int32)).cuda()
    elif case == "tombstones":  # inside the top 64 of several queries
        dead = sorted(set(ref_r[:6, ::3].ravel().tolist()))
        ix.tombstone(dead)
        rows32[dead] = np.nan
    else:  # all but 25 rows dead
        dead = np.setdiff1d(np.arange(n), np.concatenate([ref_r[1, :20], np.arange(5)]))
        ix.tombstone(dead)
        rows32[dead] = np.nan
    ix.enable_screen(1)
    assert ix.search_plan(nq, k) == 12
    ws = torch.empty(ix.workspace_bytes(nq, k), dtype=torch.uint8, device="cuda")
    s, r = _check(ix, rows32, q, q32, k, row_mask=row_mask, allowed=allowed, workspace=ws)
    if case.startswith("duplicates"):
        assert r[0, 0] == top and list(r[0, 1:]) == list(range(first, first + k - 1))
        diag, fb = ix.screen_diag(nq, k, ws)
        print(case, "fallback:", fb, "query 0 kept / survivors:", diag[0])
        if case == "duplicates_overflow":
            assert fb and diag[0, 1] == -1  # the diagnostic says the fallback answered, and for which query
    ix.close()


def test_wide_two_logical_shards_equal_unsharded(rindex):
    """The records path with a row offset: two logical shards at k 40, nq 16 against the whole store."""
    from rfx.sharded import ShardedIndex
    n = 80_000
    whole, _ = _make(rindex, n, 768, "bf16", seed=61)
    sh = ShardedIndex(768, "bf16", [0, 0])
    cuts = sh._cuts(n)
    for i, s in enumerate(sh.shards):
        s.add_synthetic(61, cuts[i + 1] - cuts[i], gen_row0=cuts[i])
        sh.bases[i] = cuts[i]
    sh._split = True
    sh.enable_screen(1)
    q, _ = _queries(rindex, 16, 768, "bf16", seed=62)
    assert all(s.search_plan(16, 40) == 12 for s in sh.shards) and whole.search_plan(16, 40) == 12
    a, b = whole.search(q, 40), sh.search(q, 40)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    whole.close()
    sh.close()


def test_wide_serves_the_diversified_batch(rindex):
    """One consumer: 12 questions at k 10 with MMR fetch 40 candidates each (plan 12) — the same answer as with
    the screen off."""
    ix, _ = _make(rindex, 40_000, 768, "bf16")
    q, _ = _queries(rindex, 12, 768, "bf16")
    assert ix.search_plan(12, 40) == 12
    on = ix.search_mmr(q, 10, 40)
    ix.enable_screen(0)
    off = ix.search_mmr(q, 10, 40)
    assert all(torch.equal(a, b) for a, b in zip(on, off))
    ix.close()
