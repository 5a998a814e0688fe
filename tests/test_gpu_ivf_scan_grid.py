"""Every instantiation of the IVF list scan (csrc/k_ivf_scan.hip: list_scan_kernel<K, NC, policy>) run once and held
BIT-EXACT (rows equal, scores equal as int32) to the numpy reference of the neighbouring tests, oracle/ivf.py
through tests/ivf_mask_ref.py / tests/ivf_multi_ref.py: d 256, 512, 768, 1024 x the three list_k slots k 4, 16, 64 x
the three eligibility policies (no mask, one row_mask, row_masks / mask_of).  tests/test_gpu_ivf_masked.py and
tests/test_gpu_ivf_multi.py go deep at d 256 and 768 only.

The smallest corpus at which the scan can still go wrong: hostile_ivf.planted lists of 0, 1, 65 and 700 rows (no
pairs' rows / a single lane / a second chunk with one valid lane / at one split wave 0 takes the 64-row groups 0, 4
and 8: past kSeedChunks = 2, into offer()).  Nine questions probe every list, so each list's pairs are one full
staged batch of 8 and a batch of 1.  The masks are `sparse` (rows r % 16 == 0: 48 of the 766 rows, so k 4 and 16
are filled and k 64 ends in padding, -inf and row -1, which the comparison includes) and its complement; the
per-question case gives the questions sparse, ~sparse and no mask in turn, so any 8 of a list's 9 pairs hold all
three in one staged batch.  766 % 32 != 0 and the spare bits of the last mask word are set."""
import numpy as np
import pytest
import torch

import hostile_ivf as hi
import ivf_mask_ref as mr
import ivf_multi_ref as mu
from oracle import ivf as oivf

SIZES = [0, 1, 65, 700]
NQ = 9
MASK_OF = np.array([0, 1, -1] * 3, dtype=np.int32)
POLICIES = ("none", "one_mask", "per_question")

_corpora, _indexes = {}, {}


def corpus(d):
    """(IvfCorpus, the two selections) at dimension d, built once."""
    if d not in _corpora:
        rows, lab, qc, rng = hi.planted(d, SIZES, "bf16", seed=31)
        q = hi.queries(rng, len(SIZES), d, NQ, "bf16", SIZES)
        rows.setflags(write=False)
        c = hi.IvfCorpus(f"grid{d}", "bf16", rows, qc, {"law": q}, {"labels": lab, "sizes": SIZES})
        sparse = np.arange(len(lab)) % 16 == 0
        _corpora[d] = (c, [sparse, ~sparse])
    return _corpora[d]


def selections(d, policy):
    """One bool [n] per question."""
    c, sels = corpus(d)
    ones = np.ones(c.rows.shape[0], dtype=bool)
    if policy == "none":
        return [ones] * NQ
    if policy == "one_mask":
        return [sels[0]] * NQ
    return [ones if m < 0 else sels[m] for m in MASK_OF]


def reference(d, k, policy):
    c, _ = corpus(d)
    codes, inv, lab, fc = c.quantized()
    qq, qinv = oivf.quantize(c.queries["law"])
    return mu.search(qq, qinv, codes, inv, lab, c.qc, fc, [len(SIZES)] * NQ, k, selections(d, policy))


def test_reference_fills_k_4_and_16_and_pads_k_64():
    """No GPU: what the grid relies on, from the reference alone."""
    assert sum(SIZES) % 32, "the last mask word must have spare bits"
    for policy in POLICIES:
        elig = [int(s.sum()) for s in selections(256, policy)]
        assert min(elig) >= 16
        for k in (4, 16, 64):
            ref_s, ref_r = reference(256, k, policy)
            for i in range(NQ):  # every list is probed: min(k, eligible rows) come back, padding behind
                n = min(k, elig[i])
                assert (ref_r[i, :n] >= 0).all() and (ref_r[i, n:] == -1).all() and np.isneginf(ref_s[i, n:]).all()
    assert min(int(s.sum()) for s in selections(256, "per_question")) == 48  # k 64 is padded where a mask is sparse


@pytest.fixture(scope="module")
def rivf():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rfx.ivf as rivf
    yield rivf
    for ix, _ in _indexes.values():
        ix.close()
    _indexes.clear()


def up(x):
    t = torch.from_numpy(np.array(x, dtype=np.float32)).to(torch.bfloat16)
    assert np.array_equal(t.to(torch.float32).numpy(), x)
    return t.cuda()


def index_of(rivf, d):
    """(index, the two device masks with the spare bits set) at dimension d, built once."""
    if d not in _indexes:
        c, sels = corpus(d)
        ix = rivf.IvfIndex(d, c.nlist)
        ix.set_centroids(torch.from_numpy(c.qc).cuda())
        ix.add(up(c.rows))
        _indexes[d] = (ix, [torch.from_numpy(mr.to_words(s)).cuda() for s in sels])
    return _indexes[d]


@pytest.mark.gpu
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("k", [4, 16, 64])
@pytest.mark.parametrize("d", [256, 512, 768, 1024])
def test_scan_grid(rivf, monkeypatch, d, k, policy):
    c, _ = corpus(d)
    ix, masks = index_of(rivf, d)
    q = up(c.queries["law"])
    monkeypatch.setenv("RFX_IVF_SPLITS", "1")
    if policy == "none":
        s, r = ix.search(q, k, c.nlist)
    elif policy == "one_mask":
        s, r = ix.search(q, k, c.nlist, row_mask=masks[0])
    else:
        s, r = ix.search(q, k, None, row_masks=masks, mask_of=MASK_OF, nprobes=[c.nlist] * NQ)
    ref_s, ref_r = reference(d, k, policy)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    assert np.array_equal(r, ref_r), f"rows differ in queries {np.flatnonzero((r != ref_r).any(axis=1)).tolist()}"
    assert np.array_equal(s.view(np.int32), ref_s.view(np.int32)), "scores differ"
