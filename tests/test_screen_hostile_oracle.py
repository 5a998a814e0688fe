"""CPU: the two-pass rule (oracle/screen.py) on the hostile corpora of tests/hostile.py returns exactly the
brute-force top-k of oracle/search.py — tile scales 2^-20 .. 2^10 apart, live all-zero tiles, negative k-th
scores and bounds, rint ties, thousands of survivors.  This keeps the reference honest: a mismatch in
tests/test_gpu_screen_hostile.py is then the kernels', not the rule's.  Each case prints the survivors per
query (min / mean / max), the numbers DESIGN §4.10 quotes."""
import numpy as np
import pytest

import hostile
from oracle import screen as oscreen
from oracle import search as osearch

N, D, NQ = 4113, 768, 16  # 129 tiles, the last one ragged

CASES = [("aniso", "same"), ("aniso", "neg"), ("shifted", "lean"), ("mixed", "iso"), ("mixed_small", "iso"),
         ("zeros_a", "lean"), ("zeros_b", "lean"), ("zeros_c", "lean"), ("zeros_d", "lean")]
_built = {}


def _corpus(name, dtype="bf16", d=D):
    key = (name, dtype, d)
    if key not in _built:
        if name == "aniso":
            c = hostile.aniso(N, d, dtype, NQ)
        elif name == "shifted":
            c = hostile.shifted(N, d, dtype, NQ)
        elif name == "mixed":
            c = hostile.mixed(N, d, dtype, NQ)
        elif name == "mixed_small":  # the small-scale tiles alone: the tiles of 2^0 and above, the tie tile (row norm
            c = hostile.mixed(N, d, dtype, NQ)  # 16) and the one-hot row (norm 1) tombstoned: Xmax is 2^-1
            big = np.nonzero(np.repeat(c.notes["exponents"] >= 0, hostile.TM)[:N])[0]
            c.dead = sorted(set(big.tolist()) | set(range(c.notes["tie_tile"] * 32, c.notes["tie_tile"] * 32 + 32))
                            | {c.notes["onehot_row"]})
        else:
            c = hostile.zeros(N, d, dtype, NQ, name[-1])
        c.rows.setflags(write=False)
        _built[key] = c
    return _built[key]


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("name,qset", CASES)
def test_screen_rule_equals_brute_force(name, qset, k):
    c = _corpus(name)
    x, y = hostile.live_rows(c), c.queries[qset]
    s, r, nsv = oscreen.screen_topk(y, x, k)
    rs, rr = osearch.topk(y.astype(np.float64), x.astype(np.float64), k)
    print(f"{name}/{qset} k {k}: survivors min {nsv.min()} mean {nsv.mean():.0f} max {nsv.max()} of "
          f"{int((~np.isnan(x).any(axis=1)).sum())} live rows")
    assert np.array_equal(r, rr)
    assert np.allclose(s, rs, atol=1e-12 * hostile.scale_bound(x, y), rtol=0)
    assert (nsv >= k).all()


@pytest.mark.parametrize("dtype,d", [("f16", 1024), ("f32", 768)])
@pytest.mark.parametrize("name", ["mixed", "zeros_a", "zeros_b"])
def test_screen_rule_other_types(name, dtype, d):
    c = _corpus(name, dtype, d)
    x, y = hostile.live_rows(c), next(iter(c.queries.values()))
    s, r, nsv = oscreen.screen_topk(y, x, 10)
    rs, rr = osearch.topk(y.astype(np.float64), x.astype(np.float64), 10)
    print(f"{name} {dtype} d {d}: survivors min {nsv.min()} mean {nsv.mean():.0f} max {nsv.max()}")
    assert np.array_equal(r, rr)


def test_builders_plant_what_they_promise():
    c = _corpus("mixed")
    codes, scales, live, stats = oscreen.quantize_tiles(c.rows)
    nt = scales.size
    for t in c.notes["zero_tiles"]:
        assert scales[t] == 0 and live[t] == 0xFFFFFFFF and not codes[t * 32:(t + 1) * 32].any()
    t = c.notes["onehot_tile"]
    blk = codes[t * 32:(t + 1) * 32]
    assert blk.min() == -127 and np.count_nonzero(blk) == 1 and scales[t] == np.float32(1 / 127)
    t = c.notes["tie_tile"]
    blk = codes[t * 32:(t + 1) * 32].astype(np.int64)
    assert scales[t] == np.float32(2.0 ** -7) and blk.max() == 127 and blk.min() == -126
    # every tie went to the even neighbour: no odd code but the amax's 127
    assert (blk[blk != 127] % 2 == 0).all() and set(np.abs(blk[blk != 127]).tolist()) == set(range(0, 127, 2))
    pos = scales[scales > 0]
    assert pos.max() / pos.min() > 2.0 ** 28 and nt == 129
    # zeros: the answer is known outright and the oracle agrees with it
    for v in ("zeros_a", "zeros_b"):
        z = _corpus(v)
        want, nz = hostile.known_zero_answer(z, 10)
        rs, rr = osearch.topk(z.queries["lean"].astype(np.float64), hostile.live_rows(z).astype(np.float64), 10)
        assert np.array_equal(rr, want) and (rs[:, :nz] == 0.0).all() and (rs[:, nz:] < 0).all()
        assert nz == (10 if v == "zeros_a" else 4)
