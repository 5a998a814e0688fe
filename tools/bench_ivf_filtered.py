"""Metadata-filtered IVF search against the exact masked scan, at the config-5 per-GPU shard shape
(BASELINE.json configs[4]: 12.5M x 768 bf16, nlist 4096, nprobe 32) or any smaller one.

One store's worth of state is built once, as tools/bench_ivf.py builds it: the clustered synthetic corpus in an
IvfIndex (int8 lists) and in a DeviceIndex (the bf16 rows, which the exact scan reads and the re-rank reads in
place).  A filter is a set of contiguous row ranges as files make them: the rows are cut into --files equal
"files" and every (1/f)-th is selected, f = 1, 1/2, 1/4, 1/8.  For every (f, nq in 1, 8, 256) the two searches a
filtered question can take run in the same process on the same mask, interleaved round by round:

  ivf    IvfIndex.search_index(row_mask=mask) at the widened probe count ivf_filter_nprobe(.., mode "1")
         (min(ceil(nprobe / f), 64); the line says when RFX_IVF_FILTERED=auto would have kept the exact path),
         exact re-rank of min(64, max(16, 2k)) candidates;
  exact  DeviceIndex.search(row_mask=mask).

Per line: median ms per call of each over the rounds (device events around --steps calls), their ratio, and
recall@k of the former against the latter; ivf_nomask_ms is the same IVF call without the mask (the same probes
and lists, another answer): what the mask lookup in the list scan costs.  Nothing is asserted: the numbers go
into DESIGN as measured.

Usage: python tools/bench_ivf_filtered.py [--rows R] [--nlist L] [--nprobe P] [--k K] [--steps S] [--rounds N]
       python tools/bench_ivf_filtered.py --rows 400000 --nlist 512 --nprobe 8 --centres 2048   (a quick run)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rag-foundation_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rfx import filters  # noqa: E402
from rfx.index import DeviceIndex  # noqa: E402
from rfx.ivf import IvfIndex, synth_clustered  # noqa: E402
from rfx.store import ivf_filter_nprobe  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=12_500_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--nlist", type=int, default=4096)
ap.add_argument("--nprobe", type=int, default=32)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--files", type=int, default=1000)
ap.add_argument("--centres", type=int, default=16384)
ap.add_argument("--train-rows", type=int, default=262_144)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--nq", type=int, nargs="+", default=[1, 8, 256])
ap.add_argument("--inv-f", type=int, nargs="+", default=[1, 2, 4, 8])
a = ap.parse_args()

assert torch.cuda.is_available(), "bench_ivf_filtered needs a GPU"
torch.cuda.set_device(0)
CSEED, SEED, QSEED, CHUNK = 1234, 1, 2, 1 << 20

ix = IvfIndex(a.dim, a.nlist)
ix.train(synth_clustered(CSEED, a.centres, SEED, 0, min(a.train_rows, a.rows), a.dim, "bf16"), iters=a.iters)
bf = DeviceIndex(a.dim, "bf16", capacity=a.rows)
for r0 in range(0, a.rows, CHUNK):
    x = synth_clustered(CSEED, a.centres, SEED, r0, min(CHUNK, a.rows - r0), a.dim, "bf16")
    ix.add(x)
    bf.add(x)
del x
ix.build()
torch.cuda.synchronize()
print(json.dumps({"rows": a.rows, "dim": a.dim, "nlist": a.nlist, "nprobe": a.nprobe, "k": a.k, "files": a.files,
                  "steps": a.steps, "rounds": a.rounds}), flush=True)

rk = min(64, max(16, 2 * a.k))
bounds = np.linspace(0, a.rows, a.files + 1).astype(np.int64)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn):
    e0.record()
    for _ in range(a.steps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.steps, out


for inv_f in a.inv_f:
    ranges = [(int(bounds[i]), int(bounds[i + 1] - bounds[i])) for i in range(0, a.files, inv_f)]
    selected = sum(n for _, n in ranges)
    mask = bf.mask_tensor(filters.row_mask_words(a.rows, ranges))
    nprobe = ivf_filter_nprobe(a.nprobe, a.nlist, selected, a.rows, "1")
    auto = ivf_filter_nprobe(a.nprobe, a.nlist, selected, a.rows, "auto")
    for nq in a.nq:
        q = synth_clustered(CSEED, a.centres, QSEED, 0, nq, a.dim, "bf16")
        ivf = lambda: ix.search_index(q, a.k, nprobe, bf, rerank_k=rk, row_mask=mask)
        exact = lambda: bf.search(q, a.k, row_mask=mask)
        nomask = lambda: ix.search_index(q, a.k, nprobe, bf, rerank_k=rk)
        for _ in range(2):  # warm every shape
            ivf(), exact(), nomask()
        torch.cuda.synchronize()
        ti, te, tn = [], [], []
        for _ in range(a.rounds):  # interleaved: one window of each per round
            ms, (_, ri) = timed(ivf)
            ti.append(ms)
            ms, (_, re) = timed(exact)
            te.append(ms)
            tn.append(timed(nomask)[0])
        ri, re = ri.cpu().tolist(), re.cpu().tolist()
        sel = np.zeros(a.rows, dtype=bool)
        for lo, n in ranges:
            sel[lo:lo + n] = True
        flat = np.array(ri)
        assert sel[flat[flat >= 0]].all(), "the filtered IVF search returned an unselected row"
        hit = sum(len(set(x) & set(y)) for x, y in zip(ri, re))
        want = sum(len([r for r in y if r >= 0]) for y in re)
        mi, me = statistics.median(ti), statistics.median(te)
        print(json.dumps({"f": f"1/{inv_f}", "selected": selected, "nq": nq, "nprobe": nprobe,
                          "auto_path": "ivf" if auto is not None else "exact",
                          "ivf_ms": round(mi, 4), "ivf_ms_min_max": [round(min(ti), 4), round(max(ti), 4)],
                          "ivf_nomask_ms": round(statistics.median(tn), 4), "exact_ms": round(me, 4),
                          "exact_ms_min_max": [round(min(te), 4), round(max(te), 4)],
                          "exact_over_ivf": round(me / mi, 2), "recall_at_k": round(hit / max(want, 1), 4)}), flush=True)
bf.close()
ix.close()
