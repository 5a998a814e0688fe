"""One list search for a batch under different filters against one list search per filter group, at
the config-5 per-GPU shard shape (12.5M x 768 bf16, nlist 4096, nprobe 32) or any smaller one.

The corpus is built as tools/bench_ivf_filtered.py builds it (an IvfIndex and a DeviceIndex over the same clustered
synthetic rows).  The two paths are LocalStore's own methods — search_lists_filtered_multi (one search) and
search_lists_filtered once per group (the per-group loop of RFX_IVF_MULTI=0) — bound to a stand-in that supplies
what they read of a store (lock, ivf, index, spec, the row counts, mask_ranges, row_mask): the lock, the rule, the
mask cache and the device-to-host copies are the store's code, the files are not written.  Filters: G groups, group
g selecting every second "file" of 1,000 (f = 1/2, probe count doubled) when g is odd and all of them (f = 1) when g
is even, from offset g, so the masks differ and so do the probe counts.  Per (G, questions per group): median ms per
call over --rounds interleaved rounds of --steps calls, wall clock around calls that end with their host copies.
G = 1 is the batch of one tenant: there the "loop" is the one one-mask search the retriever keeps for it, and the
line prices the per-question entry point against it.

The kernel alone: IvfIndex.search with one mask in the table against the one-mask form (row_mask=), and with 8
identical masks under 8 table indices, one per question of each staged batch (what a scan that reloads its mask
word for every staged question would pay).  Nothing is asserted: the numbers go into DESIGN as measured.

Usage: python tools/bench_ivf_multifilter.py [--rows R] [--nlist L] [--nprobe P] [--k K] [--steps S] [--rounds N]
       python tools/bench_ivf_multifilter.py --rows 400000 --nlist 512 --nprobe 8 --centres 2048   (a quick run)
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rag-foundation_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rfx import filters  # noqa: E402
from rfx.index import DeviceIndex  # noqa: E402
from rfx.ivf import IvfIndex, synth_clustered  # noqa: E402
from rfx.store import LocalStore  # noqa: E402

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
ap.add_argument("--groups", type=int, nargs="+", default=[1, 2, 8, 32])
ap.add_argument("--per-group", type=int, nargs="+", default=[1, 8])
a = ap.parse_args()

assert torch.cuda.is_available(), "bench_ivf_multifilter needs a GPU"
torch.cuda.set_device(0)
os.environ["RFX_IVF_FILTERED"] = "1"
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
bounds = np.linspace(0, a.rows, a.files + 1).astype(np.int64)


class StoreView:
    """What LocalStore.search_lists_filtered / _multi / filtered_nprobe read of a store; a filter is {"g": g}."""
    lock = threading.RLock()
    ivf, index = ix, bf
    spec = {"kind": "ivf", "nlist": a.nlist, "nprobe": a.nprobe}
    rows = range(a.rows)
    _masks = {}
    ivf_ready = staticmethod(lambda: True)
    dead_rows = staticmethod(lambda: 0)
    filtered_nprobe = LocalStore.filtered_nprobe
    search_lists_filtered = LocalStore.search_lists_filtered
    search_lists_filtered_multi = LocalStore.search_lists_filtered_multi

    _ranges = {}

    def mask_ranges(self, filt):  # cached per filter, as LocalStore caches them
        g = filt["g"]
        if g not in self._ranges:
            step = 2 if g % 2 else 1
            self._ranges[g] = [(int(bounds[i]), int(bounds[i + 1] - bounds[i]))
                               for i in range((g // 2) % step, a.files, step)]
        return self._ranges[g]

    def row_mask(self, filt):
        if filt["g"] not in self._masks:
            words = filters.row_mask_words(a.rows, self.mask_ranges(filt)).copy()
            words[(filt["g"] * 7919) % len(words)] ^= 1 << 5  # no two groups' masks are equal
            self._masks[filt["g"]] = bf.mask_tensor(words)
        return self._masks[filt["g"]]


st = StoreView()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / a.steps, out


for G in a.groups:
    for per in a.per_group:
        nq = G * per
        q = synth_clustered(CSEED, a.centres, QSEED, 0, nq, a.dim, "bf16")
        filts = [{"g": i // per} for i in range(nq)]
        qs = [q[g * per:(g + 1) * per].contiguous() for g in range(G)]

        def one():
            return st.search_lists_filtered_multi(q, a.k, filts)

        def loop():
            return [st.search_lists_filtered(qs[g], a.k, {"g": g}) for g in range(G)]

        for _ in range(2):
            m, lp = one(), loop()
        assert m[2] == [] and torch.equal(m[1], torch.cat([r for _, r in lp])), "the two paths disagree"
        t1, tl = [], []
        for _ in range(a.rounds):
            t1.append(timed(one)[0])
            tl.append(timed(loop)[0])
        m1, ml = statistics.median(t1), statistics.median(tl)
        print(json.dumps({"groups": G, "per_group": per, "nq": nq,
                          "nprobes": sorted({st.filtered_nprobe({"g": g}) for g in range(G)}),
                          "one_search_ms": round(m1, 4), "one_min_max": [round(min(t1), 4), round(max(t1), 4)],
                          "per_group_loop_ms": round(ml, 4), "loop_min_max": [round(min(tl), 4), round(max(tl), 4)],
                          "loop_over_one": round(ml / m1, 2)}), flush=True)

# the kernel form alone: one mask through the table against the one-mask form; 8 indices per staged batch
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def dev_timed(fn):
    e0.record()
    for _ in range(a.steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.steps


mask = st.row_mask({"g": 1})
copies = [mask.clone() for _ in range(8)]
for nq in (8, 256):
    q = synth_clustered(CSEED, a.centres, QSEED, 0, nq, a.dim, "bf16")
    ws = torch.empty(ix.workspace_bytes(nq, 16, a.nprobe), dtype=torch.uint8, device="cuda")
    forms = {
        "one_mask_form": lambda: ix.search(q, 16, a.nprobe, workspace=ws, row_mask=mask),
        "table_of_1": lambda: ix.search(q, 16, a.nprobe, workspace=ws, row_masks=[mask]),
        "table_of_8_grouped": lambda: ix.search(q, 16, a.nprobe, workspace=ws, row_masks=copies,
                                                mask_of=[i * 8 // nq for i in range(nq)]),
        "table_of_8_interleaved": lambda: ix.search(q, 16, a.nprobe, workspace=ws, row_masks=copies,
                                                    mask_of=[i % 8 for i in range(nq)]),
    }
    for f in forms.values():
        f(), f()
    t = {n: [] for n in forms}
    for _ in range(a.rounds):
        for n, f in forms.items():
            t[n].append(dev_timed(f))
    print(json.dumps({"kernel_forms_nq": nq, "nprobe": a.nprobe,
                      **{n: round(statistics.median(v), 4) for n, v in t.items()}}), flush=True)
bf.close()
ix.close()
