#!/usr/bin/env python3
"""Batches of 9+ questions at top_k 11..64: the wide form of the two-pass scan (plan 12) against the
plan the same search has without it, alternating inside one process on one GPU.

For each (rows, dtype, nq, k) cell the two paths are timed in turn, `--repeats` rounds (default 7) of `--iters`
searches each between two events; the median per search and the spread (min, max) of the rounds are reported,
every timed path's answer is compared with the exact one (rows and score bits), and the wide path's kept
candidates / survivors per query and its fallback flag are read back.  One JSON line per cell.

    python tools/bench_topk_batch.py --rows 1000000 --dtype bf16 --nq 16,32,64,256 --k 16,17,40,64

RFX_SCREEN_WIDE=2 in the environment plans the wide form also in the cells the plan leaves to the exact plans (how
those cells were measured); --forced-fallback times a batch that takes the fallback.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rag-foundation_amd"))

import torch  # noqa: E402

import rfx.index as ri  # noqa: E402


def timed(ix, q, k, ws, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        ix.search(q, k, workspace=ws)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us per search


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--nq", default="16,32,64,256")
    ap.add_argument("--k", default="16,17,40,64")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--forced-fallback", action="store_true",
                    help="screen mode 2: every batch through the gated exact pass (the cost of a fallback)")
    a = ap.parse_args()
    # two copies of the store: one without the int8 copy (the plan these searches had before the wide form), one
    # with it; nothing is rebuilt between the timed rounds
    ixs = {}
    for mode in (0, 1):
        ixs[mode] = ri.DeviceIndex(a.dim, a.dtype)
        ixs[mode].add_synthetic(7, a.rows)
    ixs[1].enable_screen(2 if a.forced_fallback else 1)
    torch.cuda.synchronize()
    for nq in (int(x) for x in a.nq.split(",")):
        q = ri.synth_rows(8, 0, nq, a.dim, a.dtype)
        for k in (int(x) for x in a.k.split(",")):
            t = {0: [], 1: []}
            ans, plans, diag = {}, {}, None
            for rnd in range(a.repeats + 1):  # round 0 warms both paths up and is dropped
                for mode in (0, 1):
                    ix = ixs[mode]
                    plans[mode] = ix.search_plan(nq, k)
                    ws = torch.empty(ix.workspace_bytes(nq, k), dtype=torch.uint8, device="cuda")
                    s, r = ix.search(q, k, workspace=ws)
                    torch.cuda.synchronize()
                    ans[mode] = (s.clone(), r.clone())
                    us = timed(ix, q, k, ws, a.iters)
                    if rnd:
                        t[mode].append(us)
                    if mode == 1 and plans[1] == 12:
                        d, fb = ix.screen_diag(nq, k, ws)
                        diag = {"kept": float(d[:, 0].mean()), "survivors": float(d[:, 1].mean()), "fallback": bool(fb)}
            same = bool(torch.equal(ans[0][1], ans[1][1]) and torch.equal(ans[0][0].view(torch.int32), ans[1][0].view(torch.int32)))
            print(json.dumps({
                "rows": a.rows, "dim": a.dim, "dtype": a.dtype, "nq": nq, "k": k, "plan_parent": plans[0], "plan_wide": plans[1],
                "parent_us": {"median": statistics.median(t[0]), "min": min(t[0]), "max": max(t[0])},
                "wide_us": {"median": statistics.median(t[1]), "min": min(t[1]), "max": max(t[1])},
                "same_bits_as_exact": same, "screen": diag,
                "forced_fallback": a.forced_fallback}), flush=True)
    for ix in ixs.values():
        ix.close()


if __name__ == "__main__":
    main()
