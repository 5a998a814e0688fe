#!/usr/bin/env python3
"""The sampled-threshold deep search against its two yardsticks, over the cells of DESIGN §4.18's table.

Per cell (rows x nq x k), in one process and alternating within every repeat:
  deep_us      DeviceIndex.search_deep           (the parent's route, and the fallback of the new one)
  sampled_us   DeviceIndex.search_deep_sampled
  matmul_us    torch.matmul + torch.topk on the same device and rows
HIP events around `--iters` back-to-back calls over rotating query sets; median and spread ((max - min) / median)
of `--repeats`.  `fell` = questions of the checked call that took the fallback; `oracle` = two questions of the
cell against the f64 rule.  The per-kernel split (sample / tau-select / main / select / re-score) is a run of its
own: rocprofv3 --kernel-trace --stats -- python tools/bench_deep_sampled.py --only sampled --repeats 1
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rag-foundation_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def alternated_us(routes, iters, repeats):
    """{name: (median us, spread)}: in every repeat each route runs `iters` calls, one route after the other."""
    import torch
    for fns in routes.values():
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in routes}
    for _ in range(repeats):
        for name, fns in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(iters):
                fns[i % len(fns)]()
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) * 1000.0 / iters)
    return {name: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for name, v in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 8, 32, 256])
    ap.add_argument("--k", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sets", type=int, default=3, help="query sets in rotation")
    ap.add_argument("--only", nargs="+", default=["deep", "sampled", "matmul"], help="routes to time")
    ap.add_argument("--matmul-max-bytes", type=int, default=24 << 30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_sampled_bench.json"))
    args = ap.parse_args()

    import torch
    from bench_deep import check_sample
    from rfx import _lib
    from rfx.index import DeviceIndex, deep_sampled_plan, synth_rows

    torch.cuda.set_device(0)
    ix = DeviceIndex(args.dim, args.dtype, 0)
    ix.add_synthetic(7, args.rows)
    x = ix.read(0, args.rows)
    cells = []
    for nq in args.nq:
        qs = [synth_rows(11 + i, 0, nq, args.dim, args.dtype, 0) for i in range(args.sets)]
        for k in args.k:
            wd = torch.empty(ix.deep_workspace_bytes(nq, k), dtype=torch.uint8, device="cuda")
            wsm = torch.empty(ix.deep_sampled_workspace_bytes(nq, k), dtype=torch.uint8, device="cuda")
            routes = {}
            if "deep" in args.only:
                routes["deep"] = [lambda q=q: ix.search_deep(q, k, workspace=wd) for q in qs]
            if "sampled" in args.only:
                routes["sampled"] = [lambda q=q: ix.search_deep_sampled(q, k, workspace=wsm) for q in qs]
            if "matmul" in args.only and nq * args.rows * 4 <= args.matmul_max_bytes:
                routes["matmul"] = [lambda q=q: torch.topk(q @ x.T, k, dim=1) for q in qs]
            t = alternated_us(routes, args.iters, args.repeats)
            s, r, fell = ix.search_deep_sampled(qs[-1], k, workspace=wsm, stats=True)
            probs = check_sample(ix, x, qs[-1], s, r, k, 2)
            dense, S, stride, cap, qwg, ranges = deep_sampled_plan(args.rows, args.dim, args.dtype, nq, k)
            cell = {"nq": nq, "k": k, "S": S, "cap": cap, "q_per_wg": qwg, "ranges": ranges, "fell": fell,
                    "workspace_mb": wsm.numel() / 1e6, "oracle_problems": probs[:3]}
            for name, (us, spread) in t.items():
                cell[name + "_us"], cell[name + "_spread"] = us, spread
            cells.append(cell)
            print(" ".join(f"{a}={cell[a]:.1f}" if isinstance(cell[a], float) else f"{a}={cell[a]}" for a in cell), flush=True)
    res = {"rows": args.rows, "dim": args.dim, "dtype": args.dtype, "iters": args.iters, "repeats": args.repeats,
           "build_id": _lib.BUILD_ID, "cells": cells}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
