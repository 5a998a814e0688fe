"""Dev tool: what a deep search costs on an f32 store (k in 65..1024), on one box in one call.

Per store size (--rows, default 100k, 1M and 10M x --dim 768 f32) and cell (nq 1 / 8 / 32 / 256, k 100 / 1000), by
HIP events around --iters back-to-back calls over rotating query sets; the three routes take turns inside every
repeat, and the median of --repeats is reported:
  deep_us      DeviceIndex.search_deep
  hbm_share    rows * dim * 4 B * question groups / deep_us, as a share of --peak-gbs (the rows are read once per
               question group; the merge and the workspace are not counted)
  matmul_us    torch.matmul + torch.topk on the same device and data: the only other way to these answers (it
               materialises nq x rows f32 scores; skipped past --matmul-max-bytes)
  search64_us  search(k=64) of the same build: the floor a 64-row answer costs
Every cell's last answer is checked on --sample questions against the f64 oracle rule (the candidates of an f32
matmul at depth 2k, re-scored in f64 on the host, judged by oracle.search.check_topk).

Prints a table and one JSON line, and writes profiles/deep_f32_bench.json (or --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rag-foundation_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed_routes_us(routes, iters, repeats):
    """routes: {name: [fn per query set]}.  Per route the median over `repeats` of the mean time of `iters`
    back-to-back calls (its fns in rotation), by HIP events; the routes alternate inside each repeat."""
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
    ap.add_argument("--rows", type=int, nargs="+", default=[100_000, 1_000_000, 10_000_000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 8, 32, 256])
    ap.add_argument("--k", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sets", type=int, default=3, help="query sets in rotation")
    ap.add_argument("--sample", type=int, default=2, help="questions of a cell checked against the oracle")
    ap.add_argument("--peak-gbs", type=float, default=8000.0, help="HBM peak of the device, GB/s")
    ap.add_argument("--matmul-max-bytes", type=int, default=24 << 30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_f32_bench.json"))
    args = ap.parse_args()

    import torch
    from bench_deep import check_sample
    from rfx import _lib
    from rfx.index import DeviceIndex, deep_plan, synth_rows

    torch.cuda.set_device(0)
    cells = []
    for rows in args.rows:
        ix = DeviceIndex(args.dim, "f32", 0)
        ix.add_synthetic(7, rows)
        x = ix.read(0, rows)
        for nq in args.nq:
            qs = [synth_rows(11 + i, 0, nq, args.dim, "f32", 0) for i in range(args.sets)]
            ws64 = torch.empty(max(ix.workspace_bytes(nq, 64), 1), dtype=torch.uint8, device="cuda")
            for k in args.k:
                ws = torch.empty(ix.deep_workspace_bytes(nq, k), dtype=torch.uint8, device="cuda")
                routes = {"deep": [lambda q=q: ix.search_deep(q, k, workspace=ws) for q in qs],
                          "search64": [lambda q=q: ix.search(q, 64, workspace=ws64) for q in qs]}
                if nq * rows * 4 <= args.matmul_max_bytes:
                    routes["matmul"] = [lambda q=q: torch.topk(q @ x.T, k, dim=1) for q in qs]
                t = timed_routes_us(routes, args.iters, args.repeats)
                s, r = ix.search_deep(qs[-1], k, workspace=ws)
                probs = check_sample(ix, x, qs[-1], s, r, k, args.sample)
                # the split is dtype-blind; the plan query describes the bf16 / f16 scan and refuses f32
                ranges, _, kb, qg = deep_plan(rows, args.dim, "bf16", nq, k)
                groups = -(-nq // qg)
                deep = t["deep"][0]
                cells.append({"rows": rows, "nq": nq, "k": k, "deep_us": deep, "deep_spread": t["deep"][1],
                              "matmul_us": t["matmul"][0] if "matmul" in t else None, "search64_us": t["search64"][0],
                              "search64_spread": t["search64"][1], "ranges": ranges, "kb": kb, "q_per_wg": qg,
                              "hbm_share": rows * args.dim * 4 * groups / (deep * 1e-6) / (args.peak_gbs * 1e9),
                              "oracle_problems": probs[:3]})
        del x
        ix.close()
        torch.cuda.empty_cache()
    res = {"dim": args.dim, "dtype": "f32", "iters": args.iters, "repeats": args.repeats, "build_id": _lib.BUILD_ID,
           "cells": cells}
    print(f"{'rows':>9} {'nq':>4} {'k':>5} {'deep_us':>11} {'hbm':>6} {'matmul_us':>11} {'search64_us':>11} {'oracle':>7}")
    for c in cells:
        print(f"{c['rows']:>9} {c['nq']:>4} {c['k']:>5} {c['deep_us']:>11.1f} {c['hbm_share']:>6.2f} "
              f"{c['matmul_us'] if c['matmul_us'] is not None else float('nan'):>11.1f} {c['search64_us']:>11.1f} "
              f"{'ok' if not c['oracle_problems'] else 'FAIL':>7}")
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
