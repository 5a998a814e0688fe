"""Dev tool: what a deep search (k in 65..1024) costs, on one box in one call.

Per cell (--rows x --dim of --dtype, default 1M x 768 bf16; nq 1 / 8 / 32 / 256, k 100 / 1000), by HIP events
around --iters back-to-back calls over rotating query sets, median of --repeats:
  deep_us      DeviceIndex.search_deep
  hbm_share    rows * dim * 2 B * question groups / deep_us, as a share of --peak-gbs (the rows are read once per
               question group; the merge and the workspace are not counted)
  matmul_us    torch.matmul + torch.topk on the same device and data: the only other way to these answers (it
               materialises nq x rows f32 scores; skipped past --matmul-max-bytes)
  search64_us  search(k=64) of the same build: the floor a 64-row answer costs
Every cell's last answer is checked on --sample questions against the f64 oracle rule (the candidates of an f32
matmul at depth 2k, re-scored in f64 on the host, judged by oracle.search.check_topk).

Prints a table and one JSON line, and writes profiles/deep_bench.json (or --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rag-foundation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed_us(fns, iters, repeats):
    """Median over `repeats` of the mean time of `iters` back-to-back calls (fns in rotation), by HIP events."""
    import torch
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fns[i % len(fns)]()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / iters)
    med = statistics.median(out)
    return med, (max(out) - min(out)) / med


def check_sample(ix, x, q, s, r, k, sample):
    """Problems of the answers (s, r) of the first `sample` questions against the f64 rule."""
    import numpy as np
    import torch
    from oracle import search as osearch
    n = min(sample, q.shape[0])
    cand = torch.topk(q[:n].float() @ x.float().T, min(2 * k, x.shape[0]), dim=1).indices
    probs = []
    for i in range(n):
        rows = cand[i].cpu().numpy()
        x64 = x[cand[i]].float().cpu().numpy().astype(np.float64)
        q64 = q[i].float().cpu().numpy().astype(np.float64)
        sc = x64 @ q64
        o = np.lexsort((rows, -sc))[:k]
        by_row = dict(zip(rows.tolist(), sc.tolist()))
        probs += osearch.check_topk(s[i:i + 1].cpu().numpy(), r[i:i + 1].cpu().numpy(), sc[o][None], rows[o][None],
                                    lambda _, rr: np.array([by_row.get(int(v), -np.inf) for v in rr]))
    return probs


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
    ap.add_argument("--sample", type=int, default=2, help="questions of a cell checked against the oracle")
    ap.add_argument("--peak-gbs", type=float, default=8000.0, help="HBM peak of the device, GB/s")
    ap.add_argument("--matmul-max-bytes", type=int, default=24 << 30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_bench.json"))
    args = ap.parse_args()

    import torch
    from rfx import _lib
    from rfx.index import DeviceIndex, deep_plan, synth_rows

    torch.cuda.set_device(0)
    ix = DeviceIndex(args.dim, args.dtype, 0)
    ix.add_synthetic(7, args.rows)
    x = ix.read(0, args.rows)
    cells = []
    for nq in args.nq:
        qs = [synth_rows(11 + i, 0, nq, args.dim, args.dtype, 0) for i in range(args.sets)]
        ws64 = torch.empty(max(ix.workspace_bytes(nq, 64), 1), dtype=torch.uint8, device="cuda")
        s64, s64_spread = timed_us([lambda q=q: ix.search(q, 64, workspace=ws64) for q in qs], args.iters, args.repeats)
        for k in args.k:
            ws = torch.empty(ix.deep_workspace_bytes(nq, k), dtype=torch.uint8, device="cuda")
            deep, spread = timed_us([lambda q=q: ix.search_deep(q, k, workspace=ws) for q in qs], args.iters, args.repeats)
            s, r = ix.search_deep(qs[-1], k, workspace=ws)
            probs = check_sample(ix, x, qs[-1], s, r, k, args.sample)
            ranges, rpr, kb, qg = deep_plan(args.rows, args.dim, args.dtype, nq, k)
            groups = -(-nq // qg)
            mm = None
            if nq * args.rows * 4 <= args.matmul_max_bytes:
                mm, _ = timed_us([lambda q=q: torch.topk(q @ x.T, k, dim=1) for q in qs], args.iters, args.repeats)
            cells.append({"nq": nq, "k": k, "deep_us": deep, "deep_spread": spread, "matmul_us": mm, "search64_us": s64,
                          "search64_spread": s64_spread, "ranges": ranges, "kb": kb, "q_per_wg": qg,
                          "hbm_share": args.rows * args.dim * 2 * groups / (deep * 1e-6) / (args.peak_gbs * 1e9),
                          "oracle_problems": probs[:3]})
    res = {"rows": args.rows, "dim": args.dim, "dtype": args.dtype, "iters": args.iters, "repeats": args.repeats,
           "build_id": _lib.BUILD_ID, "cells": cells}
    print(f"{'nq':>4} {'k':>5} {'deep_us':>10} {'hbm':>6} {'matmul_us':>10} {'search64_us':>11} {'oracle':>7}")
    for c in cells:
        print(f"{c['nq']:>4} {c['k']:>5} {c['deep_us']:>10.1f} {c['hbm_share']:>6.2f} "
              f"{c['matmul_us'] if c['matmul_us'] is not None else float('nan'):>10.1f} {c['search64_us']:>11.1f} "
              f"{'ok' if not c['oracle_problems'] else 'FAIL':>7}")
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
