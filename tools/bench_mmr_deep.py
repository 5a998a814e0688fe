"""Dev tool: what the deep MMR selection adds to a deep search, on one box in one call.

Per cell (--rows x --dim of --dtype, default 1M x 768 bf16; nq 1 / 32 / 256 x fetch_k 128 / 1,024 x k 10 / 64,
lambda 0.5), by HIP events around --iters back-to-back calls after a warm-up call, median of --repeats, the query
set rotating between the calls:
  select_us   rfx_mmr_select_deep alone (no objectives asked for): fetch_k candidates -> k picks
  search_us   search_deep at k = fetch_k, the search that feeds it, in the same process
  added       select_us / search_us
  contenders  mean contenders per step and question;  dots: mean exact dots per question
--clustered draws rows and queries from 64 centres (rfx.ivf.synth_clustered) instead of synth_rows: near-copies
make more candidates contend.

Prints a table and one JSON line, and writes profiles/mmr_deep_bench.json (or --out)."""
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
    """Median over `repeats` of the mean time of `iters` back-to-back calls, fns taken in rotation; the spread."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--fetch-k", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--k", type=int, nargs="+", default=[10, 64])
    ap.add_argument("--sets", type=int, default=3, help="query sets in rotation")
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clustered", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmr_deep_bench.json"))
    args = ap.parse_args()

    import torch
    from rfx import _lib
    from rfx.index import DeviceIndex, synth_rows
    from rfx.ivf import synth_clustered

    torch.cuda.set_device(0)
    ix = DeviceIndex(args.dim, args.dtype, 0)
    if args.clustered:
        for r0 in range(0, args.rows, 250_000):
            ix.add(synth_clustered(3, 64, 7, r0, min(250_000, args.rows - r0), args.dim, args.dtype))
    else:
        ix.add_synthetic(7, args.rows)
    cells = []
    for nq in args.nq:
        qs = [synth_clustered(3, 64, 11 + i, 0, nq, args.dim, args.dtype) if args.clustered else
              synth_rows(11 + i, 0, nq, args.dim, args.dtype, 0) for i in range(args.sets)]
        for fk in args.fetch_k:
            sws = torch.empty(ix.deep_workspace_bytes(nq, fk), dtype=torch.uint8, device="cuda")
            search, search_spread = timed_us([lambda q=q: ix.search_deep(q, fk, workspace=sws) for q in qs], args.iters,
                                             args.repeats)
            cands = [ix.search_deep(q, fk, workspace=sws) for q in qs]
            mws = torch.empty(ix.mmr_deep_workspace_bytes(nq, fk), dtype=torch.uint8, device="cuda")
            for k in args.k:
                fns = [lambda q=q, c=c: ix.mmr_select_deep(q, c[0], c[1], k, lam=0.5, workspace=mws) for q, c in zip(qs, cands)]
                sel, sel_spread = timed_us(fns, args.iters, args.repeats)
                _, r, stats = ix.mmr_select_deep(qs[0], *cands[0], k, lam=0.5, workspace=mws, stats=True)
                st = stats.float().mean(dim=0).tolist()
                cells.append({"nq": nq, "fetch_k": fk, "k": k, "select_us": sel, "select_spread": sel_spread,
                              "search_us": search, "search_spread": search_spread, "added": sel / search,
                              "contenders_per_step": st[0] / max(k - 1, 1), "exact_dots": st[1],
                              "selections_differing_from_top_k": int((r != cands[0][1][:, :k]).any(dim=1).sum())})
    res = {"rows": args.rows, "dim": args.dim, "dtype": args.dtype, "clustered": args.clustered, "iters": args.iters,
           "repeats": args.repeats, "sets": args.sets, "build_id": _lib.BUILD_ID, "cells": cells}
    print(f"{'nq':>4} {'fetch_k':>7} {'k':>3} {'select_us':>10} {'search_us':>10} {'added':>6} {'cont/step':>9} {'dots':>7}")
    for c in cells:
        print(f"{c['nq']:>4} {c['fetch_k']:>7} {c['k']:>3} {c['select_us']:>10.1f} {c['search_us']:>10.1f} {c['added']:>6.3f} "
              f"{c['contenders_per_step']:>9.2f} {c['exact_dots']:>7.1f}")
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
