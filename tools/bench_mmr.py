"""Dev tool: what diversified retrieval adds to a search, on one box in one call.

Per cell (--rows x --dim of --dtype, default 1M x 768 bf16, the int8 copy on as the stores keep it; nq 1 / 32 /
256, fetch_k 16 / 64, k = --k), by HIP events around --iters back-to-back calls, median of --repeats:
  select_us        rfx_mmr_select alone: fetch_k candidates -> k picks at lambda 0.5
  search_fetch_us  the search at k = fetch_k that feeds it
  search_k_us      the plain search at k = --k of the same batch: what the question costs without diversity
  added            (search_fetch_us + select_us - search_k_us) / search_k_us
--baseline-tree DIR (a built checkout of the parent commit): search_k_us is ALSO measured in a fresh child
process that imports that tree's package and library, on the same corpus and queries: baseline_search_k_us, and
added_vs_baseline against it.

Prints a table and one JSON line, and writes profiles/r10/mmr_bench.json (or --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("RFX_BENCH_TREE", ROOT)  # (the child of --baseline-tree imports the package from there)
for p in (TREE, os.path.join(TREE, "rag-foundation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed_us(fn, iters, repeats):
    """Median over `repeats` of the mean time of `iters` back-to-back calls, by HIP events; and the spread."""
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
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
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--fetch-k", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--screen", type=int, default=1, help="keep the int8 copy (the two-pass scan) as the stores do")
    ap.add_argument("--baseline-tree", default=None, help="a built checkout of the parent commit, for search_k_us")
    ap.add_argument("--search-only", action="store_true", help="(child of --baseline-tree) the plain searches only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "mmr_bench.json"))
    args = ap.parse_args()

    import torch
    from rfx import _lib
    from rfx.index import DeviceIndex, synth_rows

    torch.cuda.set_device(0)
    ix = DeviceIndex(args.dim, args.dtype, 0)
    ix.add_synthetic(7, args.rows)
    if args.screen:
        ix.enable_screen(1)
    cells = []
    for nq in args.nq:
        q = synth_rows(11, 0, nq, args.dim, args.dtype, 0)
        ws = torch.empty(max(ix.workspace_bytes(nq, 64), ix.workspace_bytes(nq, args.k), 1), dtype=torch.uint8, device="cuda")
        sk, sk_spread = timed_us(lambda: ix.search(q, args.k, workspace=ws), args.iters, args.repeats)
        if args.search_only:
            cells.append({"nq": nq, "k": args.k, "search_k_us": sk, "search_k_spread": sk_spread})
            continue
        for fk in args.fetch_k:
            sf, sf_spread = timed_us(lambda: ix.search(q, fk, workspace=ws), args.iters, args.repeats)
            cs, cr = ix.search(q, fk, workspace=ws)
            mws = torch.empty(ix.mmr_workspace_bytes(nq, fk), dtype=torch.uint8, device="cuda")
            sel, sel_spread = timed_us(lambda: ix.mmr_select(q, cs, cr, args.k, lam=0.5, workspace=mws), args.iters,
                                       args.repeats)
            s, r = ix.mmr_select(q, cs, cr, args.k, lam=0.5, workspace=mws)
            differ = int((r != cr[:, :args.k]).any(dim=1).sum())
            cells.append({"nq": nq, "k": args.k, "fetch_k": fk, "select_us": sel, "select_spread": sel_spread,
                          "search_fetch_us": sf, "search_fetch_spread": sf_spread, "search_k_us": sk,
                          "search_k_spread": sk_spread, "added": (sf + sel - sk) / sk,
                          "plan_k": ix.search_plan(nq, args.k), "plan_fetch": ix.search_plan(nq, fk),
                          "selections_differing_from_top_k": differ})
    res = {"rows": args.rows, "dim": args.dim, "dtype": args.dtype, "screen": args.screen, "iters": args.iters,
           "repeats": args.repeats, "build_id": _lib.BUILD_ID, "cells": cells}
    if args.search_only:
        print(json.dumps(res))
        return
    if args.baseline_tree:
        env = dict(os.environ, RFX_BENCH_TREE=os.path.abspath(args.baseline_tree))
        cmd = [sys.executable, os.path.abspath(__file__), "--search-only", "--rows", str(args.rows), "--dim", str(args.dim),
               "--dtype", args.dtype, "--k", str(args.k), "--iters", str(args.iters), "--repeats", str(args.repeats),
               "--screen", str(args.screen), "--nq"] + [str(n) for n in args.nq]
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, check=True, timeout=600).stdout
        base = json.loads(out.strip().splitlines()[-1])
        res["baseline_build_id"] = base["build_id"]
        by_nq = {c["nq"]: c for c in base["cells"]}
        for c in cells:
            b = by_nq[c["nq"]]
            c["baseline_search_k_us"] = b["search_k_us"]
            c["baseline_search_k_spread"] = b["search_k_spread"]
            c["added_vs_baseline"] = (c["search_fetch_us"] + c["select_us"] - b["search_k_us"]) / b["search_k_us"]
    print(f"{'nq':>4} {'fetch_k':>7} {'select_us':>10} {'search@fetch':>12} {'search@k':>10} {'baseline@k':>10} {'added':>7}")
    for c in cells:
        print(f"{c['nq']:>4} {c['fetch_k']:>7} {c['select_us']:>10.1f} {c['search_fetch_us']:>12.1f} "
              f"{c['search_k_us']:>10.1f} {c.get('baseline_search_k_us', float('nan')):>10.1f} {c['added']:>7.3f}")
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
