"""Dev tool: what the distinct-document search costs next to the plain search of the same call.

Two corpora of --rows x --dim rows of --dtype (default 1M x 768 bf16, the int8 copy on as the stores keep it),
cut into files of --chunks rows (default 40):
  spread    synthetic rows: the best fetch_k rows of a question come from many files, round 1 completes
  dominant  the same rows plus ONE file of 256 near-copies of the questions' common direction: it owns the best
            64 rows of every question, so a completion round runs
Per corpus and nq (default 1 / 8 / 32 / 256) at k = --k, by HIP events around --iters back-to-back calls, median
of --repeats:
  search_k_us      the plain search at k
  search_fetch_us  the plain search at fetch_k = default_fetch_k(k)
  distinct_us      DeviceIndex.search_distinct (its host copies and its rounds included), and the rounds taken
Each of the three answers is checked on --check questions against the CPU reference: the oracle's exact top
--depth rows (oracle.search.topk_blocks over the stored rows read back), collapsed by file for the distinct one.

Prints a table and one JSON line, and writes profiles/r11/distinct_bench.json (or --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rag-foundation_amd")):
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


def reference(ix, q, row_doc_h, k, depth, block=1 << 16):
    """CPU: (plain rows [n][depth], distinct rows [n][k]) of the questions q, from the oracle's exact top `depth`."""
    import numpy as np
    from oracle import search as osearch
    q64 = q.float().cpu().numpy().astype(np.float64)
    blocks = ((r0, ix.read(r0, min(block, ix.rows - r0)).float().cpu().numpy()) for r0 in range(0, ix.rows, block))
    s, r = osearch.topk_blocks(q64, blocks, depth)
    order = [np.lexsort((r[i], -s[i].astype(np.float32))) for i in range(len(r))]  # the rule: fl32 desc, row asc
    r = np.stack([r[i][o] for i, o in enumerate(order)])
    dist = np.full((len(r), k), -1, dtype=np.int64)
    for i in range(len(r)):
        seen, n = set(), 0
        for row in r[i]:
            d = int(row_doc_h[row]) if row >= 0 else -1
            if d < 0 or d in seen:
                continue
            seen.add(d)
            dist[i, n] = row
            n += 1
            if n == k:
                break
        assert n == k, f"the top {depth} rows hold only {n} files: raise --depth"
    return r, dist


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--chunks", type=int, default=40)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 8, 32, 256])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--screen", type=int, default=1, help="keep the int8 copy (the two-pass scan) as the stores do")
    ap.add_argument("--check", type=int, default=2, help="questions per corpus checked against the CPU reference")
    ap.add_argument("--depth", type=int, default=1024, help="rows of the exact ranking the reference collapses")
    ap.add_argument("--corpora", nargs="+", default=["spread", "dominant"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "distinct_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from rfx import _lib, distinct
    from rfx.index import DeviceIndex, synth_rows

    torch.cuda.set_device(0)
    tdt = _lib.TORCH_DTYPES[args.dtype]
    fetch_k = distinct.default_fetch_k(args.k)
    nq_max = max(args.nq)
    unit = lambda t: (t / t.norm(dim=1, keepdim=True)).to(tdt)
    cells = []
    for name in args.corpora:
        ix = DeviceIndex(args.dim, args.dtype, 0)
        ix.add_synthetic(7, args.rows)
        if name == "dominant":
            base = synth_rows(99, 0, 1, args.dim, "f32", 0)
            ix.add(unit(base + 0.05 * synth_rows(13, 0, 256, args.dim, "f32", 0)))
            queries = unit(base + 0.05 * synth_rows(11, 0, nq_max, args.dim, "f32", 0))
        else:
            queries = synth_rows(11, 0, nq_max, args.dim, args.dtype, 0)
        if args.screen:
            ix.enable_screen(1)
        n_docs = (args.rows + args.chunks - 1) // args.chunks
        row_doc_h = (np.arange(ix.rows, dtype=np.int64) // args.chunks).astype(np.int32)
        row_doc_h[args.rows:] = n_docs  # the dominant file
        doc_ranges = np.array([(d * args.chunks, min(args.chunks, args.rows - d * args.chunks)) for d in range(n_docs)]
                              + ([(args.rows, ix.rows - args.rows)] if ix.rows > args.rows else []), dtype=np.int64)
        row_doc = torch.from_numpy(row_doc_h).cuda()
        n_chk = min(args.check, nq_max)
        ref_plain, ref_dist = reference(ix, queries[:n_chk], row_doc_h, args.k, args.depth) if n_chk else (None, None)
        for nq in args.nq:
            q = queries[:nq].contiguous()
            sk, sk_sp = timed_us(lambda: ix.search(q, args.k), args.iters, args.repeats)
            sf, sf_sp = timed_us(lambda: ix.search(q, fetch_k), args.iters, args.repeats)
            rounds = []
            ds, ds_sp = timed_us(lambda: rounds.append(ix.search_distinct(q, args.k, row_doc, doc_ranges)[3]),
                                 args.iters, args.repeats)
            m = min(n_chk, nq)
            if m:
                assert np.array_equal(ix.search(q, args.k)[1][:m].cpu().numpy(), ref_plain[:m, :args.k]), (name, nq, "k")
                assert np.array_equal(ix.search(q, fetch_k)[1][:m].cpu().numpy(), ref_plain[:m, :fetch_k]), (name, nq)
                got = ix.search_distinct(q, args.k, row_doc, doc_ranges)
                assert np.array_equal(got[1][:m].cpu().numpy(), ref_dist[:m]), (name, nq, "distinct")
            cells.append({"corpus": name, "nq": nq, "k": args.k, "fetch_k": fetch_k, "search_k_us": sk,
                          "search_k_spread": sk_sp, "search_fetch_us": sf, "search_fetch_spread": sf_sp,
                          "distinct_us": ds, "distinct_spread": ds_sp, "rounds": sorted(set(rounds)),
                          "distinct_over_search_k": ds / sk, "checked_questions": m,
                          "plan_k": ix.search_plan(nq, args.k), "plan_fetch": ix.search_plan(nq, fetch_k)})
        ix.close()
    res = {"rows": args.rows, "dim": args.dim, "dtype": args.dtype, "chunks": args.chunks, "screen": args.screen,
           "iters": args.iters, "repeats": args.repeats, "build_id": _lib.BUILD_ID, "cells": cells}
    print(f"{'corpus':>9} {'nq':>4} {'search@k':>10} {'search@fetch':>12} {'distinct':>10} {'x':>6} rounds")
    for c in cells:
        print(f"{c['corpus']:>9} {c['nq']:>4} {c['search_k_us']:>10.1f} {c['search_fetch_us']:>12.1f} "
              f"{c['distinct_us']:>10.1f} {c['distinct_over_search_k']:>6.2f} {c['rounds']}")
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
