"""Dev tool: what hybrid retrieval at depth costs, on one box in one call.

The corpus of tools/bench_hybrid.py (--rows x --dim of --dtype, default 1M x 768 bf16, and its synthetic lexical CSR
over V = 4096).  Per nq (1 / 8 / 32 / 256) and k (100, 1,000), by HIP events around --iters back-to-back calls,
median of --repeats:
  lex64_us / lex10_us  rfx_lex_search at k = 64 / 10: the existing path's time, the yardstick
  lex_deep_us          rfx_lex_search_deep at k (weight tables + scan + selection)
  fuse64_us            rfx_lex_fuse: 2 x 64 candidates -> 64, the yardstick
  fuse_deep_us         rfx_lex_fuse_deep: 2 x k candidates -> k
  dense_deep_us        the dense deep search at k (store.flat_search_deep)
  hybrid_deep_us       dense at k + lexical at k + fusion, back to back: the whole hybrid candidate call
Prints a table and one JSON line, and writes profiles/r21/hybrid_deep_bench.json (or --out)."""
import argparse
import json
import os

from bench_hybrid import ROOT, synth_csr, timed_us


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--k", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 8, 32, 256])
    ap.add_argument("--V", type=int, default=4096)
    ap.add_argument("--draws", type=int, default=160)
    ap.add_argument("--q-terms", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "hybrid_deep_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from rfx import _lib
    from rfx.index import DeviceIndex, synth_rows
    from rfx.lexical import LexIndex
    from rfx.store import flat_search_deep

    torch.cuda.set_device(0)
    ix = DeviceIndex(args.dim, args.dtype, 0)
    ix.add_synthetic(7, args.rows)
    lex = LexIndex(args.V)
    for lo in range(0, args.rows, 100_000):
        lex.add_csr(*synth_csr(3, lo, min(100_000, args.rows - lo), args.V, args.draws))
    res = {"rows": args.rows, "dim": args.dim, "dtype": args.dtype, "V": args.V, "iters": args.iters,
           "repeats": args.repeats, "build_id": _lib.BUILD_ID, "cells": []}
    t = lambda fn: timed_us(fn, args.iters, args.repeats)[0]
    for nq in args.nq:
        q = synth_rows(11, 0, nq, args.dim, args.dtype, 0)
        qip, qbk, qct = synth_csr(5, 0, nq, args.V, args.q_terms)
        qcsr = (qip, qbk, np.where(qct > 0, 1, 0).astype(np.int16))
        _, r64 = lex.search(qcsr, 64)
        _, d64 = ix.search(q, 64)
        base = {"nq": nq, "lex10_us": t(lambda: lex.search(qcsr, 10)), "lex64_us": t(lambda: lex.search(qcsr, 64)),
                "fuse64_us": t(lambda: lex.fuse(d64, r64, 64, 0.5))}
        for k in args.k:
            ws = torch.empty(lex.deep_workspace_bytes(nq, k), dtype=torch.uint8, device="cuda")
            _, rl = lex.search_deep(qcsr, k, workspace=ws)
            _, rd = flat_search_deep(ix, q, k, None)

            def hybrid():
                _, d = flat_search_deep(ix, q, k, None)
                _, l = lex.search_deep(qcsr, k, workspace=ws)
                lex.fuse_deep(d, l, k, 0.5)

            c = dict(base, k=k, lex_deep_us=t(lambda: lex.search_deep(qcsr, k, workspace=ws)),
                     fuse_deep_us=t(lambda: lex.fuse_deep(rd, rl, k, 0.5)),
                     dense_deep_us=t(lambda: flat_search_deep(ix, q, k, None)), hybrid_deep_us=t(hybrid))
            res["cells"].append(c)
            print(" ".join(f"{n} {v:.1f}" if isinstance(v, float) else f"{n} {v}" for n, v in c.items()), flush=True)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
