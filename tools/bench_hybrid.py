"""Dev tool: what hybrid retrieval costs, on one box in one call.

Corpus: --rows x --dim of --dtype (default 1M x 768 bf16, the int8 copy on as the stores keep it) and, beside it, a
synthetic lexical CSR from a counter-based Zipf-like generator over V = 4096 (splitmix64; --draws bucket draws per
row, repeats merged: about 120 distinct entries per row at the default).  Per nq (1 / 8 / 32 / 256), k = --k,
fetch_k = --fetch-k, by HIP events around --iters back-to-back calls, median of --repeats:
  lex_us           rfx_lex_search alone at fetch_k (weight tables + scan + merge)
  fuse_us          rfx_lex_fuse alone: 2 x fetch_k candidates -> k
  dense_fetch_us   the dense search at fetch_k, the exact index's own search (the path the retriever's hybrid
                   batch takes: DeviceIndex.search, whatever plan it picks, the two-pass scan included)
  hybrid_us        dense at fetch_k + lexical at fetch_k + fuse, back to back: the whole hybrid answer
  search_k_us      the plain dense search at k: what the question costs without hybrid, on this build
For the lexical search it prints the algorithmic bytes (entries x 4 + indptr + len, once per group of questions)
and the rate they imply against the measured copy rate (--copy-tbps, 6.29).
--baseline-tree DIR (a built checkout of the parent commit): search_k_us is ALSO measured in a fresh child process
that imports that tree's package and library, on the same corpus and queries (baseline_search_k_us): the check
that nothing existing moved.

Prints a table and one JSON line, and writes profiles/r11/hybrid_bench.json (or --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

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


def splitmix64(x):
    import numpy as np
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def synth_csr(seed, row0, n, V, draws, skew=2.0):
    """Rows row0 .. row0 + n - 1: `draws` Zipf-like bucket draws each (bucket = floor(V * u ** skew)), sorted; a
    repeated bucket keeps its first draw and the others get count 0, which the index drops; tf 1..9."""
    import numpy as np
    key = (np.uint64(seed) << np.uint64(40)) + (np.arange(row0, row0 + n, dtype=np.uint64)[:, None] * np.uint64(draws)
                                                 + np.arange(draws, dtype=np.uint64)[None, :])
    h = splitmix64(key)
    u = ((h >> np.uint64(40)).astype(np.float64) + 0.5) / float(1 << 24)
    bucket = np.minimum((V * u ** skew).astype(np.int32), V - 1)
    order = np.argsort(bucket, axis=1, kind="stable")
    bucket = np.take_along_axis(bucket, order, axis=1)
    tf = (1 + ((h & np.uint64(0xFFFF)) % np.uint64(9))).astype(np.int16)
    tf = np.take_along_axis(tf, order, axis=1)
    tf[:, 1:][bucket[:, 1:] == bucket[:, :-1]] = 0
    indptr = (np.arange(n + 1, dtype=np.int64) * draws).astype(np.int32)
    return indptr, bucket.reshape(-1), tf.reshape(-1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--fetch-k", type=int, default=40)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 8, 32, 256])
    ap.add_argument("--V", type=int, default=4096)
    ap.add_argument("--draws", type=int, default=160)
    ap.add_argument("--q-terms", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--screen", type=int, default=1, help="keep the int8 copy (the two-pass scan) as the stores do")
    ap.add_argument("--copy-tbps", type=float, default=6.29, help="the measured device copy rate, TB/s")
    ap.add_argument("--baseline-tree", default=None, help="a built checkout of the parent commit, for search_k_us")
    ap.add_argument("--search-only", action="store_true", help="(child of --baseline-tree) the plain searches only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "hybrid_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from rfx import _lib
    from rfx.index import DeviceIndex, synth_rows

    torch.cuda.set_device(0)
    ix = DeviceIndex(args.dim, args.dtype, 0)
    ix.add_synthetic(7, args.rows)
    if args.screen:
        ix.enable_screen(1)
    res = {"rows": args.rows, "dim": args.dim, "dtype": args.dtype, "screen": args.screen, "iters": args.iters,
           "repeats": args.repeats, "k": args.k, "fetch_k": args.fetch_k, "build_id": _lib.BUILD_ID}
    lex = None
    if not args.search_only:
        from rfx.lexical import LexIndex
        lex = LexIndex(args.V)
        t0 = time.monotonic()
        step = 100_000
        for lo in range(0, args.rows, step):
            lex.add_csr(*synth_csr(3, lo, min(step, args.rows - lo), args.V, args.draws))
        rows, live, nnz, total_len = lex.info()
        alg = nnz * 4 + (rows + 1) * 8 + rows * 4
        res.update({"V": args.V, "lex_entries": nnz, "entries_per_row": nnz / rows, "avg_len": total_len / live,
                    "lex_build_s_generator_and_add": time.monotonic() - t0, "scan_bytes_per_group": alg,
                    "copy_tbps": args.copy_tbps})
    cells = []
    for nq in args.nq:
        q = synth_rows(11, 0, nq, args.dim, args.dtype, 0)
        ws = torch.empty(max(ix.workspace_bytes(nq, 64), ix.workspace_bytes(nq, args.k), 1), dtype=torch.uint8, device="cuda")
        sk, sk_spread = timed_us(lambda: ix.search(q, args.k, workspace=ws), args.iters, args.repeats)
        c = {"nq": nq, "search_k_us": sk, "search_k_spread": sk_spread}
        cells.append(c)
        if args.search_only:
            continue
        fk = args.fetch_k
        qip, qbk, qct = synth_csr(5, 0, nq, args.V, args.q_terms)
        qcsr = (qip, qbk, np.where(qct > 0, 1, 0).astype(np.int16))
        lws = torch.empty(lex.workspace_bytes(nq, fk), dtype=torch.uint8, device="cuda")
        ls = torch.empty((nq, fk), dtype=torch.float32, device="cuda")
        lr = torch.empty((nq, fk), dtype=torch.int64, device="cuda")
        lx, lx_spread = timed_us(lambda: lex.search(qcsr, fk, out=(ls, lr), workspace=lws), args.iters, args.repeats)
        df, df_spread = timed_us(lambda: ix.search(q, fk, workspace=ws), args.iters, args.repeats)
        _, dr = ix.search(q, fk, workspace=ws)
        fo = (torch.empty((nq, args.k), dtype=torch.float32, device="cuda"),
              torch.empty((nq, args.k), dtype=torch.int64, device="cuda"), None)
        fu, fu_spread = timed_us(lambda: lex.fuse(dr, lr, args.k, 0.5, out=fo), args.iters, args.repeats)

        def hybrid():
            _, d = ix.search(q, fk, workspace=ws)
            lex.search(qcsr, fk, out=(ls, lr), workspace=lws)
            lex.fuse(d, lr, args.k, 0.5, out=fo)

        hy, hy_spread = timed_us(hybrid, args.iters, args.repeats)
        groups = 1 if nq == 1 else (nq + 7) // 8
        found = int((lr[:, 0] >= 0).sum())
        c.update({"lex_us": lx, "lex_spread": lx_spread, "fuse_us": fu, "fuse_spread": fu_spread, "dense_fetch_us": df,
                  "dense_fetch_spread": df_spread, "hybrid_us": hy, "hybrid_spread": hy_spread, "groups": groups,
                  "lex_alg_bytes": res["scan_bytes_per_group"] * groups,
                  "lex_tbps": res["scan_bytes_per_group"] * groups / (lx * 1e-6) / 1e12,
                  "lex_fraction_of_copy": res["scan_bytes_per_group"] * groups / (lx * 1e-6) / 1e12 / args.copy_tbps,
                  "plan_k": ix.search_plan(nq, args.k), "plan_fetch": ix.search_plan(nq, fk),
                  "questions_with_a_lexical_hit": found})
    res["cells"] = cells
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
            c["search_k_vs_baseline"] = c["search_k_us"] / b["search_k_us"] - 1.0
    print(f"{'nq':>4} {'lex_us':>9} {'TB/s':>6} {'of copy':>7} {'fuse_us':>8} {'dense@fetch':>11} {'hybrid_us':>9} "
          f"{'search@k':>9} {'parent@k':>9} {'delta':>7}")
    for c in cells:
        print(f"{c['nq']:>4} {c['lex_us']:>9.1f} {c['lex_tbps']:>6.2f} {c['lex_fraction_of_copy']:>7.3f} {c['fuse_us']:>8.1f} "
              f"{c['dense_fetch_us']:>11.1f} {c['hybrid_us']:>9.1f} {c['search_k_us']:>9.1f} "
              f"{c.get('baseline_search_k_us', float('nan')):>9.1f} {c.get('search_k_vs_baseline', float('nan')):>7.3f}")
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
