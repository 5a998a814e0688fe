"""Dev tool: what a store compaction costs and what it buys, in ONE process on one box.

Per cell: --rows x --dim (default 1M x 768 bf16), files of --file-rows rows, a uniformly chosen 10 / 25 / 50 /
90 % of the files deleted.

Index level (the deleted files' rows tombstoned):
  gather_ms    the gather kernel alone, by HIP events around its launch inside rfx_index_compact
               (DeviceIndex.compact_times)
  copy_ms      a plain device-to-device copy of the same number of bytes (the kept rows), by HIP events, in the
               same process: the measured copy rate the gather is held against; gather_ratio = gather / copy
  compact_ms   the whole rfx_index_compact call by wall clock (it synchronises), and its other phases by the
               host clock: alloc (new allocation, mapping, table upload, NaN tail), release (device
               synchronise + unmap of the old rows), bitmap (host tombstone bitmap), screen (int8 copy rebuild)
  search       nq 1 and nq 256 at k 10 by HIP events (--iters back-to-back searches, median of --repeats):
               before the compaction (the tombstoned store), after it, and on a FRESH index built from the kept
               rows only; spread = (max - min) / median over the repeats.  The answers after the compaction and
               of the fresh index are compared: equal rows, equal score bits.
Store level (--store-rows, default = --rows; a LocalStore in a temporary directory, every file one
add_document commit, the same share of the files deleted through delete_file):
  store_compact_s   LocalStore.compact() wall time, the file rewrite and its fsyncs included
  follow_s / reload_s   another LocalStore object standing at the compacted version catches up on its own
               index, against a fresh object that loads the new generation from disk (the only behaviour
               before compaction existed)

Prints a table and one JSON line, and writes profiles/r09/compact_sweep.json (or --out)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rag-foundation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def keep_ranges(rng, n_rows, file_rows, deleted):
    """(kept ranges with touching files joined, deleted file numbers) for a uniformly chosen fraction."""
    n_files = n_rows // file_rows
    dead = np.sort(rng.choice(n_files, size=int(round(deleted * n_files)), replace=False))
    alive = np.setdiff1d(np.arange(n_files), dead)
    out = []
    for f in alive.tolist():
        first = f * file_rows
        if out and out[-1][0] + out[-1][1] == first:
            out[-1] = (out[-1][0], out[-1][1] + file_rows)
        else:
            out.append((first, file_rows))
    return out, dead


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--file-rows", type=int, default=64)
    ap.add_argument("--deleted", type=float, nargs="+", default=[0.1, 0.25, 0.5, 0.9])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--store-rows", type=int, default=-1, help="rows of the store-level part (-1: --rows; 0 skips it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "compact_sweep.json"))
    args = ap.parse_args()

    import torch
    from rfx import _lib
    from rfx import store as rstore
    from rfx.index import DeviceIndex, synth_rows

    torch.cuda.set_device(0)
    rb = args.dim * _lib.ESIZE[args.dtype]
    rows = args.rows // args.file_rows * args.file_rows

    def timed_search(ix, q):
        ws = torch.empty(max(ix.workspace_bytes(q.shape[0], args.k), 1), dtype=torch.uint8, device="cuda")
        ix.search(q, args.k, workspace=ws)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                out = ix.search(q, args.k, workspace=ws)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / args.iters)
        med = statistics.median(ms)
        return med, (max(ms) - min(ms)) / med, out

    queries = {nq: synth_rows(2, 0, nq, args.dim, args.dtype) for nq in (1, 256)}
    warm = DeviceIndex(args.dim, args.dtype)  # the first launch of the gather loads its code object
    warm.add_synthetic(1, 4096)
    warm.compact([(0, 64), (1024, 512)])
    warm.close()
    cells = []
    for deleted in args.deleted:
        ranges, dead = keep_ranges(np.random.default_rng(17), rows, args.file_rows, deleted)
        kept = sum(n for _, n in ranges)
        ix = DeviceIndex(args.dim, args.dtype)
        ix.add_synthetic(1, rows)
        dead_rows = (dead[:, None] * args.file_rows + np.arange(args.file_rows)[None, :]).reshape(-1)
        ix.tombstone(dead_rows)
        cell = {"deleted": deleted, "rows": rows, "kept": kept, "ranges": len(ranges), "kept_bytes": kept * rb}
        for nq, q in queries.items():
            cell[f"before_nq{nq}_ms"], cell[f"before_nq{nq}_spread"], _ = timed_search(ix, q)
        # the fresh index over the kept rows, and the copy yardstick on the same bytes
        keep_idx = torch.from_numpy(np.concatenate([np.arange(f, f + n) for f, n in ranges])).to("cuda")
        kept_rows = ix.read(0, rows)[keep_idx].contiguous()
        dst = torch.empty_like(kept_rows)
        cp = []
        for _ in range(args.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(kept_rows)
            e1.record()
            e1.synchronize()
            cp.append(e0.elapsed_time(e1))
        cell["copy_ms"] = statistics.median(cp[1:])
        del dst
        fresh = DeviceIndex(args.dim, args.dtype)
        fresh.add(kept_rows)
        del kept_rows, keep_idx
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert ix.compact(ranges) == kept
        cell["compact_ms"] = (time.perf_counter() - t0) * 1e3
        for name, ms in ix.compact_times().items():
            cell[f"{name}_ms"] = ms
        cell["gather_ratio"] = cell["gather_ms"] / cell["copy_ms"]
        cell["call_ratio"] = cell["compact_ms"] / cell["copy_ms"]
        cell["copy_tb_s"] = 2 * kept * rb / cell["copy_ms"] / 1e9
        same = True
        for nq, q in queries.items():
            cell[f"after_nq{nq}_ms"], cell[f"after_nq{nq}_spread"], a = timed_search(ix, q)
            cell[f"fresh_nq{nq}_ms"], cell[f"fresh_nq{nq}_spread"], b = timed_search(fresh, q)
            same = same and torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        cell["after_equals_fresh"] = bool(same)
        cells.append(cell)
        ix.close()
        fresh.close()
        print(json.dumps(cell), flush=True)

    store_rows = rows if args.store_rows < 0 else args.store_rows // args.file_rows * args.file_rows
    for cell in cells if store_rows else []:
        n_files = store_rows // args.file_rows
        with tempfile.TemporaryDirectory() as root:
            reg = rstore.StoreRegistry(root=root, device=0)
            st = reg.create("bench", args.dim, args.dtype)
            fids = []
            t0 = time.perf_counter()
            for i in range(n_files):
                chunks = [f"{i}-{j}" for j in range(args.file_rows)]
                fids.append(st.add_document(chunks, synth_rows(3, i * args.file_rows, args.file_rows, args.dim, args.dtype),
                                            f"{i}.md")[0])
            build_s = time.perf_counter() - t0
            dead = np.random.default_rng(17).choice(n_files, size=int(round(cell["deleted"] * n_files)), replace=False)
            for i in dead.tolist():
                st.delete_file(fids[i])
            follower = rstore.StoreRegistry(root=root, device=0).get(st.name)
            out = st.compact()
            t0 = time.perf_counter()
            follower.refresh()
            torch.cuda.synchronize()
            follow_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            loaded = rstore.StoreRegistry(root=root, device=0).get(st.name)
            torch.cuda.synchronize()
            reload_s = time.perf_counter() - t0
            assert follower.index.rows == loaded.index.rows == out["rows"]
            cell["store"] = {"rows": n_files * args.file_rows, "files": n_files, "kept": out["rows"], "build_s": build_s,
                             "store_compact_s": out["seconds"], "follow_s": follow_s, "reload_s": reload_s}
            for s_ in (follower, loaded, st):
                s_.close()
        print(json.dumps({"deleted": cell["deleted"], **cell["store"]}), flush=True)

    print(f"{'deleted':>8} {'kept':>9} {'ranges':>7} {'gather':>8} {'copy':>8} {'ratio':>6} {'call':>8} | "
          f"{'nq1 before/after/fresh (ms)':>30} | {'nq256 before/after/fresh (ms)':>32}")
    for c in cells:
        print(f"{c['deleted']:8.2f} {c['kept']:9d} {c['ranges']:7d} {c['gather_ms']:7.3f}m {c['copy_ms']:7.3f}m "
              f"{c['gather_ratio']:6.2f} {c['compact_ms']:7.2f}m | {c['before_nq1_ms']:9.4f} {c['after_nq1_ms']:9.4f} {c['fresh_nq1_ms']:9.4f} | "
              f"{c['before_nq256_ms']:10.4f} {c['after_nq256_ms']:10.4f} {c['fresh_nq256_ms']:10.4f}")
    result = {"tool": "bench_compact", "build_id": _lib.BUILD_ID, "dim": args.dim, "dtype": args.dtype,
              "file_rows": args.file_rows, "k": args.k, "iters": args.iters, "repeats": args.repeats, "cells": cells}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
