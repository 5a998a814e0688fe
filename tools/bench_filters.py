"""Dev tool: a batch of questions under DIFFERENT metadata filters, the segmented search (one launch that reads
only the selected rows, rfx_search_segmented) against the path it replaces (one masked search per
distinct filter, each reading the whole store), in ONE process on one box.

Shape: a 1M x 768 bf16 store; 32 questions under 32 distinct filters; each filter selects `selectivity` of the
rows as file-shaped ranges (files of --file-rows rows drawn per filter from a seeded generator, touching files
joined, as LocalStore.segment_ranges hands them over); selectivity 0.1 % / 1 % / 10 % / 50 %; k = 10.

Timing: HIP events around `--iters` back-to-back batches on one stream, `--repeats` times after a warm-up of both
paths, the two paths ALTERNATING within every repeat; the figure is the median repeat, `spread` the
(max - min) / median over the repeats.  The segmented figure includes what the call does on the host (work
list, table upload, the permutation into group order); the masked figure is 32 DeviceIndex.search calls with
their device masks built beforehand (the store caches them).  Every answer of the last pass is compared between
the two paths: equal rows, equal score bits (one score rule).

bytes: what each path's scans read by the algorithm: selected rows x ceil(questions / 8) x row bytes per filter
against filters x store rows x row bytes.

Prints a table and one JSON line, and writes profiles/r08/filters_sweep.json (or --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rag-foundation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def filter_ranges(rng, n_rows, file_rows, selectivity):
    """Sorted (first, count) ranges of about selectivity * n_rows rows: whole files, touching ones joined."""
    n_files = n_rows // file_rows
    want = max(1, int(round(selectivity * n_rows / file_rows)))
    files = np.sort(rng.choice(n_files, size=min(want, n_files), replace=False))
    out = []
    for f in files.tolist():
        first = f * file_rows
        if out and out[-1][0] + out[-1][1] == first:
            out[-1] = (out[-1][0], out[-1][1] + file_rows)
        else:
            out.append((first, file_rows))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--filters", type=int, default=32)
    ap.add_argument("--per-filter", type=int, default=1, help="questions per filter")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--file-rows", type=int, default=500)
    ap.add_argument("--selectivity", type=float, nargs="+", default=[0.001, 0.01, 0.1, 0.5])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "filters_sweep.json"))
    a = ap.parse_args()

    import torch
    from rfx import filters as rfilters
    from rfx.index import DeviceIndex, synth_rows

    if not torch.cuda.is_available():
        raise SystemExit("bench_filters.py needs a GPU (there is no CPU path)")
    torch.cuda.set_device(0)
    ix = DeviceIndex(a.dim, a.dtype, 0)
    ix.add_synthetic(0, a.rows)
    nq = a.filters * a.per_filter
    q = synth_rows(1, 0, nq, a.dim, a.dtype, 0)
    esz = 4 if a.dtype == "f32" else 2
    row_bytes = a.dim * esz
    results = []
    for sel in a.selectivity:
        rng = np.random.default_rng(int(sel * 1e6) + 17)
        per_filter = [filter_ranges(rng, a.rows, a.file_rows, sel) for _ in range(a.filters)]
        # questions interleaved over the filters, as concurrent tenants' questions arrive
        groups = [([g + a.filters * j for j in range(a.per_filter)], per_filter[g]) for g in range(a.filters)]
        masks = [ix.mask_tensor(rfilters.row_mask_words(a.rows, rngs)) for rngs in per_filter]
        qg = [q[torch.as_tensor(idx, device=q.device)] for idx, _ in groups]
        wss = torch.empty(max(ix.workspace_bytes(a.per_filter, a.k), 1), dtype=torch.uint8, device="cuda")

        def run_seg():
            return ix.search_segmented(q, a.k, groups)

        def run_masked():
            return [ix.search(qg[g], a.k, workspace=wss, row_mask=masks[g]) for g in range(a.filters)]

        for _ in range(a.warmup):
            run_seg()
            run_masked()
        torch.cuda.synchronize()
        t = {"segmented": [], "masked": []}
        for _ in range(a.repeats):
            for name, fn in (("segmented", run_seg), ("masked", run_masked)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                e1.synchronize()
                t[name].append(e0.elapsed_time(e1) * 1000.0 / a.iters)
        ss, sr = run_seg()
        ms = [(s.clone(), r.clone()) for s, r in run_masked()]  # (one workspace: clone before the next search)
        torch.cuda.synchronize()
        ss, sr = ss.cpu().numpy(), sr.cpu().numpy()
        rows_differ = bits_differ = 0
        for g, (idx, _) in enumerate(groups):
            m_s, m_r = ms[g][0].cpu().numpy(), ms[g][1].cpu().numpy()
            rows_differ += int((m_r != sr[idx]).any(axis=1).sum())
            same = m_r == sr[idx]
            bits_differ += int((m_s.view(np.uint32)[same] != ss[idx].view(np.uint32)[same]).sum())
        sel_rows = [sum(n for _, n in rngs) for rngs in per_filter]
        seg_bytes = sum(n * ((a.per_filter + 7) // 8) for n in sel_rows) * row_bytes
        masked_bytes = a.filters * a.rows * row_bytes
        med = {name: statistics.median(v) for name, v in t.items()}
        results.append({
            "selectivity": sel, "selected_rows_per_filter": int(np.mean(sel_rows)),
            "ranges_per_filter": int(np.mean([len(r) for r in per_filter])),
            "segmented_us": med["segmented"], "masked_us": med["masked"],
            "segmented_spread": (max(t["segmented"]) - min(t["segmented"])) / med["segmented"],
            "masked_spread": (max(t["masked"]) - min(t["masked"])) / med["masked"],
            "speedup": med["masked"] / med["segmented"],
            "segmented_bytes": seg_bytes, "masked_bytes": masked_bytes,
            "segmented_GBps": seg_bytes / med["segmented"] / 1e3, "masked_GBps": masked_bytes / med["masked"] / 1e3,
            "queries_with_other_rows": rows_differ, "score_bits_differ": bits_differ,
            "segmented_us_repeats": t["segmented"], "masked_us_repeats": t["masked"],
        })
    print(f"{a.rows} x {a.dim} {a.dtype}, {a.filters} filters x {a.per_filter} questions, k={a.k}, files of {a.file_rows} rows")
    print("select  rows/filter  ranges  segmented us (spread)  masked us (spread)  masked/seg   seg MB   masked MB  rows differ")
    for r in results:
        print(f"{r['selectivity']:6.3f}  {r['selected_rows_per_filter']:11d}  {r['ranges_per_filter']:6d}  "
              f"{r['segmented_us']:12.1f} ({r['segmented_spread']:.2f})  {r['masked_us']:9.1f} ({r['masked_spread']:.2f})  "
              f"{r['speedup']:10.2f}  {r['segmented_bytes'] / 1e6:7.1f}  {r['masked_bytes'] / 1e6:10.1f}  "
              f"{r['queries_with_other_rows']:d}")
    faster = [r["selectivity"] for r in results if r["speedup"] > 1.0]
    out = {"shape": {"rows": a.rows, "dim": a.dim, "dtype": a.dtype, "filters": a.filters, "per_filter": a.per_filter,
                     "k": a.k, "file_rows": a.file_rows, "iters": a.iters, "repeats": a.repeats},
           "largest_fraction_segmented_faster": max(faster) if faster else None, "results": results}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    if any(r["queries_with_other_rows"] or r["score_bits_differ"] for r in results):
        raise SystemExit("the two paths disagree")


if __name__ == "__main__":
    main()
