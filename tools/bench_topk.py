"""Dev tool: kernel 11 (the two-pass scan of nq <= 8 questions) against the exact one-launch
search at every top_k class, in ONE call on one box (boxes differ by ~5 % with the same build, README).

Shapes: config 2's store (100k x 768 f32) and a 1M x 768 bf16 store; nq in {1, 8}; k in {1, 3, 4, 10, 16,
17, 32, 64}.  For each combination: us per search with the int8 copy on (rfx_search_plan 11) and off (plan 0,
the exact search — what every k outside 5..16 took before round 7).

Timing: HIP events around `--iters` back-to-back searches on one stream, `--repeats` times after a warm-up;
the figure is the median repeat, `spread` the (max - min) / median over the repeats.  Searches rotate through
`--copies` copies of the small store (307 MB of f32 rows would otherwise be re-read from the 256-MB Infinity
Cache) and through 16 different query batches.  Every timed answer of the screened run is compared with the
exact run's for the same (copy, queries): scores within 1e-5, rows equal wherever the scores differ.

Prints a table and writes profiles/r07/topk_sweep.json (or --out)."""
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
import torch  # noqa: E402

NQ_COPIES = 16
KS = (1, 3, 4, 10, 16, 17, 32, 64)
NQS = (1, 8)


def time_case(ixs, qs, nq, k, iters, repeats, warmup):
    """-> (us per search per repeat, the answers of the last pass over every (copy, query batch))."""
    wss = [torch.empty(max(ix.workspace_bytes(nq, k), 1), dtype=torch.uint8, device="cuda") for ix in ixs]
    n_slots = len(ixs) * NQ_COPIES // np.gcd(len(ixs), NQ_COPIES)
    answers = {}

    def run(n, keep):
        for i in range(n):
            c, qi = i % len(ixs), i % NQ_COPIES
            out = ixs[c].search(qs[qi], k, workspace=wss[c])
            if keep and i >= n - n_slots:
                answers[(c, qi)] = out
    run(warmup, False)
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(iters, False)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1000.0 / iters)
    run(n_slots, True)
    torch.cuda.synchronize()
    return us, {key: (s.cpu().numpy(), r.cpu().numpy()) for key, (s, r) in answers.items()}


def compare(on, off):
    worst, bad_rows = 0.0, 0
    for key, (s1, r1) in on.items():
        s0, r0 = off[key]
        fin = np.isfinite(s0)
        if not np.array_equal(fin, np.isfinite(s1)):
            return float("inf"), -1
        diff = np.where(fin, np.abs(np.where(fin, s1, 0.0) - np.where(fin, s0, 0.0)), 0.0)
        worst = max(worst, float(diff.max(initial=0.0)))
        # (two rows within the tie band may swap between the plans; any other row must agree)
        bad_rows += int(((r1 != r0) & (diff > 2e-6)).sum()) + int(((r1 != r0) & ~fin).sum())
    return worst, bad_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--copies", type=int, default=4, help="copies of the 100k store the searches rotate through")
    ap.add_argument("--shapes", default="100000:f32,1000000:bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "topk_sweep.json"))
    a = ap.parse_args()
    from rfx.index import DeviceIndex, synth_rows
    assert torch.cuda.is_available(), "bench_topk needs a GPU"
    torch.cuda.set_device(0)
    results = []
    for shape in a.shapes.split(","):
        rows, dtype = shape.split(":")
        rows = int(rows)
        esz = 4 if dtype == "f32" else 2
        copies = a.copies if rows * 768 * esz < (1 << 30) else 1
        ixs = []
        for c in range(copies):
            ix = DeviceIndex(768, dtype, 0)
            ix.add_synthetic(100 + c, rows)
            ixs.append(ix)
        iters = a.iters if rows <= 200_000 else max(a.iters // 4, 16)
        for nq in NQS:
            qs = [synth_rows(200 + i, 0, nq, 768, dtype, 0) for i in range(NQ_COPIES)]
            off = {}
            for ix in ixs:
                ix.enable_screen(0)
            for k in KS:
                assert all(ix.search_plan(nq, k) == 0 for ix in ixs)
                off[k] = time_case(ixs, qs, nq, k, iters, a.repeats, a.warmup)
            for ix in ixs:
                ix.enable_screen(1)
            for k in KS:
                plan = ixs[0].search_plan(nq, k)
                us_on, ans_on = time_case(ixs, qs, nq, k, iters, a.repeats, a.warmup)
                us_off, ans_off = off[k]
                worst, bad = compare(ans_on, ans_off)
                assert worst <= 1e-5 and bad == 0, (shape, nq, k, worst, bad)
                m_on, m_off = statistics.median(us_on), statistics.median(us_off)
                rec = {"rows": rows, "dim": 768, "dtype": dtype, "nq": nq, "k": k, "plan_screen_on": plan,
                       "us_screen_on": round(m_on, 2), "us_screen_off": round(m_off, 2),
                       "spread_on": round((max(us_on) - min(us_on)) / m_on, 4),
                       "spread_off": round((max(us_off) - min(us_off)) / m_off, 4),
                       "repeats_on_us": [round(u, 2) for u in us_on], "repeats_off_us": [round(u, 2) for u in us_off],
                       "max_score_diff": worst, "speedup": round(m_off / m_on, 3)}
                results.append(rec)
                print(f"{rows:>8} {dtype:>5} nq={nq} k={k:>2} plan={plan:>2}  on {m_on:8.1f} us (+-{rec['spread_on']:.1%})"
                      f"  off {m_off:8.1f} us (+-{rec['spread_off']:.1%})  x{rec['speedup']:.2f}", flush=True)
        for ix in ixs:
            ix.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_topk.py", "device": torch.cuda.get_device_name(0), "iters": a.iters,
                   "repeats": a.repeats, "copies_small_store": a.copies, "query_batches": NQ_COPIES,
                   "results": results}, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
