// deep_plan.h — host-only: validation and work split of the deep search (rfx_search_deep, rfx_deep_plan;
// kernels: k_deep.h).  Plain C++ (no HIP): the library includes it, and so can a stand-alone host program.
//
// Path: the retrieval slice of ask_stream (gemini_rag.py:517-551) at a depth of 65..1,024 rows per question —
// what a re-ranking stage, rank fusion at depth 100+ or recall@100 reads.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>

namespace rfx {

constexpr int kDeepMinK = 65, kDeepMaxK = 1024;
constexpr int64_t kDeepMaxNq = 1024;
constexpr int kDeepMaxDim = 1024;          // dim % 64 == 0 up to this
constexpr int kDeepThreads = 256;          // 4 waves
constexpr int kDeepRound = 64;             // rows of one round of a workgroup: 4 waves x one 16-row tile
constexpr int kDeepRangeAlign = 64;        // a range is a multiple of a round (the last one excepted)
constexpr int kDeepLdsBudget = 160 * 1024; // bytes of LDS a workgroup may use; the candidate buffers
                                           // (q_per_wg * 2 * KB * 8 B) take at most 128 KiB of it
constexpr int kDeepLdsBuffers = 128 * 1024;
constexpr int kDeepTargetWgs = 512;        // scan workgroups of a call (two per CU), ranges x question groups

struct DeepPlan {
  int ranges = 0;          // row ranges: range i = rows [i * rows_per_range, (i + 1) * rows_per_range), the LAST one
                           // runs to the end of the store (rows_per_range .. 2 * rows_per_range - 1 rows)
  int rows_per_range = 0;  // a multiple of kDeepRangeAlign, at least 4 * kb
  int kb = 0;              // k rounded up to 128 / 256 / 512 / 1024: entries a buffer keeps (it holds 2 * kb)
  int q_per_wg = 0;        // questions of a workgroup: 16, or 8 at kb 1024
  int q_groups = 0;        // ceil(nq / q_per_wg)
  int check_rounds = 0;    // rounds between two looks at the buffers' fill (scan kernel)
};

inline int deep_kb(int k) { return k <= 128 ? 128 : k <= 256 ? 256 : k <= 512 ? 512 : 1024; }

inline std::string deep_validate(int64_t rows, int dim, int64_t nq, int k) {
  if (k < kDeepMinK || k > kDeepMaxK)
    return "k=" + std::to_string(k) + " out of range [" + std::to_string(kDeepMinK) + ", " + std::to_string(kDeepMaxK) + "]";
  if (nq < 0 || nq > kDeepMaxNq) return "nq out of [0, " + std::to_string(kDeepMaxNq) + "]";
  if (rows < 0 || rows > 0x7fffffffll - 1) return "rows out of [0, 2^31 - 2]";
  if (dim < 1) return "dim < 1";
  return "";
}

// The split of a VALID call.  A range holds at least 4 * kb rows (so that the threshold has risen well before
// its end) unless the store is smaller than that: then one range, and the merge still runs.
inline DeepPlan deep_plan(int64_t rows, int64_t nq, int k) {
  DeepPlan p;
  p.kb = deep_kb(k);
  p.q_per_wg = p.kb == 1024 ? 8 : 16;
  p.q_groups = (int)std::max<int64_t>(1, (nq + p.q_per_wg - 1) / p.q_per_wg);
  const int64_t target = std::max<int64_t>(1, (kDeepTargetWgs + p.q_groups - 1) / p.q_groups);
  int64_t rpr = std::max<int64_t>(4 * (int64_t)p.kb, (rows + target - 1) / target);
  rpr = (rpr + kDeepRangeAlign - 1) / kDeepRangeAlign * kDeepRangeAlign;
  p.rows_per_range = (int)rpr;
  p.ranges = (int)std::max<int64_t>(1, rows / rpr);
  // a buffer of 2 * kb entries holds kb kept ones and what check_rounds rounds can append (64 each)
  p.check_rounds = std::min(4, p.kb / kDeepRound);
  return p;
}

inline size_t deep_ws_bytes(const DeepPlan& p, int64_t nq) {
  const size_t b = (size_t)std::max<int64_t>(nq, 1) * (size_t)p.ranges * (size_t)p.kb * 8;
  return (b + 255) / 256 * 256;
}

}  // namespace rfx
