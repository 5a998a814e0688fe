// deep_sampled_plan.h — host-only: the plan of the sampled-threshold deep search (rfx_search_deep_sampled,
// rfx_deep_sampled_plan; kernels: k_deep_sampled.h; design: DESIGN §4.20).  Plain C++ (no HIP), like deep_plan.h,
// whose limits (deep_validate, KB = deep_kb(k)) it keeps.
//
// Path: the retrieval slice of ask_stream (gemini_rag.py:517-551) at a depth of 65..1,024 rows per question.
//
// A threshold that is fixed BEFORE the scan needs no buffers, sorts or barriers inside it: the k-th best score
// of a strided sample of the rows is a lower bound of the k-th best score of the store.  The scan then writes the
// few rows at or above it as keys into a per-question slab, and a selection afterwards picks the k best.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "deep_plan.h"

namespace rfx {

constexpr int kDsDenseFactor = 8;    // a store of at most 8 * KB rows writes every row's key: no sample
constexpr int kDsSampleFactor = 2;   // S = ceil(sqrt(2 * KB * rows)): the sample's keys and the expected passers
                                     // of the main pass (k * rows / S) are then of the same order
constexpr int kDsRound = 64;         // rows a workgroup stages at a time (4 tiles of 16)
constexpr int kDsTargetWgs = 512;    // scan workgroups of a pass: two per CU, whatever KB
constexpr int kDsNarrowQ = 16;       // questions of a workgroup for nq <= 16: 4 waves split the rows
// questions of a workgroup for nq > 64 at dim <= 768: 8 waves of 16 (one pass over the rows per 128 questions).
// Batches of 17..64 questions, and every batch above 16 at dim > 768 (the 8-wave form would spill), take 4 waves.
// (-DRFX_DS_WIDE_Q=64 builds the side library of a comparison.)
#ifndef RFX_DS_WIDE_Q
#define RFX_DS_WIDE_Q 128
#endif
constexpr int kDsWideQ = RFX_DS_WIDE_Q;
constexpr int kDsWideMaxDim = 768;
constexpr size_t kDsHeaderBytes = 256;  // int32[0] = questions that fell back

struct DeepSampledPlan {
  int dense = 0;           // 1: rows <= 8 * KB, one pass writes every row's key
  int S = 0;               // sample rows (0 when dense): rows i * stride, i < S
  int stride = 1;
  int cap = 0;             // keys a question's slab takes in the main pass; even
  int64_t slab = 0;        // keys of a question's slab: max(S, cap); even
  int kb = 0;
  int q_per_wg = 0;        // 16 (nq <= 16), 64 or 128
  int q_groups = 0;
  int ranges = 0;          // row ranges of the main pass, rows_per_range rows each (the last one shorter)
  int rows_per_range = 0;  // a multiple of 64
};

// n rows (or sample ordinals) over about kDsTargetWgs / q_groups ranges of equal length, a multiple of a round
inline void deep_sampled_split(int64_t n, int q_groups, int* per_range, int* ranges) {
  const int64_t want = std::max<int64_t>(1, kDsTargetWgs / std::max(1, q_groups));
  int64_t per = (std::max<int64_t>(n, 1) + want - 1) / want;
  per = (per + kDsRound - 1) / kDsRound * kDsRound;
  *per_range = (int)per;
  *ranges = (int)std::max<int64_t>(1, (n + per - 1) / per);
}

// The plan of a VALID call (deep_validate passed).
inline DeepSampledPlan deep_sampled_plan(int64_t rows, int dim, int64_t nq, int k) {
  DeepSampledPlan p;
  p.kb = deep_kb(k);
  if (rows <= (int64_t)kDsDenseFactor * p.kb) {
    p.dense = 1;
    p.cap = (int)((std::max<int64_t>(rows, 1) + 1) & ~(int64_t)1);
    p.slab = p.cap;
  } else {
    int64_t s = (int64_t)std::ceil(std::sqrt((double)kDsSampleFactor * p.kb * (double)rows));
    while (s * s < (int64_t)kDsSampleFactor * p.kb * rows) ++s;  // (the square root's rounding)
    s = (s + 15) / 16 * 16;
    p.S = (int)s;
    p.stride = (int)(rows / s);
    p.cap = (int)(kDsSampleFactor * (int64_t)p.kb * ((rows + s - 1) / s) + 64);
    p.slab = std::max<int64_t>(p.S, p.cap);
  }
  p.q_per_wg = nq <= kDsNarrowQ ? kDsNarrowQ : (nq <= 64 || dim > kDsWideMaxDim) ? 64 : kDsWideQ;
  p.q_groups = (int)std::max<int64_t>(1, (nq + p.q_per_wg - 1) / p.q_per_wg);
  deep_sampled_split(rows, p.q_groups, &p.rows_per_range, &p.ranges);
  return p;
}

// Workspace: header | count, n_keys, fell-back list [nq] i32, tau [nq] f32 | slabs | the selections' (score,
// row) pairs and the re-scored scores [nq][k] | the fallback's compact questions and outputs | the parent's.
struct DeepSampledWs {
  size_t count, n_keys, fb_list, tau, slab, sel_s, sel_r, rs_s, fb_q, fb_s, fb_r, parent, total;
};
inline DeepSampledWs deep_sampled_ws(const DeepSampledPlan& p, int64_t rows, int dim, int64_t nq, int k) {
  const size_t n = (size_t)std::max<int64_t>(nq, 1);
  size_t at = kDsHeaderBytes;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += (bytes + 255) / 256 * 256;
    return o;
  };
  DeepSampledWs w;
  w.count = take(n * 4);
  w.n_keys = take(n * 4);
  w.fb_list = take(n * 4);
  w.tau = take(n * 4);
  w.slab = take(n * (size_t)p.slab * 8);
  w.sel_s = take(n * k * 4);
  w.sel_r = take(n * k * 8);
  w.rs_s = take(n * k * 4);
  w.fb_q = take(n * (size_t)dim * 2);
  w.fb_s = take(n * k * 4);
  w.fb_r = take(n * k * 8);
  w.parent = take(deep_ws_bytes(deep_plan(rows, nq, k), nq));
  w.total = at;
  return w;
}
inline size_t deep_sampled_ws_bytes(const DeepSampledPlan& p, int64_t rows, int dim, int64_t nq, int k) {
  return deep_sampled_ws(p, rows, dim, nq, k).total;
}

}  // namespace rfx
