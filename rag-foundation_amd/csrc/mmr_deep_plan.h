// mmr_deep_plan.h — host-only: validation, slices and workspace layout of the deep MMR selection
// (rfx_mmr_select_deep; kernels: k_mmr_deep.h).  Plain C++ (no HIP): the library includes it, and so can a
// stand-alone host program.
//
// Path: the stage after the retrieval slice of ask_stream (gemini_rag.py:517-551) when it hands 65..1,024
// candidates on — the pool of a diversified answer, or the candidate set of a re-ranker.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>

namespace rfx {

constexpr int kMmrDeepMinCand = 65, kMmrDeepMaxCand = 1024;
constexpr int64_t kMmrDeepMaxNq = 1024;
constexpr int kMmrDeepMaxDim = 1024;      // dim % 64 == 0 up to this
constexpr int kMmrDeepTile = 64;          // a Gram workgroup's output tile is kMmrDeepTile x kMmrDeepTile
constexpr size_t kMmrDeepGramBudget = (size_t)512 << 20;  // bytes of similarity matrices alive at once

struct MmrDeepPlan {
  int n_pad = 0;      // n_cand_max rounded up to the tile: a question's matrix is [n_pad][n_pad] f32
  int tiles = 0;      // n_pad / kMmrDeepTile
  int pairs = 0;      // tile pairs (ti <= tj) of the upper triangle: the Gram grid's x
  int slice_q = 0;    // questions of one slice (Gram + select run once per slice)
  int slices = 0;     // ceil(nq / slice_q)
  // workspace offsets (bytes); stats sit at offset 0
  size_t lam = 0, ncand = 0, norm = 0, flag = 0, bits = 0, gram = 0, total = 0;
  size_t tables = 0;  // bytes staged from the host: the lambdas and the n_cand, back to back from `lam`
};

inline std::string mmr_deep_validate(int64_t nq, int n_cand_max, int k) {
  if (n_cand_max < kMmrDeepMinCand || n_cand_max > kMmrDeepMaxCand)
    return "n_cand_max=" + std::to_string(n_cand_max) + " out of range [" + std::to_string(kMmrDeepMinCand) + ", " +
           std::to_string(kMmrDeepMaxCand) + "]";
  if (k < 1 || k > n_cand_max) return "k=" + std::to_string(k) + " out of range [1, n_cand_max=" + std::to_string(n_cand_max) + "]";
  if (nq < 1 || nq > kMmrDeepMaxNq) return "nq out of [1, " + std::to_string(kMmrDeepMaxNq) + "]";
  return "";
}

// The plan of a VALID call.  The matrices of a slice stay at or under kMmrDeepGramBudget: 128 questions at
// n_pad 1,024, every question of the call at n_pad <= 256.
inline MmrDeepPlan mmr_deep_plan(int64_t nq, int n_cand_max) {
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  MmrDeepPlan p;
  p.n_pad = (n_cand_max + kMmrDeepTile - 1) / kMmrDeepTile * kMmrDeepTile;
  p.tiles = p.n_pad / kMmrDeepTile;
  p.pairs = p.tiles * (p.tiles + 1) / 2;
  const size_t mat = (size_t)p.n_pad * p.n_pad * sizeof(float);
  p.slice_q = (int)std::min<int64_t>(nq, (int64_t)(kMmrDeepGramBudget / mat));
  p.slices = (int)((nq + p.slice_q - 1) / p.slice_q);
  p.lam = up((size_t)nq * 2 * sizeof(int32_t));                 // after the stats: [nq][2] int32
  p.ncand = p.lam + (size_t)nq * sizeof(float);
  p.tables = (size_t)nq * (sizeof(float) + sizeof(int32_t));
  p.norm = up(p.ncand + (size_t)nq * sizeof(int32_t));
  p.flag = p.norm + up((size_t)p.slice_q * p.n_pad * sizeof(float));
  p.bits = p.flag + up((size_t)p.slice_q * p.n_pad);
  p.gram = p.bits + up((size_t)p.slice_q * p.n_pad * (p.n_pad / 8));
  p.total = p.gram + (size_t)p.slice_q * mat;
  return p;
}

}  // namespace rfx
