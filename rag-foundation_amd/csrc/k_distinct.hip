// k_distinct.hip — the collapse-by-document kernel and its launcher (see k_distinct.h).
#include "k_distinct.h"

#include "rfx_device.h"

namespace rfx {
namespace {

constexpr int kWavesPerBlock = kDistinctThreads / kWave;

__global__ __launch_bounds__(kDistinctThreads) void distinct_collapse_kernel(
    const int32_t* __restrict__ row_doc, int64_t rows, int nq, int n_cand, int k, const float* __restrict__ cand_s,
    const int64_t* __restrict__ cand_r, const int32_t* have, float* __restrict__ out_s, int64_t* __restrict__ out_r,
    int32_t* out_docs, int32_t* out_n, int32_t* __restrict__ out_done) {
  // (have may be out_n of the round before, and out_docs is read and written: neither is __restrict__)
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t q = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x / kWave);
  if (q >= nq) return;  // the whole wave leaves: the lanes of a wave share q

  // lane i holds candidate i
  float s = -__builtin_inff();
  long long r = -1;
  if (lane < n_cand) {
    s = cand_s[q * n_cand + lane];
    r = cand_r[q * n_cand + lane];
  }
  const bool valid = lane < n_cand && r >= 0 && r < rows;
  const int doc = valid ? row_doc[r] : -1;

  // the documents the earlier rounds found: lane i holds out_docs[q][i], i < have (read before any write below)
  int h = have ? have[q] : 0;
  h = h < 0 ? 0 : (h > k ? k : h);
  const int found = lane < h ? out_docs[q * k + lane] : -2;

  bool keep = doc >= 0;  // (an invalid lane holds -1)
  // every lane runs all 64 steps of both loops: the shuffles see a converged wave
  for (int j = 0; j < kWave; ++j) {
    const int dj = __shfl(doc, j);
    const int fj = __shfl(found, j);
    if (j < lane && dj == doc) keep = false;  // a better chunk of the same document (doc >= 0: lane j is valid)
    if (fj == doc) keep = false;              // found by an earlier round (found is -2 or >= 0, never -1)
  }

  const uint64_t surv = __ballot(keep);
  const uint64_t nvalid = __ballot(valid);
  const int pos = h + __builtin_popcountll(surv & ((1ull << lane) - 1ull));
  int n_new = h + __builtin_popcountll(surv);
  n_new = n_new > k ? k : n_new;
  if (keep && pos < k) {
    out_s[q * k + pos] = s;
    out_r[q * k + pos] = r;
    out_docs[q * k + pos] = doc;
  }
  for (int e = n_new + lane; e < k; e += kWave) {  // (k <= 64: one step)
    out_s[q * k + e] = -__builtin_inff();
    out_r[q * k + e] = -1;
    out_docs[q * k + e] = -1;
  }
  if (lane == 0) {
    out_n[q] = n_new;
    out_done[q] = (n_new >= k || __builtin_popcountll(nvalid) < n_cand) ? 1 : 0;
  }
}

}  // namespace

int launch_distinct_collapse(const int32_t* row_doc, int64_t rows, int nq, int n_cand, int k, const float* cand_s,
                             const int64_t* cand_r, const int32_t* have, float* out_s, int64_t* out_r,
                             int32_t* out_docs, int32_t* out_n, int32_t* out_done, hipStream_t st) {
  if (nq < 1 || nq > kDistinctMaxNq || n_cand < 1 || n_cand > kDistinctMaxCand || k < 1 || k > kDistinctMaxCand)
    return -1;
  if (rows < 0 || (rows > 0 && !row_doc)) return -1;
  if (!cand_s || !cand_r || !out_s || !out_r || !out_docs || !out_n || !out_done) return -1;
  const unsigned blocks = (unsigned)((nq + kWavesPerBlock - 1) / kWavesPerBlock);
  hipLaunchKernelGGL(distinct_collapse_kernel, dim3(blocks), dim3(kDistinctThreads), 0, st, row_doc, rows, nq, n_cand,
                     k, cand_s, cand_r, have, out_s, out_r, out_docs, out_n, out_done);
  return 0;
}

}  // namespace rfx
