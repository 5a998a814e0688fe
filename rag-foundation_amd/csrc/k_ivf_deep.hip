// k_ivf_deep.hip — the IVF deep search kernels (k_ivf_deep.h): the slab layout, and every probed row's key
// (k_cand_keys.h) into its question's slab.  The selection that follows: k_deep_select.h.  gfx950 only.
#include "k_ivf_deep.h"

#include "k_cand_keys.h"
#include "rfx_kernels.h"

namespace rfx {
namespace ivf {
namespace {

constexpr int kQB = 8;  // staged pairs of a batch, as in list_scan_kernel

// ---- slab layout -----------------------------------------------------------------------------------------------
// One wave per question, lane j = probe slot j: the exclusive prefix of the probed lists' lengths.
__global__ __launch_bounds__(256) void pair_base_kernel(const int64_t* __restrict__ pid, const int64_t* __restrict__ off,
                                                        int64_t nq, int nprobe, int* __restrict__ pair_base,
                                                        int* __restrict__ n_keys) {
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (q >= nq) return;  // (wave-uniform)
  int len = 0;
  if (lane < nprobe) {
    const int64_t L = pid[q * nprobe + lane];
    len = (int)(off[L + 1] - off[L]);
  }
  int incl = len;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(incl, d);
    if (lane >= d) incl += v;
  }
  if (lane < nprobe) pair_base[q * nprobe + lane] = incl - len;
  if (lane == 63) n_keys[q] = incl;
}

// ---- kernel A: scores of the probed lists ----------------------------------------------------------------------
// Eligibility, as list_scan_kernel's: EveryRow reads no mask; OneMask reads the store's row bitmap at the row id
// the lane holds (gid < rows <= 32 * mask words, checked by the caller; a past-the-end lane reads its list's
// first row and stores nothing).
enum class Elig { EveryRow, OneMask };

template <int NC, Elig E>
__global__ __launch_bounds__(256) void list_score_kernel(
    const int8_t* __restrict__ codes, const float* __restrict__ inv, const int* __restrict__ ids,
    const int64_t* __restrict__ off, const int* __restrict__ pair_off, const int* __restrict__ pairs, int nprobe,
    const int8_t* __restrict__ qq, const float* __restrict__ qinv, const int* __restrict__ pair_base, int64_t qcap,
    uint64_t* __restrict__ slab, const uint32_t* __restrict__ row_mask) {
  constexpr int D = NC * 256, NCH = D / 16;  // 16-B chunks per row
  constexpr int G = 4;                       // chunks per load group (double-buffered)
  static_assert(NCH % G == 0, "chunk groups");
  constexpr int NG = NCH / G;
  const int L = blockIdx.x, S = gridDim.y, sp = blockIdx.y;
  const int p0 = pair_off[L], p1 = pair_off[L + 1];
  if (p0 == p1) return;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t r0 = off[L], r1 = off[L + 1];
  for (int pb = p0; pb < p1; pb += kQB) {
    const int nb = min(kQB, p1 - pb);
    // the staged pairs: question codes, question scale and the pair's run of the slab (all wave-uniform)
    const uint4* qv[kQB];
    float qf[kQB];
    uint64_t* run[kQB];
#pragma unroll
    for (int qi = 0; qi < kQB; ++qi) {
      const int p = pairs[pb + (qi < nb ? qi : 0)];
      const int q = p / nprobe;
      qv[qi] = (const uint4*)(qq + (int64_t)q * D);
      qf[qi] = qinv[q];
      run[qi] = slab + (int64_t)q * qcap + pair_base[p];
    }
    // (the load loop of list_scan_kernel, restated: that kernel is measured code and shares nothing)
    for (int64_t base = r0 + (int64_t)(sp * 4 + w) * 64; base < r1; base += 256 * S) {
      const int64_t crow = base + lane;
      const bool valid = crow < r1;
      const int64_t cr = valid ? crow : r0;                              // in-list row (never past the list)
      const int8_t* rp = codes + (cr >> 6) * (64 * D) + (cr & 63) * 16;  // chunk c at rp + c * 1024
      int acc[kQB];
#pragma unroll
      for (int qi = 0; qi < kQB; ++qi) acc[qi] = 0;
      uint4 va[G], vb[G];
#pragma unroll
      for (int c = 0; c < G; ++c) va[c] = *(const uint4*)(rp + c * 1024);
#pragma unroll
      for (int cg = 0; cg < NG; ++cg) {
        uint4(&cur)[G] = (cg & 1) ? vb : va;
        uint4(&nxt)[G] = (cg & 1) ? va : vb;
        if (cg + 1 < NG) {
#pragma unroll
          for (int c = 0; c < G; ++c) nxt[c] = *(const uint4*)(rp + ((cg + 1) * G + c) * 1024);
        }
#pragma unroll
        for (int qi = 0; qi < kQB; ++qi) {
          if (qi < nb) {
#pragma unroll
            for (int c = 0; c < G; ++c) {
              const uint4 q = qv[qi][cg * G + c];
              acc[qi] = __builtin_amdgcn_sdot4((int)cur[c].x, (int)q.x, acc[qi], false);
              acc[qi] = __builtin_amdgcn_sdot4((int)cur[c].y, (int)q.y, acc[qi], false);
              acc[qi] = __builtin_amdgcn_sdot4((int)cur[c].z, (int)q.z, acc[qi], false);
              acc[qi] = __builtin_amdgcn_sdot4((int)cur[c].w, (int)q.w, acc[qi], false);
            }
          }
        }
      }
      const float ir = inv[cr];
      const int gid = ids[cr];
      bool ok = true;
      if constexpr (E == Elig::OneMask) ok = (row_mask[(uint32_t)gid >> 5] >> (gid & 31)) & 1u;
      const int64_t rel = crow - r0;  // < the list's rows: inside the pair's run
      if (valid) {
#pragma unroll
        for (int qi = 0; qi < kQB; ++qi)
          if (qi < nb)  // |dot| < 2^24: exact in f32; the two roundings of oracle/ivf.py search
            run[qi][rel] = ok ? cand_key(__fmul_rn((float)acc[qi], __fmul_rn(ir, qf[qi])), gid) : 0ull;
      }
    }
  }
}

template <Elig E>
int launch_score(int D, int m, int splits, hipStream_t st, const int8_t* codes, const float* inv, const int* ids,
                 const int64_t* off, const int* pair_off, const int* pairs, int nprobe, const int8_t* qq, const float* qinv,
                 const int* pair_base, int64_t qcap, uint64_t* slab, const uint32_t* row_mask) {
#define RFX_LSC(NCV)                                                                                                  \
  if (D == NCV * 256) {                                                                                               \
    hipLaunchKernelGGL((list_score_kernel<NCV, E>), dim3(m, splits), dim3(256), 0, st, codes, inv, ids, off, pair_off, \
                       pairs, nprobe, qq, qinv, pair_base, qcap, slab, row_mask);                                     \
    return 0;                                                                                                         \
  }
  RFX_LSC(1) RFX_LSC(2) RFX_LSC(3) RFX_LSC(4)
#undef RFX_LSC
  return -1;
}

}  // namespace

void launch_pair_base(const int64_t* pid, const int64_t* off, int64_t nq, int nprobe, int* pair_base, int* n_keys,
                      hipStream_t st) {
  if (nq <= 0) return;
  hipLaunchKernelGGL(pair_base_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, pid, off, nq, nprobe, pair_base,
                     n_keys);
}

int launch_list_score(int D, int m, int splits, const int8_t* codes, const float* inv, const int* ids, const int64_t* off,
                      const int* pair_off, const int* pairs, int nprobe, const int8_t* qq, const float* qinv,
                      const int* pair_base, int64_t qcap, uint64_t* slab, const uint32_t* row_mask, hipStream_t st) {
  if (nprobe < 1 || nprobe > kDeepMaxProbe || qcap < 2 || (qcap & 1)) return -1;
  return row_mask ? launch_score<Elig::OneMask>(D, m, splits, st, codes, inv, ids, off, pair_off, pairs, nprobe, qq, qinv,
                                                pair_base, qcap, slab, row_mask)
                  : launch_score<Elig::EveryRow>(D, m, splits, st, codes, inv, ids, off, pair_off, pairs, nprobe, qq, qinv,
                                                 pair_base, qcap, slab, row_mask);
}

}  // namespace ivf
}  // namespace rfx
