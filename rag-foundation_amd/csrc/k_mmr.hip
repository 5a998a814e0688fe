// k_mmr.hip — the MMR selection kernel and its launcher (see k_mmr.h).
#include "k_mmr.h"

#include "../../include/rfx.h"
#include "rfx_device.h"

namespace rfx {
namespace {

template <int DT>
constexpr int mmr_esz() {
  return DT == RFX_F32 ? 4 : 2;
}

// does a 16-byte piece of a row hold a NaN?
template <int DT>
__device__ __forceinline__ bool piece_has_nan(const uint4& u) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
  bool bad = false;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (DT == RFX_F32) {
      bad |= (w[i] & 0x7fffffffu) > 0x7f800000u;
    } else {
      constexpr uint32_t inf = DT == RFX_BF16 ? 0x7f80u : 0x7c00u;
      bad |= (w[i] & 0x7fffu) > inf || ((w[i] >> 16) & 0x7fffu) > inf;
    }
  }
  return bad;
}

template <int DT>
__device__ __forceinline__ float half_to_f32(uint32_t h) {
  return DT == RFX_BF16 ? bf16_to_f32((uint16_t)h) : f16_to_f32((uint16_t)h);
}

// elements [8 * c8, 8 * c8 + 8) of the row at `row` (LDS or global), widened to f32
template <int DT, class P>
__device__ __forceinline__ void load8(P row, int c8, float (&e)[8]) {
  if constexpr (DT == RFX_F32) {
    const uint4 a = ((const uint4*)row)[2 * c8], b = ((const uint4*)row)[2 * c8 + 1];
    e[0] = __uint_as_float(a.x), e[1] = __uint_as_float(a.y), e[2] = __uint_as_float(a.z), e[3] = __uint_as_float(a.w);
    e[4] = __uint_as_float(b.x), e[5] = __uint_as_float(b.y), e[6] = __uint_as_float(b.z), e[7] = __uint_as_float(b.w);
  } else {
    const uint4 a = ((const uint4*)row)[c8];
    const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      e[2 * i] = half_to_f32<DT>(w[i] & 0xffffu);
      e[2 * i + 1] = half_to_f32<DT>(w[i] >> 16);
    }
  }
}

// obj = L * s - (1 - L) * m in f64, each operation rounded on its own
__device__ __forceinline__ double mmr_objective(double L, float s, float m) {
#pragma clang fp contract(off)
  const double rel = L * (double)s;
  const double pen = (1.0 - L) * (double)m;
  return rel - pen;
}

template <int DT, bool STAGED>
__global__ __launch_bounds__(kMmrThreads) void mmr_select_kernel(const uint8_t* __restrict__ X, int64_t nrows, int D,
                                                                 int n_max, int k, const float* __restrict__ lam,
                                                                 const int* __restrict__ ncand,
                                                                 const float* __restrict__ cand_s,
                                                                 const int64_t* __restrict__ cand_r,
                                                                 float* __restrict__ out_s, int64_t* __restrict__ out_r,
                                                                 float* __restrict__ out_obj) {
  extern __shared__ __attribute__((aligned(16))) uint8_t mmr_lds[];
  __shared__ long long s_row[kMmrMaxCand];  // the candidate's row, -1 = padding
  __shared__ float s_m[kMmrMaxCand];        // max similarity to the picked candidates
  __shared__ int s_bad[kMmrMaxCand];        // padding: row out of range, or a NaN in the row
  __shared__ int s_sel;
  constexpr int ESZ = mmr_esz<DT>();
  double* xj = (double*)mmr_lds;                   // [D] the last pick's row in f64
  uint8_t* staged = mmr_lds + (size_t)D * 8;       // STAGED: [n][D + kMmrRowPad] elements
  const int stride = (D + kMmrRowPad) * ESZ;       // bytes
  const int64_t row_bytes = (int64_t)D * ESZ;
  const int cpr = (int)(row_bytes / 16);           // 16-byte pieces per row
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  const int n = min(max(ncand[q], 0), min(n_max, kMmrMaxCand));
  const double L = (double)lam[q];

  // wave 0: lane i owns candidate i
  float my_s = -__builtin_inff();
  long long my_r = -1;
  if (tid < kMmrMaxCand) {
    if (tid < n) {
      my_s = cand_s[q * n_max + tid];
      my_r = cand_r[q * n_max + tid];
    }
    const bool in = tid < n && my_r >= 0 && my_r < nrows;
    s_row[tid] = in ? my_r : -1;
    s_bad[tid] = !in;
    s_m[tid] = -__builtin_inff();
  }
  __syncthreads();

  // gather: every 16-byte piece of every candidate row once (NaN check; staged rows to LDS), four loads in flight
  const int total = n * cpr;
  for (int v0 = tid; v0 < total; v0 += kMmrThreads * 4) {
    uint4 u[4];
    int ci[4], cc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int v = v0 + i * kMmrThreads;
      ci[i] = -1;
      if (v < total) {
        const int c = v / cpr;
        const long long row = s_row[c];
        if (row >= 0) {
          ci[i] = c;
          cc[i] = v - c * cpr;
          u[i] = ((const uint4*)(X + row * row_bytes))[cc[i]];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (ci[i] < 0) continue;
      if (piece_has_nan<DT>(u[i])) s_bad[ci[i]] = 1;  // (every writer stores the same value)
      if constexpr (STAGED) *(uint4*)(staged + (size_t)ci[i] * stride + (size_t)cc[i] * 16) = u[i];
    }
  }
  __syncthreads();

  bool avail = tid < n && !s_bad[tid < kMmrMaxCand ? tid : 0];
  // lanes per candidate of the similarity column: 256 / pow2(n), 4 (n > 32) .. 64 (n <= 4); a function of the
  // query's own n_cand alone, so its sums do not depend on the batch it rides in
  int G = 4;
  while (G < 64 && (kMmrThreads / (2 * G)) >= n) G *= 2;
  const int ci = tid / G, cp = tid - ci * G;
  const bool dot_on = ci < n && !s_bad[ci < kMmrMaxCand ? ci : 0];
  const long long dot_row = dot_on ? s_row[ci] : 0;

  int t = 0;
  for (; t < k; ++t) {
    if (tid < kWave) {  // wave 0 (uniform for the wave): pick
      double obj = L * (double)my_s;  // step 0 has no penalty; its pick is the first valid candidate
      int sel;
      const uint64_t av = __ballot(avail);
      if (t == 0) {
        sel = av ? __builtin_ctzll(av) : -1;
      } else {
        obj = mmr_objective(L, my_s, s_m[tid]);
        double best = avail ? obj : -__builtin_inf();
#pragma unroll
        for (int off = 32; off; off >>= 1) best = fmax(best, __shfl_xor(best, off));
        const uint64_t eq = __ballot(avail && obj == best);
        sel = eq ? __builtin_ctzll(eq) : (av ? __builtin_ctzll(av) : -1);  // ties: the lower position
      }
      if (tid == sel) {
        out_s[q * k + t] = my_s;
        out_r[q * k + t] = my_r;
        if (out_obj) out_obj[q * k + t] = (float)obj;
        avail = false;
      }
      if (tid == 0) s_sel = sel;
    }
    __syncthreads();
    const int sel = s_sel;
    if (sel < 0) break;        // no valid candidate left: the rest is padding
    if (t == k - 1) {
      ++t;
      break;
    }
    // the pick's row in f64
    if constexpr (STAGED) {
      const uint8_t* rj = staged + (size_t)sel * stride;
      for (int c8 = tid; c8 < D / 8; c8 += kMmrThreads) {
        float e[8];
        load8<DT>(rj, c8, e);
#pragma unroll
        for (int i = 0; i < 8; ++i) xj[8 * c8 + i] = (double)e[i];
      }
    } else {
      const uint8_t* rj = X + s_row[sel] * row_bytes;
      for (int c8 = tid; c8 < D / 8; c8 += kMmrThreads) {
        float e[8];
        load8<DT>(rj, c8, e);
#pragma unroll
        for (int i = 0; i < 8; ++i) xj[8 * c8 + i] = (double)e[i];
      }
    }
    __syncthreads();
    // the column sim(., sel): exact products (f32 x f32 fits f64), f64 sum, rounded to f32 once
    double acc = 0.0;
    if (dot_on) {
      for (int c8 = cp; c8 < D / 8; c8 += G) {
        float e[8];
        if constexpr (STAGED)
          load8<DT>((const uint8_t*)(staged + (size_t)ci * stride), c8, e);
        else
          load8<DT>(X + dot_row * row_bytes, c8, e);
        const double2* xp = (const double2*)(xj + 8 * c8);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double2 x2 = xp[i];
          acc = __builtin_fma((double)e[2 * i], x2.x, acc);
          acc = __builtin_fma((double)e[2 * i + 1], x2.y, acc);
        }
      }
    }
    for (int off = G >> 1; off; off >>= 1) acc += __shfl_xor(acc, off);
    if (dot_on && cp == 0) s_m[ci] = fmaxf(s_m[ci], (float)acc);
    __syncthreads();
  }
  // fewer than k valid candidates: (-inf, -1)
  for (int e = t + tid; e < k; e += kMmrThreads) {
    out_s[q * k + e] = -__builtin_inff();
    out_r[q * k + e] = -1;
    if (out_obj) out_obj[q * k + e] = -__builtin_inff();
  }
}

template <int DT, bool STAGED>
int launch_t(size_t lds, const void* X, int64_t nrows, int D, int64_t nq, int n_max, int k, const float* lam,
             const int* ncand, const float* cs, const int64_t* cr, float* out_s, int64_t* out_r, float* out_obj,
             hipStream_t st) {
  auto kern = mmr_select_kernel<DT, STAGED>;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return -1;
  hipLaunchKernelGGL(kern, dim3((unsigned)nq), dim3(kMmrThreads), lds, st, (const uint8_t*)X, nrows, D, n_max, k, lam,
                     ncand, cs, cr, out_s, out_r, out_obj);
  return 0;
}

}  // namespace

size_t mmr_lds_bytes(int D, int dtype, int n_cand_max, bool* staged) {
  const size_t xj = (size_t)D * 8;
  const size_t rows = dtype == RFX_F32 ? 0 : (size_t)n_cand_max * (D + kMmrRowPad) * 2;
  const bool st = rows > 0 && xj + rows <= kMmrLdsBudget;
  if (staged) *staged = st;
  return st ? xj + rows : xj;
}

int launch_mmr_select(const void* X, int64_t nrows, int D, int dtype, int64_t nq, int n_cand_max, int k,
                      const float* lam_d, const int* ncand_d, const float* cand_s, const int64_t* cand_r, float* out_s,
                      int64_t* out_r, float* out_obj, hipStream_t st) {
  if (nq < 1 || nq > kMmrMaxNq || n_cand_max < 1 || n_cand_max > kMmrMaxCand || k < 1 || k > n_cand_max) return -1;
  if (D <= 0 || D % 64 != 0 || (size_t)D * 8 > kMmrLdsBudget || nrows < 0 || (nrows > 0 && !X)) return -1;
  if (!lam_d || !ncand_d || !cand_s || !cand_r || !out_s || !out_r) return -1;
  bool staged = false;
  const size_t lds = mmr_lds_bytes(D, dtype, n_cand_max, &staged);
#define RFX_MMR_ARGS lds, X, nrows, D, nq, n_cand_max, k, lam_d, ncand_d, cand_s, cand_r, out_s, out_r, out_obj, st
  switch (dtype) {
    case RFX_F32: return launch_t<RFX_F32, false>(RFX_MMR_ARGS);
    case RFX_BF16: return staged ? launch_t<RFX_BF16, true>(RFX_MMR_ARGS) : launch_t<RFX_BF16, false>(RFX_MMR_ARGS);
    case RFX_F16: return staged ? launch_t<RFX_F16, true>(RFX_MMR_ARGS) : launch_t<RFX_F16, false>(RFX_MMR_ARGS);
  }
#undef RFX_MMR_ARGS
  return -1;
}

}  // namespace rfx
