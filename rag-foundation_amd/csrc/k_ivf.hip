// k_ivf.hip — IVF-Flat int8 (build plan item 8): clustered synthetic rows,
// int8 quantisation, MFMA i8 coarse scoring (k-means assignment and probe selection), k-means
// update, posting-list build, probe selection, pair grouping and the re-rank (the posting-list scan: k_ivf_scan.hip).
//
// Numerics are exact by construction (oracle/ivf.py restates them and the GPU is held to it
// bit-for-bit): int8 x int8 dot products accumulate in int32 (|dot| <= 768·127² < 2^24, so the
// f32 conversion is exact too), and every floating-point step is ONE correctly rounded IEEE op
// (__fdiv_rn / __fmul_rn / __fsqrt_rn, rintf) that numpy's float32 performs identically.
#include <rocprim/device/device_radix_sort.hpp>

#include "rfx_device.h"
#include "rfx_kernels.h"

namespace rfx {
namespace ivf {

typedef __attribute__((ext_vector_type(4))) int v4i;
typedef __attribute__((ext_vector_type(16))) int v16i;

constexpr uint64_t kCentreKey = 1ull << 63;  // generator key spaces (oracle/ivf.py C_KEY, L_KEY)
constexpr uint64_t kLabelKey = 1ull << 62;

// KERNEL<DT> for a runtime dtype, in 256-thread blocks (the kernels take one wave per row)
#define RFX_LAUNCH_DT(KERNEL, dtype, blocks, st, ...) do {                                                        \
    if (dtype == RFX_F32) hipLaunchKernelGGL(KERNEL<RFX_F32>, dim3(blocks), dim3(256), 0, st, __VA_ARGS__);       \
    else if (dtype == RFX_BF16) hipLaunchKernelGGL(KERNEL<RFX_BF16>, dim3(blocks), dim3(256), 0, st, __VA_ARGS__); \
    else hipLaunchKernelGGL(KERNEL<RFX_F16>, dim3(blocks), dim3(256), 0, st, __VA_ARGS__);                        \
  } while (0)

// ---- clustered synthetic rows: centre(cluster(r)) + noise(r), normalised exactly ---------------
template <int DT>
__global__ __launch_bounds__(256) void synth_clustered_kernel(uint64_t bc, uint64_t bn, uint64_t ncenters,
                                                              int64_t row0, int64_t n, int dim,
                                                              void* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nwaves) {
    const uint64_t r = (uint64_t)(row0 + i);
    const uint64_t lab = (splitmix64(bn + kLabelKey + r) >> 32) % ncenters;
    const uint64_t ck = kCentreKey + lab * (uint64_t)dim, nk = r * (uint64_t)dim;
    long long ss = 0;
    for (int c = lane; c < dim; c += 64) {
      const long long v = (long long)synth_raw(bc, ck + c) + synth_raw(bn, nk + c);
      ss += v * v;
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) ss += __shfl_xor(ss, off);
    const double rs = ss > 0 ? 1.0 / sqrt((double)ss) : 0.0;
    for (int c = lane; c < dim; c += 64) {
      const long long v = (long long)synth_raw(bc, ck + c) + synth_raw(bn, nk + c);
      const float x = (float)((double)v * rs);
      if constexpr (DT == RFX_F32)
        ((float*)out)[i * dim + c] = x;
      else if constexpr (DT == RFX_BF16)
        ((uint16_t*)out)[i * dim + c] = f32_to_bf16(x);
      else
        ((uint16_t*)out)[i * dim + c] = f32_to_f16(x);
    }
  }
}

void launch_synth_clustered(uint64_t cseed, uint64_t ncenters, uint64_t seed, int64_t row0, int64_t n, int dim,
                            int dtype, void* out, hipStream_t st) {
  const uint64_t bc = splitmix64(cseed), bn = splitmix64(seed);
  const int blocks = (int)std::min<int64_t>((std::max<int64_t>(n, 1) + 3) / 4, 8192);
  RFX_LAUNCH_DT(synth_clustered_kernel, dtype, blocks, st, bc, bn, ncenters, row0, n, dim, out);
}

// ---- int8 quantisation (one wave per row) --------------------------------------------------------
template <int DT>
__device__ __forceinline__ float load_elem(const void* X, int64_t i) {
  if constexpr (DT == RFX_F32)
    return ((const float*)X)[i];
  else if constexpr (DT == RFX_BF16)
    return bf16_to_f32(((const uint16_t*)X)[i]);
  else
    return f16_to_f32(((const uint16_t*)X)[i]);
}

template <int DT>
__global__ __launch_bounds__(256) void quantize_kernel(const void* __restrict__ X, int64_t n, int dim,
                                                       int8_t* __restrict__ codes, float* __restrict__ inv) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nwaves) {
    float amax = 0.f;
    for (int c = lane; c < dim; c += 64) amax = fmaxf(amax, fabsf(load_elem<DT>(X, i * dim + c)));
#pragma unroll
    for (int off = 32; off; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
    // sub-scale rule (oracle/ivf.py): 127 / amax = inf (amax < 127 / FLT_MAX) makes a zero row, codes 0 and
    // inv 0 — the row's zero elements would be 0 * inf = NaN, clamped to -127
    const float s0 = amax > 0.f ? __fdiv_rn(127.f, amax) : 0.f;
    const bool sub = s0 == __builtin_inff();
    const float s = sub ? 0.f : s0;
    for (int c = lane; c < dim; c += 64) {
      const float q = rintf(__fmul_rn(load_elem<DT>(X, i * dim + c), s));
      codes[i * dim + c] = (int8_t)fminf(fmaxf(q, -127.f), 127.f);
    }
    if (lane == 0) inv[i] = sub ? 0.f : __fdiv_rn(amax, 127.f);
  }
}

void launch_quantize(const void* X, int64_t n, int dim, int dtype, int8_t* codes, float* inv, hipStream_t st) {
  const int blocks = (int)std::min<int64_t>((std::max<int64_t>(n, 1) + 3) / 4, 8192);
  RFX_LAUNCH_DT(quantize_kernel, dtype, blocks, st, X, n, dim, codes, inv);
}

// ---- coarse scoring: MFMA i8 (v_mfma_i32_32x32x32_i8) -------------------------------------------
// Block: 128 rows of X (queries / rows to assign) resident in LDS, the centroid table streamed in
// 128-centroid × 64-byte chunks (double-buffered).  4 waves in a 2×2 grid, each 64 centroids ×
// 64 X rows = 2×2 MFMA tiles.  A operand = centroids (accumulator rows), B = X rows (accumulator
// columns = lanes), so a lane holds 16 centroids of ONE X row: the argmax is in-lane.
// LDS images are XOR-swizzled by 16-byte chunk: X row r chunk c at c ^ (r & xs_mask); centroid
// row r (64 B) chunk c at c ^ ((r >> 2) & 3): the 32-row fragment reads hit distinct banks.
constexpr int kXT = 128, kCT = 128, kKC = 64, kMaxD = 1024;
constexpr int kXBytes = kXT * kMaxD, kCBytes = kCT * kKC;

__device__ __forceinline__ v16i mfma_i8(const uint4& a, const uint4& b, const v16i& c) {
  v4i av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w}, bv = {(int)b.x, (int)b.y, (int)b.z, (int)b.w};
  return __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, c, 0, 0, 0);
}

// MODE 0: write scores S[x][c] = f32(dot) * fc[c] and ids[x][c] = c (probe selection: the merge
// kernel then takes the top nprobe per row); grid.y splits the centroids.
// MODE 1: labels[x] = argmax_c (f32(dot) * fc[c]), ties -> lowest c (k-means / list assignment).
template <int MODE>
__global__ __launch_bounds__(256, 1) void coarse_kernel(const int8_t* __restrict__ X, int64_t n,
                                                        const int8_t* __restrict__ C, int m, int D,
                                                        const float* __restrict__ fc, int ctiles_per_block,
                                                        float* __restrict__ out_s, int* __restrict__ out_i) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kXBytes + 2 * kCBytes];
  uint8_t* const xs = lds;
  uint8_t* const cs = lds + kXBytes;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int h = lane >> 5, l32 = lane & 31;
  const int wm = w & 1, wn = w >> 1;
  const int64_t x0 = (int64_t)blockIdx.x * kXT;
  const int nch = D >> 4;  // 16-byte chunks per X row
  const int xs_mask = min(15, (nch & -nch) - 1);
  const int ctiles = (m + kCT - 1) / kCT;
  const int ct0 = blockIdx.y * ctiles_per_block;
  const int ct1 = min(ctiles, ct0 + ctiles_per_block);
  const int nk = D / kKC;
  const int T = (ct1 - ct0) * nk;
  if (T <= 0) return;

  // resident X tile
  for (int i = tid; i < kXT * nch; i += 256) {
    const int r = i / nch, c = i - r * nch;
    const int64_t xr = min(x0 + r, n - 1);
    const uint4 v = *(const uint4*)(X + xr * D + c * 16);
    *(uint4*)(xs + r * D + (((c & ~xs_mask) | ((c ^ r) & xs_mask)) << 4)) = v;
  }
  auto load_c = [&](int t, uint4 (&v)[2]) {
    const int ct = ct0 + t / nk, kc = t - (t / nk) * nk;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = tid + 256 * u, r = i >> 2, c = i & 3;
      const int cr = ct * kCT + r;
      v[u] = cr < m ? *(const uint4*)(C + (int64_t)cr * D + kc * kKC + c * 16) : uint4{0u, 0u, 0u, 0u};
    }
  };
  auto store_c = [&](int buf, const uint4 (&v)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = tid + 256 * u, r = i >> 2, c = i & 3;
      *(uint4*)(cs + buf * kCBytes + r * kKC + ((c ^ ((r >> 2) & 3)) << 4)) = v[u];
    }
  };
  {
    uint4 v[2];
    load_c(0, v);
    store_c(0, v);
  }
  __syncthreads();

  v16i acc[2][2];
  float bs[2] = {-__builtin_inff(), -__builtin_inff()};
  int bc[2] = {0x7fffffff, 0x7fffffff};
  for (int t = 0; t < T; ++t) {
    const int kc = t % nk;
    if (kc == 0) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = v16i{};
    }
    uint4 nv[2];
    if (t + 1 < T) load_c(t + 1, nv);
    const uint8_t* cb = cs + (t & 1) * kCBytes;
#pragma unroll
    for (int s = 0; s < 2; ++s) {  // two 32-deep k-steps per 64-byte chunk
      const int cc = 2 * s + h;
      uint4 a[2], b[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const int r = wm * 64 + mi * 32 + l32;
        a[mi] = *(const uint4*)(cb + r * kKC + ((cc ^ ((r >> 2) & 3)) << 4));
      }
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int r = wn * 64 + ni * 32 + l32;
        const int c = kc * 4 + cc;
        b[ni] = *(const uint4*)(xs + r * D + (((c & ~xs_mask) | ((c ^ r) & xs_mask)) << 4));
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          // MODE 0: X rows as accumulator rows, centroids as lanes, so the score rows go out in 128-B runs
          if constexpr (MODE == 0)
            acc[mi][ni] = mfma_i8(b[ni], a[mi], acc[mi][ni]);
          else
            acc[mi][ni] = mfma_i8(a[mi], b[ni], acc[mi][ni]);
        }
    }
    if (t + 1 < T) store_c((t + 1) & 1, nv);
    if (MODE == 0 && kc == nk - 1) {
      // round 6: lane l32 holds centroid cbase + 32 mi + l32 for 16 X rows, so each store of a row's scores
      // is 32 consecutive floats (before: a lane per X row, 16-KB strides between lanes; 43.7 us per batch)
      const int cbase = (ct0 + t / nk) * kCT + wm * 64;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const int c = cbase + mi * 32 + l32;
        const bool cok = c < m;
        const float fcc = cok ? fc[c] : 0.f;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int64_t x = x0 + wn * 64 + ni * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (cok && x < n) {
              out_s[x * m + c] = __fmul_rn((float)acc[mi][ni][r], fcc);
              out_i[x * m + c] = c;
            }
          }
      }
    }
    if (MODE == 1 && kc == nk - 1) {
      const int cbase = (ct0 + t / nk) * kCT + wm * 64;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int64_t x = x0 + wn * 64 + ni * 32 + l32;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int c = cbase + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (c < m) {
              const float f = __fmul_rn((float)acc[mi][ni][r], fc[c]);
              if (f > bs[ni] || (f == bs[ni] && c < bc[ni])) {
                bs[ni] = f;
                bc[ni] = c;
              }
            }
          }
      }
    }
    __syncthreads();
  }
  if constexpr (MODE == 1) {
    // combine the two lane halves (disjoint centroid rows), then the two centroid-half waves
    float* rs = (float*)cs;      // [2 wn][64] scores
    int* ri = (int*)(cs + 512);  // [2 wn][64] ids
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const float os = __shfl_xor(bs[ni], 32);
      const int oc = __shfl_xor(bc[ni], 32);
      if (os > bs[ni] || (os == bs[ni] && oc < bc[ni])) {
        bs[ni] = os;
        bc[ni] = oc;
      }
      if (wm == 1 && h == 0) {
        rs[wn * 64 + ni * 32 + l32] = bs[ni];
        ri[wn * 64 + ni * 32 + l32] = bc[ni];
      }
    }
    __syncthreads();
    if (wm == 0 && h == 0) {
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const float os = rs[wn * 64 + ni * 32 + l32];
        const int oc = ri[wn * 64 + ni * 32 + l32];
        if (os > bs[ni] || (os == bs[ni] && oc < bc[ni])) {
          bs[ni] = os;
          bc[ni] = oc;
        }
        const int64_t x = x0 + wn * 64 + ni * 32 + l32;
        if (x < n) {
          out_i[x] = bc[ni];
          if (out_s) out_s[x] = bs[ni];
        }
      }
    }
  }
}

int launch_coarse_scores(const int8_t* X, int64_t n, const int8_t* C, int m, int D, const float* fc, float* S,
                         int* ids, hipStream_t st) {
  if (D % kKC || D > kMaxD || n <= 0 || m <= 0) return -1;
  const int64_t xb = (n + kXT - 1) / kXT;
  const int ctiles = (m + kCT - 1) / kCT;
  // spread the (few) query tiles over the chip: ~512 blocks
  const int splits = (int)std::max<int64_t>(1, std::min<int64_t>(ctiles, 512 / std::max<int64_t>(xb, 1)));
  const int per = (ctiles + splits - 1) / splits;
  dim3 grid((unsigned)xb, (unsigned)((ctiles + per - 1) / per));
  hipLaunchKernelGGL(coarse_kernel<0>, grid, dim3(256), 0, st, X, n, C, m, D, fc, per, S, ids);
  return 0;
}

int launch_assign(const int8_t* X, int64_t n, const int8_t* C, int m, int D, const float* fc, int* labels,
                  float* best, hipStream_t st) {
  if (D % kKC || D > kMaxD || n <= 0 || m <= 0) return -1;
  const int64_t xb = (n + kXT - 1) / kXT;
  if (xb > 0x7fffffff) return -1;
  const int ctiles = (m + kCT - 1) / kCT;
  hipLaunchKernelGGL(coarse_kernel<1>, dim3((unsigned)xb, 1), dim3(256), 0, st, X, n, C, m, D, fc, ctiles, best,
                     labels);
  return 0;
}

// ---- k-means update -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kmeans_accum_kernel(const int8_t* __restrict__ X, int64_t n, int D,
                                                           const int* __restrict__ labels,
                                                           int* __restrict__ sums, int* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nwaves) {
    const int l = labels[i];
    for (int c = lane; c < D; c += 64) atomicAdd(sums + (int64_t)l * D + c, (int)X[i * D + c]);
    if (lane == 0) atomicAdd(counts + l, 1);
  }
}

// f_c = RN(1 / RN(sqrt(x))) for an integer-valued float 0 < x < 2^24, exactly as numpy's IEEE
// float32 computes it.  The device sqrtf / reciprocal are not relied on for the last bit (a 1-ulp
// difference was measured on the k-means path): each step is fixed against the midpoints to its
// float neighbours, with products that are exact in f64 (<= 50 significant bits).
__device__ __forceinline__ float f32_up(float v) { return __uint_as_float(__float_as_uint(v) + 1u); }
__device__ __forceinline__ float f32_dn(float v) { return __uint_as_float(__float_as_uint(v) - 1u); }
__device__ __forceinline__ float cr_inv_sqrt_int(float x) {
  float y = (float)sqrt((double)x);
#pragma unroll
  for (int it = 0; it < 2; ++it) {  // y = RN(sqrt(x)): no midpoint squares to an integer, no ties
    const double mu = 0.5 * ((double)y + (double)f32_up(y)), md = 0.5 * ((double)y + (double)f32_dn(y));
    if ((double)x > mu * mu)
      y = f32_up(y);
    else if ((double)x < md * md)
      y = f32_dn(y);
  }
  float r = (float)(1.0 / (double)y);
#pragma unroll
  for (int it = 0; it < 2; ++it) {  // r = RN(1 / y): compare 1 with midpoint * y (exact in f64)
    const double pu = 0.5 * ((double)r + (double)f32_up(r)) * (double)y;
    const double pd = 0.5 * ((double)r + (double)f32_dn(r)) * (double)y;
    if (pu < 1.0 || (pu == 1.0 && (__float_as_uint(r) & 1u)))
      r = f32_up(r);
    else if (pd > 1.0 || (pd == 1.0 && (__float_as_uint(r) & 1u)))
      r = f32_dn(r);
  }
  return r;
}

// qc_c = clamp(rint(f32(sum) * (127 / f32(amax))), ±127) where the cluster is non-empty and
// amax > 0 (else unchanged); then f_c = 1 / sqrt(f32(sum qc²)).  One wave per centroid.
__global__ __launch_bounds__(256) void centroid_update_kernel(const int* __restrict__ sums,
                                                              const int* __restrict__ counts, int m, int D,
                                                              int8_t* __restrict__ qc, float* __restrict__ fc) {
  const int lane = threadIdx.x & 63;
  const int c = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (c >= m) return;
  if (sums) {
    int amax = 0;
    for (int d = lane; d < D; d += 64) amax = max(amax, abs(sums[(int64_t)c * D + d]));
#pragma unroll
    for (int off = 32; off; off >>= 1) amax = max(amax, __shfl_xor(amax, off));
    if (counts[c] > 0 && amax > 0) {
      const float sc = __fdiv_rn(127.f, (float)amax);
      for (int d = lane; d < D; d += 64) {
        const float q = rintf(__fmul_rn((float)sums[(int64_t)c * D + d], sc));
        qc[(int64_t)c * D + d] = (int8_t)fminf(fmaxf(q, -127.f), 127.f);
      }
    }
  }
  int n2 = 0;
  for (int d = lane; d < D; d += 64) {
    const int v = qc[(int64_t)c * D + d];
    n2 += v * v;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) n2 += __shfl_xor(n2, off);
  if (lane == 0) fc[c] = n2 > 0 ? cr_inv_sqrt_int((float)n2) : 0.f;
}

// initial centroids: qc_j = codes row j * step
__global__ void init_centroids_kernel(const int8_t* __restrict__ codes, int64_t step, int m, int D,
                                      int8_t* __restrict__ qc) {
  const int64_t total = (int64_t)m * (D >> 4);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = i / (D >> 4), c = i - j * (D >> 4);
    *(uint4*)(qc + j * D + c * 16) = *(const uint4*)(codes + j * step * D + c * 16);
  }
}

void launch_init_centroids(const int8_t* codes, int64_t step, int m, int D, int8_t* qc, hipStream_t st) {
  const int64_t total = (int64_t)m * (D >> 4);
  hipLaunchKernelGGL(init_centroids_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), dim3(256), 0,
                     st, codes, step, m, D, qc);
}

void launch_kmeans_accum(const int8_t* X, int64_t n, int D, const int* labels, int* sums, int* counts,
                         hipStream_t st) {
  const int blocks = (int)std::min<int64_t>((std::max<int64_t>(n, 1) + 3) / 4, 8192);
  hipLaunchKernelGGL(kmeans_accum_kernel, dim3(blocks), dim3(256), 0, st, X, n, D, labels, sums, counts);
}

void launch_centroid_update(const int* sums, const int* counts, int m, int D, int8_t* qc, float* fc, hipStream_t st) {
  hipLaunchKernelGGL(centroid_update_kernel, dim3((m + 3) / 4), dim3(256), 0, st, sums, counts, m, D, qc, fc);
}

// ---- posting lists ---------------------------------------------------------------------------------
__global__ void iota_kernel(int* __restrict__ v, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    v[i] = (int)i;
}

__global__ void histogram_kernel(const int* __restrict__ labels, int64_t n, int* __restrict__ counts) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    atomicAdd(counts + labels[i], 1);
}

// Exclusive scan of cnt[0..m) by one 1024-thread block: thread t owns the entries [b, e) and gets the sum of
// every entry before b; afterwards part[1023] is the total.
template <class T>
__device__ __forceinline__ T block_scan_1024(const int* cnt, int m, T* part, int& b, int& e) {
  const int t = threadIdx.x, per = (m + 1023) / 1024;
  b = t * per, e = min(m, b + per);
  T s = 0;
  for (int i = b; i < e; ++i) s += cnt[i];
  part[t] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const T v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  return part[t] - s;
}

// offsets[0..m] = exclusive scan of counts (one block)
__global__ __launch_bounds__(1024) void offsets_kernel(const int* __restrict__ counts, int m, int64_t* __restrict__ off) {
  __shared__ int64_t part[1024];
  int b, e;
  int64_t run = block_scan_1024(counts, m, part, b, e);
  for (int i = b; i < e; ++i) {
    off[i] = run;
    run += counts[i];
  }
  if (threadIdx.x == 1023) off[m] = part[1023];
}

// list-order copy of codes and scales: dst row p = src row ids[p] (one wave per row).  Round 6: the
// list-order codes are stored in 64-row blocks, chunk-major: 16-B chunk c of row p at
// (p / 64) * 64 D + c * 1024 + (p % 64) * 16, so the list scan's lane-per-row loads are 1-KB runs
// (kBlockRows rows of one chunk) and every lane holds a whole row's dot (list_scan_kernel).
__global__ __launch_bounds__(256) void gather_rows_kernel(const int8_t* __restrict__ codes,
                                                          const float* __restrict__ inv,
                                                          const int* __restrict__ ids, int64_t n, int D,
                                                          int8_t* __restrict__ dcodes, float* __restrict__ dinv) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int nch = D >> 4;
  for (int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; p < n; p += nwaves) {
    const int64_t src = ids[p];
    for (int c = lane; c < nch; c += 64)
      *(uint4*)(dcodes + (p >> 6) * 64 * D + c * 1024 + (p & 63) * 16) = *(const uint4*)(codes + src * D + c * 16);
    if (lane == 0) dinv[p] = inv[src];
  }
}

size_t sort_temp_bytes(int64_t n) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_pairs((void*)nullptr, bytes, (const unsigned*)nullptr, (unsigned*)nullptr,
                            (const int*)nullptr, (int*)nullptr, (size_t)n, 0u, 32u);
  return bytes;
}

// ids sorted by (label, row): stable LSD radix sort of (label, row id) pairs
int launch_build_lists(const int* labels, int64_t n, int m, const int8_t* codes, const float* inv, int D,
                       unsigned* keys_tmp, int* vals_tmp, unsigned* keys_out, int* ids_out, void* sort_tmp,
                       size_t sort_tmp_bytes, int* counts, int64_t* off, int8_t* dcodes, float* dinv,
                       hipStream_t st) {
  if (hipMemsetAsync(counts, 0, (size_t)m * sizeof(int), st) != hipSuccess) return -2;
  if (n > 0) {
    const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(histogram_kernel, dim3(blocks), dim3(256), 0, st, labels, n, counts);
    hipLaunchKernelGGL(iota_kernel, dim3(blocks), dim3(256), 0, st, vals_tmp, n);
    if (hipMemcpyAsync(keys_tmp, labels, (size_t)n * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return -2;
    unsigned end_bit = 1;
    while ((1u << end_bit) < (unsigned)m) ++end_bit;
    size_t tb = sort_tmp_bytes;
    if (rocprim::radix_sort_pairs(sort_tmp, tb, (const unsigned*)keys_tmp, keys_out, (const int*)vals_tmp, ids_out,
                                  (size_t)n, 0u, end_bit, st) != hipSuccess)
      return -3;
  }
  hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(1024), 0, st, counts, m, off);
  if (n > 0) {
    const int blocks = (int)std::min<int64_t>((n + 3) / 4, 8192);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks), dim3(256), 0, st, codes, inv, ids_out, n, D, dcodes, dinv);
  }
  return 0;
}

// ---- search: (query, probe) pairs grouped by list ---------------------------------------------------
// pair p = q * nprobe + j probes list probes[p]; out: pair_off[0..m] (CSR by list), pairs[].
// SKIP (a probe count per question): probes[p] < 0 marks a slot j >= nprobe_of[q]; such a pair is
// in no list.  SKIP = false is the code it was.
constexpr int kMaxListsGroup = 16384;
template <bool SKIP>
__global__ __launch_bounds__(1024) void group_pairs_kernel(const int64_t* __restrict__ probes, int P, int m,
                                                           int* __restrict__ pair_off, int* __restrict__ pairs) {
  __shared__ int cnt[kMaxListsGroup];
  __shared__ int part[1024];
  const int t = threadIdx.x;
  for (int i = t; i < m; i += 1024) cnt[i] = 0;
  __syncthreads();
  for (int p = t; p < P; p += 1024) {
    if constexpr (SKIP) {
      if (probes[p] < 0) continue;
    }
    atomicAdd(&cnt[(int)probes[p]], 1);
  }
  __syncthreads();
  int b, e;
  int run = block_scan_1024(cnt, m, part, b, e);
  for (int i = b; i < e; ++i) {
    const int c = cnt[i];
    pair_off[i] = run;
    cnt[i] = run;  // becomes the list's cursor
    run += c;
  }
  if (t == 1023) pair_off[m] = part[1023];
  __syncthreads();
  for (int p = t; p < P; p += 1024) {
    if constexpr (SKIP) {
      if (probes[p] < 0) continue;
    }
    pairs[atomicAdd(&cnt[(int)probes[p]], 1)] = p;
  }
}

// ---- probe selection: each query's nprobe best coarse scores (round 6) ----------------------------
// One 256-thread block per query, up to kProbeMaxLists scores held in registers (16 per thread, list
// c = tid + 256 i).  v = the nprobe-th largest orderable score by a bitwise search on block-wide ballot
// counts; ties at v are taken by the smallest list ids (a second bitwise search over the tied ids): the
// set the merge kernel's (score desc, id asc) top-nprobe returns.  The probes are written in no particular
// order (the pairs are grouped by list next, and every later step is order-free).  A coarse score is never -0.0
// (f32(dot) * f_c: f_c is 0 only for an all-zero centroid, whose dot is 0, and otherwise >= 1 / (127 * 32), far
// from underflow), so ord_f32's order is the float order here, unlike in seed_lists.
// PERQ: question q selects exactly its own nprobe_of[q] best (the writes are in no order, so the
// first n of a wider selection could not stand in); nprobe stays the stride of ps / pid.  The slots past the
// count are marked by absent_pairs_kernel.  PERQ = false never reads nprobe_of.
constexpr int kProbeMaxLists = 4096;
template <bool PERQ>
__global__ __launch_bounds__(256) void probe_select_kernel(const float* __restrict__ S, int m, int nprobe,
                                                           float* __restrict__ ps, int64_t* __restrict__ pid,
                                                           const int* __restrict__ nprobe_of) {
  constexpr int PT = kProbeMaxLists / 256;
  __shared__ int wc[2][4];
  __shared__ int npos;
  const int tid = threadIdx.x, w = tid >> 6;
  const int64_t q = blockIdx.x;
  const int stride = nprobe;
  if constexpr (PERQ) nprobe = nprobe_of[q];
  uint32_t key[PT];
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    const int c = tid + 256 * i;
    key[i] = c < m ? ord_f32(S[q * m + c]) : 0u;
  }
  if (tid == 0) npos = 0;
  // block-wide count of the keys meeting pred (two LDS slots alternate, so one barrier per count)
  int par = 0;
  auto block_count = [&](auto pred) {
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < PT; ++i) cnt += (int)__popcll(__ballot(pred(i)));
    if ((tid & 63) == 0) wc[par][w] = cnt;
    __syncthreads();
    const int t = wc[par][0] + wc[par][1] + wc[par][2] + wc[par][3];
    par ^= 1;
    return t;
  };
  uint32_t v = 0u;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t c1 = v | (1u << bit);
    if (block_count([&](int i) { return key[i] >= c1; }) >= nprobe) v = c1;
  }
  const int room = nprobe - block_count([&](int i) { return key[i] > v; });
  const int ntie = block_count([&](int i) { return key[i] == v; });
  uint32_t g2 = 0xffffffffu;  // tied ids <= g2 are kept
  if (ntie > room) {
    g2 = 0u;
    for (int bit = 12; bit >= 0; --bit) {  // ids < 4096
      const uint32_t c1 = g2 | (1u << bit);
      if (block_count([&](int i) { return key[i] == v && (uint32_t)(tid + 256 * i) < c1; }) < room) g2 = c1;
    }
  }
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    const int c = tid + 256 * i;
    const bool keep = c < m && (key[i] > v || (key[i] == v && (uint32_t)c <= g2));
    if (keep) {
      const int o = atomicAdd(&npos, 1);
      ps[q * stride + o] = S[q * m + c];
      pid[q * stride + o] = c;
    }
  }
}

int launch_probe_select(const float* S, int64_t nq, int m, int nprobe, float* ps, int64_t* pid, hipStream_t st,
                        const int* nprobe_of) {
  if (m > kProbeMaxLists || nprobe < 1 || nprobe > m || nq <= 0) return -1;
  if (nprobe_of)
    hipLaunchKernelGGL(probe_select_kernel<true>, dim3((unsigned)nq), dim3(256), 0, st, S, m, nprobe, ps, pid, nprobe_of);
  else
    hipLaunchKernelGGL(probe_select_kernel<false>, dim3((unsigned)nq), dim3(256), 0, st, S, m, nprobe, ps, pid, nullptr);
  return 0;
}

int launch_group_pairs(const int64_t* probes, int P, int m, int* pair_off, int* pairs, hipStream_t st, bool skip) {
  if (m > kMaxListsGroup) return -1;
  if (skip)
    hipLaunchKernelGGL(group_pairs_kernel<true>, dim3(1), dim3(1024), 0, st, probes, P, m, pair_off, pairs);
  else
    hipLaunchKernelGGL(group_pairs_kernel<false>, dim3(1), dim3(1024), 0, st, probes, P, m, pair_off, pairs);
  return 0;
}

// ---- a probe count per question: the slots and candidates of the pairs that do not exist ----
// Block (q, j) with j >= nprobe_of[q]: probes[q * nprobe + j] = -1 (group_pairs_kernel<true> skips it) and the
// pair's splits * 4 * K candidate slots are set empty (-inf, kEmptyRow) — no list-scan block writes them, the
// final merge reads every slot of every question, and the workspace still holds whatever an earlier, wider call
// left there.
__global__ __launch_bounds__(256) void absent_pairs_kernel(const int* __restrict__ nprobe_of, int nprobe, int per_pair,
                                                           int64_t* __restrict__ pid, float* __restrict__ ps,
                                                           float* __restrict__ cand_s, int* __restrict__ cand_r) {
  const int64_t q = blockIdx.x;
  const int j = blockIdx.y;
  if (j < nprobe_of[q]) return;
  const int64_t p = q * nprobe + j;
  if (threadIdx.x == 0) {
    pid[p] = -1;
    ps[p] = -__builtin_inff();
  }
  for (int i = threadIdx.x; i < per_pair; i += 256) {
    cand_s[p * per_pair + i] = -__builtin_inff();
    cand_r[p * per_pair + i] = kEmptyRow;
  }
}

void launch_absent_pairs(const int* nprobe_of, int64_t nq, int nprobe, int per_pair, int64_t* pid, float* ps,
                         float* cs, int* cr, hipStream_t st) {
  hipLaunchKernelGGL(absent_pairs_kernel, dim3((unsigned)nq, (unsigned)nprobe), dim3(256), 0, st, nprobe_of, nprobe,
                     per_pair, pid, ps, cs, cr);
}

// ---- exact re-rank of IVF candidates against the original rows -----------------------------------
// One block per query, one wave per candidate (strided): f32 dot of the query and the candidate's
// original row (bf16 / f16 / f32, e.g. the brute-force store's buffer), wave reduction.  Rows < 0
// (padding) stay -1 with score -inf, which the merge skips.  Row-sharded use (rfx_rerank_candidates):
// the candidates are global rows, X holds rows [row_lo, row_lo + n_rows); the others are padding here.
template <int DTQ, int DTX>
__global__ __launch_bounds__(256) void rerank_kernel(const void* __restrict__ Q, const void* __restrict__ X, int D,
                                                     const int64_t* __restrict__ cand, int kc, int64_t row_lo,
                                                     int64_t n_rows, float* __restrict__ out_s,
                                                     int64_t* __restrict__ out_r) {
  const int64_t q = blockIdx.x;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int c = w; c < kc; c += 4) {
    const int64_t r = cand[q * kc + c];
    const int64_t lr = r - row_lo;
    const bool own = r >= 0 && lr >= 0 && lr < n_rows;
    float acc = 0.f;
    if (own)
      for (int d = lane; d < D; d += 64) acc = fmaf(load_elem<DTQ>(Q, q * D + d), load_elem<DTX>(X, lr * D + d), acc);
#pragma unroll
    for (int off = 32; off; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) {
      out_s[q * kc + c] = own ? acc : -__builtin_inff();
      out_r[q * kc + c] = own ? r : -1;  // (negative rows are never live in the merge)
    }
  }
}

int launch_rerank(const void* Q, int dtq, const void* X, int dtx, int D, const int64_t* cand, int64_t nq, int kc,
                  float* out_s, int64_t* out_r, hipStream_t st, int64_t row_lo, int64_t n_rows) {
  if (nq <= 0) return 0;
#define RFX_RR(A, B)                                                                                        \
  if (dtq == A && dtx == B) {                                                                               \
    hipLaunchKernelGGL((rerank_kernel<A, B>), dim3((unsigned)nq), dim3(256), 0, st, Q, X, D, cand, kc, row_lo, \
                       n_rows, out_s, out_r);                                                               \
    return 0;                                                                                               \
  }
  RFX_RR(RFX_F32, RFX_F32) RFX_RR(RFX_F32, RFX_BF16) RFX_RR(RFX_F32, RFX_F16)
  RFX_RR(RFX_BF16, RFX_F32) RFX_RR(RFX_BF16, RFX_BF16) RFX_RR(RFX_BF16, RFX_F16)
  RFX_RR(RFX_F16, RFX_F32) RFX_RR(RFX_F16, RFX_BF16) RFX_RR(RFX_F16, RFX_F16)
#undef RFX_RR
  return -1;
}

}  // namespace ivf
}  // namespace rfx
