// k_mmr_deep.hip — the Gram pass and the selection of the deep MMR (see k_mmr_deep.h) and their launcher.
// gfx950 only.
#include "k_mmr_deep.h"

#include "k_mfma_common.h"
#include "k_mmr_rule.h"

namespace rfx {
namespace {

using namespace mmr;  // piece_has_nan, widen8, load8, mmr_objective
using mfc::v4f32x4;

constexpr int kT = kMmrDeepTile;
constexpr int kRowB = 512;            // bytes of a row in a slab: 256 columns
constexpr int kPanel = kT * kRowB;    // 32 KiB: one panel's slab
constexpr int kRpt = kT / 8;          // rows of a panel a thread stages: r0 + 8 j

struct GramArgs {
  const uint8_t* X;
  int64_t nrows;
  int D, n_max, n_pad;
  const int* ncand;
  const int64_t* cand_r;
  float* gram;
  float* norm;
  uint8_t* flag;
  uint32_t* bits;
};

// an f32 at or above sqrt(ss), ss an f64 sum of exact squares (relative error far under 2^-40)
__device__ __forceinline__ float norm_upper(double ss) {
  const double r = __builtin_sqrt(ss) * (1.0 + 0x1p-40);
  float f = (float)r;
  if (!(f < __builtin_inff())) return f;                  // inf (overflow) or NaN: the pair stays undecided
  if ((double)f < r) f = __uint_as_float(__float_as_uint(f) + 1u);
  return __uint_as_float(__float_as_uint(f) + 1u);         // f >= 0: the next f32 up
}

template <int DT>
__global__ __launch_bounds__(kMmrDeepThreads, 2) void mmr_gram_kernel(const GramArgs a) {
  __shared__ __attribute__((aligned(1024))) uint8_t lds[2 * kPanel];  // panel A (rows of tile ti), panel B (tile tj)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, g = lane >> 4;
  const int64_t q = blockIdx.y;
  const int nc = min(max(a.ncand[q], 0), a.n_max);
  const int T = a.n_pad / kT;
  int ti = 0, pr = (int)blockIdx.x;
  while (ti < T - 1 && pr >= T - ti) pr -= T - ti, ++ti;
  const int tj = min(ti + pr, T - 1);
  if (tj * kT >= nc) return;  // (uniform) a tile past the question's own candidates
  const bool diag = ti == tj;
  const int D = a.D, nds = D >> 6, nslab = (nds + 3) >> 2;
  const int W = a.n_pad >> 5;
  float* G = a.gram + q * a.n_pad * a.n_pad;

  {  // no pair of this tile (or its mirror) has an exact similarity yet
    uint32_t* B = a.bits + q * a.n_pad * W;
    const int r = (tid & 127) >> 1, w = tid & 1;
    if (tid < 128) B[(int64_t)(ti * kT + r) * W + tj * 2 + w] = 0u;
    else B[(int64_t)(tj * kT + r) * W + ti * 2 + w] = 0u;
  }

  // staging: thread -> chunk c of rows r0 + 8 j of both panels; a padding candidate's row is zeros
  const int c = tid & 31, r0 = tid >> 5;
  int64_t offA[kRpt], offB[kRpt];
#pragma unroll
  for (int j = 0; j < kRpt; ++j) {
    const int pa = ti * kT + r0 + 8 * j, pb = tj * kT + r0 + 8 * j;
    const int64_t ra = pa < nc ? a.cand_r[q * a.n_max + pa] : -1, rb = pb < nc ? a.cand_r[q * a.n_max + pb] : -1;
    offA[j] = ra >= 0 && ra < a.nrows ? ra * D * 2 : -1;
    offB[j] = rb >= 0 && rb < a.nrows ? rb * D * 2 : -1;
  }
  uint4 pf[2 * kRpt];
  auto load_slab = [&](int cs) {
    const bool on = c < min(4, nds - 4 * cs) * 8;  // the last slab may be short
    const int64_t at = (int64_t)cs * kRowB + c * 16;
#pragma unroll
    for (int j = 0; j < kRpt; ++j) {
      pf[j] = on && offA[j] >= 0 ? *(const uint4*)(a.X + offA[j] + at) : make_uint4(0, 0, 0, 0);
      pf[kRpt + j] = on && offB[j] >= 0 ? *(const uint4*)(a.X + offB[j] + at) : make_uint4(0, 0, 0, 0);
    }
  };

  double ss[kRpt];
  bool bad[kRpt];
#pragma unroll
  for (int j = 0; j < kRpt; ++j) ss[j] = 0.0, bad[j] = false;

  v4f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i >> 1][i & 1] = v4f32x4{0.f, 0.f, 0.f, 0.f};
  const int wr = wave >> 1, wc = wave & 1;  // the wave's 32 x 32 quarter of the tile
  const uint8_t* imgA = lds + (32 * wr + n) * kRowB;
  const uint8_t* imgB = lds + kPanel + (32 * wc + n) * kRowB;

  load_slab(0);
  for (int cs = 0; cs < nslab; ++cs) {
    if (diag) {  // the norms and the NaN flags of the tile's candidates, from the pieces in registers
#pragma unroll
      for (int j = 0; j < kRpt; ++j) {
        float e[8];
        widen8<DT>(pf[j], e);
        bad[j] |= piece_has_nan<DT>(pf[j]);
#pragma unroll
        for (int i = 0; i < 8; ++i) ss[j] = __builtin_fma((double)e[i], (double)e[i], ss[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < kRpt; ++j) {
      const int r = r0 + 8 * j;
      *(uint4*)(lds + r * kRowB + ((c ^ (r & 15)) << 4)) = pf[j];
      *(uint4*)(lds + kPanel + r * kRowB + ((c ^ (r & 15)) << 4)) = pf[kRpt + j];
    }
    __syncthreads();
    if (cs + 1 < nslab) load_slab(cs + 1);  // in flight under this slab's MFMAs
#pragma unroll
    for (int dl = 0; dl < 4; ++dl) {
      if (4 * cs + dl >= nds) break;  // (uniform)
      uint4 fa[2][2], fb[2][2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int at = ((dl * 8 + g * 2 + h) ^ n) << 4;
          fa[t][h] = *(const uint4*)(imgA + t * 16 * kRowB + at);
          fb[t][h] = *(const uint4*)(imgB + t * 16 * kRowB + at);
        }
#pragma unroll
      for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) {
          acc[ta][tb] = mfc::mfma16<DT>(fa[ta][0], fb[tb][0], acc[ta][tb]);
          acc[ta][tb] = mfc::mfma16<DT>(fa[ta][1], fb[tb][1], acc[ta][tb]);
        }
    }
    __syncthreads();  // every wave is done reading the slab before the next one lands
  }

  // acc[ta][tb][i] = candidate ti * 64 + 32 wr + 16 ta + 4 g + i against candidate tj * 64 + 32 wc + 16 tb + n
#pragma unroll
  for (int ta = 0; ta < 2; ++ta)
#pragma unroll
    for (int tb = 0; tb < 2; ++tb) {
      const int ra = ti * kT + 32 * wr + 16 * ta + 4 * g, cb = tj * kT + 32 * wc + 16 * tb + n;
#pragma unroll
      for (int i = 0; i < 4; ++i) G[(int64_t)(ra + i) * a.n_pad + cb] = acc[ta][tb][i];
      if (!diag) *(v4f32x4*)(G + (int64_t)cb * a.n_pad + ra) = acc[ta][tb];  // the mirror (16-byte aligned: ra % 4 == 0)
    }

  if (diag) {
#pragma unroll
    for (int j = 0; j < kRpt; ++j) {
      double s = ss[j];
      int b = bad[j];
#pragma unroll
      for (int off = 16; off; off >>= 1) {  // the 32 threads of a row are one half of a wave
        s += __shfl_xor(s, off);
        b |= __shfl_xor(b, off);
      }
      if (c == 0) {
        const int pos = ti * kT + r0 + 8 * j;
        a.norm[q * a.n_pad + pos] = norm_upper(s);
        a.flag[q * a.n_pad + pos] = (uint8_t)(b || offA[j] < 0);
      }
    }
  }
}

// ---- selection ----------------------------------------------------------------------------------------------
struct SelArgs {
  const uint8_t* X;
  int D, n_max, n_pad, k;
  const float* lam;
  const int* ncand;
  const float* cand_s;
  const int64_t* cand_r;
  float* gram;
  const float* norm;
  const uint8_t* flag;
  uint32_t* bits;
  float* out_s;
  int64_t* out_r;
  float* out_obj;
  int* stats;
};

constexpr int kNoPos = 0x7fffffff;

// rel - (1 - L) * m with m in f64: mmr_objective on a bracket's end (the same operations, each rounded on its own)
__device__ __forceinline__ double objective_at(double L, float s, double m) {
#pragma clang fp contract(off)
  const double rel = L * (double)s;
  const double pen = (1.0 - L) * m;
  return rel - pen;
}

// fl32 of the f64 FMA chain over the two rows read in place, one wave per dot (every lane returns it)
template <int DT>
__device__ __forceinline__ float exact_sim(const uint8_t* xi, const uint8_t* xj, int D, int lane) {
  double acc = 0.0;
  for (int c8 = lane; c8 < D / 8; c8 += kWave) {
    float u[8], v[8];
    load8<DT>(xi, c8, u);
    load8<DT>(xj, c8, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc = __builtin_fma((double)u[i], (double)v[i], acc);
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) acc += __shfl_xor(acc, off);
  return (float)acc;
}

// The workgroup's largest key, the lowest position among the equals (a NaN key never wins); two barriers.
__device__ __forceinline__ void block_best(double& key, int& pos, double* s_key, int* s_pos, int lane, int wave) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const double k2 = __shfl_xor(key, off);
    const int p2 = __shfl_xor(pos, off);
    if (k2 > key || (k2 == key && p2 < pos)) key = k2, pos = p2;
  }
  if (lane == 0) s_key[wave] = key, s_pos[wave] = pos;
  __syncthreads();
  key = s_key[0], pos = s_pos[0];
#pragma unroll
  for (int w = 1; w < kMmrDeepThreads / kWave; ++w)
    if (s_key[w] > key || (s_key[w] == key && s_pos[w] < pos)) key = s_key[w], pos = s_pos[w];
  __syncthreads();
}

template <int DT>
__global__ __launch_bounds__(kMmrDeepThreads) void mmr_deep_select_kernel(const SelArgs a) {
  constexpr int C = kMmrDeepMaxCand / kMmrDeepThreads;  // candidates per thread: tid + 256 c
  __shared__ float s_a[kMmrDeepMaxCand];     // a_i
  __shared__ float s_mex[kMmrDeepMaxCand];   // a contender's exact m
  __shared__ int s_pick[kMmrDeepMaxCand];    // the picked positions, in pick order
  __shared__ int s_cont[kMmrDeepMaxCand];    // this step's contenders
  __shared__ double s_key[kMmrDeepThreads / kWave];
  __shared__ int s_pos[kMmrDeepThreads / kWave];
  __shared__ int s_nc, s_dots;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q = blockIdx.x;
  const int n = min(max(a.ncand[q], 0), min(a.n_max, kMmrDeepMaxCand));
  const int k = a.k, W = a.n_pad >> 5;
  const double L = (double)a.lam[q];
  const double gamma = (double)(2 * a.D + 1) * 0x1p-24 * (1.0 + 0x1p-10);  // first order, plus the higher ones
  const double floor_ = (double)a.D * 0x1p-120;
  const double inf = __builtin_inf();
  float* G = a.gram + q * a.n_pad * a.n_pad;
  uint32_t* Bm = a.bits + q * a.n_pad * W;
  const float* cs = a.cand_s + q * a.n_max;
  const int64_t* cr = a.cand_r + q * a.n_max;
  const int64_t row_bytes = (int64_t)a.D * 2;

  float s[C], mt[C];
  double e[C];
  bool av[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int i = tid + kMmrDeepThreads * c;
    av[c] = i < n && !a.flag[q * a.n_pad + i];
    s[c] = av[c] ? cs[i] : -__builtin_inff();
    mt[c] = -__builtin_inff();
    e[c] = 0.0;
    s_a[i] = i < n ? a.norm[q * a.n_pad + i] : 0.f;
  }
  if (tid == 0) s_nc = 0, s_dots = 0;
  int n_cont = 0, n_dots = 0;  // (thread 0; lane 0 of every wave)
  __syncthreads();

  int t = 0, j = -1;
  {  // step 0: the first valid candidate
    double key = -inf;
    int pos = kNoPos;
#pragma unroll
    for (int c = C - 1; c >= 0; --c)
      if (av[c]) key = 0.0, pos = tid + kMmrDeepThreads * c;
    block_best(key, pos, s_key, s_pos, lane, wave);
    if (pos != kNoPos) {
#pragma unroll
      for (int c = 0; c < C; ++c)
        if (pos == tid + kMmrDeepThreads * c) {
          a.out_s[q * k] = s[c];
          a.out_r[q * k] = cr[pos];
          if (a.out_obj) a.out_obj[q * k] = (float)(L * (double)s[c]);
          av[c] = false;
        }
      if (tid == 0) s_pick[0] = pos;
      j = pos, t = 1;
    }
  }

  while (j >= 0 && t < k) {
    // ---- the last pick's row of G~: m~, its error, the bracket of every objective, B
    const float aj = s_a[j];
    const float* Gj = G + (int64_t)j * a.n_pad;
    double lo[C], hi[C], blo = -inf;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      lo[c] = -inf, hi[c] = inf;
      if (!av[c]) continue;
      const int i = tid + kMmrDeepThreads * c;
      const float gv = Gj[i];
      const double eps = gamma * (double)s_a[i] * (double)aj + floor_;
      if (!(eps < inf) || !(fabsf(gv) < __builtin_inff())) e[c] = inf;  // (a NaN fails both): undecided
      else e[c] = fmax(e[c], eps);
      mt[c] = fmaxf(mt[c], gv);
      if (e[c] < inf) {
        hi[c] = objective_at(L, s[c], (double)mt[c] - e[c]);
        const double l = objective_at(L, s[c], (double)mt[c] + e[c]);
        lo[c] = l == l ? l : -inf;
      }
      blo = fmax(blo, lo[c]);
    }
    int unused = kNoPos;
    block_best(blo, unused, s_key, s_pos, lane, wave);
    bool isc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      isc[c] = av[c] && !(hi[c] + 1e-12 < blo);  // (a NaN bracket is a contender)
      if (isc[c]) s_cont[atomicAdd(&s_nc, 1)] = tid + kMmrDeepThreads * c;
    }
    __syncthreads();
    const int nc = s_nc;
    if (nc == 0) break;  // (uniform) no valid candidate left: the rest is padding
    const bool exact = a.out_obj != nullptr || nc > 1;

    // ---- a wave per contender: its exact m
    if (exact) {
      for (int ci = wave; ci < nc; ci += kMmrDeepThreads / kWave) {
        const int i = s_cont[ci];
        float* Gi = G + (int64_t)i * a.n_pad;
        uint32_t* Bi = Bm + (int64_t)i * W;
        const float ai = s_a[i];
        const uint8_t* xi = a.X + cr[i] * row_bytes;
        double mlo = -inf;  // no picked j below this can hold the maximum
        for (int p = lane; p < t; p += kWave) {
          const int pj = s_pick[p];
          const float gv = Gi[pj];
          const bool ex = (Bi[pj >> 5] >> (pj & 31)) & 1u;
          const double eps = ex ? 0.0 : gamma * (double)ai * (double)s_a[pj] + floor_;
          const double l = (double)gv - eps;
          if (l == l) mlo = fmax(mlo, l);
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) mlo = fmax(mlo, __shfl_xor(mlo, off));
        float m = -__builtin_inff();
        for (int p0 = 0; p0 < t; p0 += kWave) {  // (uniform trip count: the ballot and the dots)
          const int p = p0 + lane;
          int pj = 0;
          bool need = false;
          if (p < t) {
            pj = s_pick[p];
            const float gv = Gi[pj];
            if ((Bi[pj >> 5] >> (pj & 31)) & 1u) {
              m = fmaxf(m, gv);
            } else {
              const double eps = gamma * (double)ai * (double)s_a[pj] + floor_;
              need = !((double)gv + eps < mlo);  // (non-finite: always)
            }
          }
          uint64_t todo = __ballot(need);
          while (todo) {
            const int b = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int jb = __shfl(pj, b);
            const float v = exact_sim<DT>(xi, a.X + cr[jb] * row_bytes, a.D, lane);
            m = fmaxf(m, v);
            if (lane == 0) {
              Gi[jb] = v;
              Bi[jb >> 5] |= 1u << (jb & 31);
              ++n_dots;
            }
          }
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
        if (lane == 0) s_mex[i] = m;
      }
      __syncthreads();
    }

    // ---- the pick: the largest exact objective, the lowest position among the equals
    double key = -inf;
    int pos = kNoPos;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (!isc[c]) continue;
      const int i = tid + kMmrDeepThreads * c;
      double o = 0.0;
      if (exact) {
        mt[c] = s_mex[i], e[c] = 0.0;
        o = mmr_objective(L, s[c], mt[c]);
        if (!(o == o)) o = -inf;
      }
      if (pos == kNoPos || o > key) key = o, pos = i;
    }
    block_best(key, pos, s_key, s_pos, lane, wave);
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (pos == tid + kMmrDeepThreads * c) {
        a.out_s[q * k + t] = s[c];
        a.out_r[q * k + t] = cr[pos];
        if (a.out_obj) a.out_obj[q * k + t] = (float)key;
        av[c] = false;
      }
    if (tid == 0) s_pick[t] = pos, s_nc = 0, n_cont += nc;
    j = pos, ++t;
  }

  // fewer than k valid candidates: (-inf, -1)
  for (int x = t + tid; x < k; x += kMmrDeepThreads) {
    a.out_s[q * k + x] = -__builtin_inff();
    a.out_r[q * k + x] = -1;
    if (a.out_obj) a.out_obj[q * k + x] = -__builtin_inff();
  }
  if (lane == 0 && n_dots) atomicAdd(&s_dots, n_dots);
  __syncthreads();
  if (tid == 0) a.stats[2 * q] = n_cont, a.stats[2 * q + 1] = s_dots;
}

}  // namespace

int launch_mmr_deep(const MmrDeepPlan& p, const void* X, int64_t nrows, int D, int dtype, int nq, int n_cand_max, int k,
                    const float* lam_d, const int* ncand_d, const float* cand_s, const int64_t* cand_r, float* out_s,
                    int64_t* out_r, float* out_obj, int* stats, float* norm, uint8_t* flag, uint32_t* bits, float* gram,
                    hipStream_t st) {
  if (dtype != RFX_BF16 && dtype != RFX_F16) return -1;
  if (D < 64 || D > kMmrDeepMaxDim || D % 64 != 0 || nrows < 0 || (nrows > 0 && !X)) return -1;
  if (nq < 1 || nq > p.slice_q || !mmr_deep_validate(nq, n_cand_max, k).empty()) return -1;
  if (p.n_pad < n_cand_max || p.n_pad % kT != 0 || p.n_pad > kMmrDeepMaxCand || p.tiles != p.n_pad / kT ||
      p.pairs != p.tiles * (p.tiles + 1) / 2)
    return -1;
  if (!lam_d || !ncand_d || !cand_s || !cand_r || !out_s || !out_r || !stats || !norm || !flag || !bits || !gram) return -1;
  if (((uintptr_t)gram & 15) || ((uintptr_t)bits & 3) || ((uintptr_t)norm & 3)) return -1;
  const GramArgs ga{(const uint8_t*)X, nrows, D, n_cand_max, p.n_pad, ncand_d, cand_r, gram, norm, flag, bits};
  const SelArgs sa{(const uint8_t*)X, D,     n_cand_max, p.n_pad, k,     lam_d, ncand_d, cand_s, cand_r,
                   gram,              norm,  flag,       bits,    out_s, out_r, out_obj, stats};
  const dim3 gg((unsigned)p.pairs, (unsigned)nq);
  if (dtype == RFX_BF16) {
    hipLaunchKernelGGL(mmr_gram_kernel<RFX_BF16>, gg, dim3(kMmrDeepThreads), 0, st, ga);
    hipLaunchKernelGGL(mmr_deep_select_kernel<RFX_BF16>, dim3((unsigned)nq), dim3(kMmrDeepThreads), 0, st, sa);
  } else {
    hipLaunchKernelGGL(mmr_gram_kernel<RFX_F16>, gg, dim3(kMmrDeepThreads), 0, st, ga);
    hipLaunchKernelGGL(mmr_deep_select_kernel<RFX_F16>, dim3((unsigned)nq), dim3(kMmrDeepThreads), 0, st, sa);
  }
  return 0;
}

}  // namespace rfx
