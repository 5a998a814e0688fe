// k_ivf_deep.hip — the IVF deep search kernels (k_ivf_deep.h): every probed row's key into a per-question slab,
// then a radix selection and an LDS sort per question.  gfx950 only.
#include "k_ivf_deep.h"

#include "rfx_device.h"
#include "rfx_kernels.h"

namespace rfx {
namespace ivf {
namespace {

constexpr int kQB = 8;             // staged pairs of a batch, as in list_scan_kernel
constexpr int kSelThreads = 1024;  // deep_select_kernel / deep_order_kernel: 16 waves
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kSelMaxKeys = 2 * kDeepMaxK;  // the sort buffer: 2 * KB keys, 16 KiB at KB 1,024

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

// (score desc, row asc) as one unsigned order; s + 0 folds -0 into +0, which compare equal as floats
__device__ __forceinline__ uint64_t cand_key(float s, int row) {
  return ((uint64_t)ord_f32(s + 0.0f) << 32) | (uint32_t)~(uint32_t)row;
}
__device__ __forceinline__ float key_score(uint64_t key) {
  const uint32_t o = (uint32_t)(key >> 32);  // inverse of ord_f32
  return __uint_as_float(o & 0x80000000u ? o & 0x7fffffffu : ~o);
}
__device__ __forceinline__ int64_t key_row(uint64_t key) { return (int64_t)(int)~(uint32_t)key; }

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

// ---- LDS sort ----------------------------------------------------------------------------------------------------
// Workgroup-wide: b[0 .. n) (n a power of two), best (largest) key first.  Bitonic, in place; the caller's
// writes are behind a barrier, and it ends on one.
__device__ __forceinline__ void lds_sort_desc(uint64_t* b, int n) {
  for (int k2 = 2; k2 <= n; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n / 2; i += blockDim.x) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
        const uint64_t a = b[lo], c = b[hi];
        if ((a < c) == ((lo & k2) == 0)) {
          b[lo] = c;
          b[hi] = a;
        }
      }
      __syncthreads();
    }
}

__device__ __forceinline__ void write_best(const uint64_t* buf, int64_t q, int k, float* __restrict__ out_s,
                                           int64_t* __restrict__ out_r) {
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    const uint64_t key = buf[j];
    out_s[q * k + j] = key ? key_score(key) : -__builtin_inff();
    out_r[q * k + j] = key ? key_row(key) : -1;
  }
}

// ---- kernel B: the k largest of a question's keys ----------------------------------------------------------------
// Histogram: one private 256-bin table per wave (16 KiB), so LDS adds of different waves never meet, and one test
// in front of the adds: when every participating lane of the wave holds the same bin — the high passes, where the
// byte is the score's sign and exponent and nearly every key agrees — one lane adds the count.  Otherwise each lane
// adds 1 to its bin; in the low passes (mantissa and row bits) the bins are spread and such adds rarely collide.
// A ballot per distinct bin would serve the first case equally and take up to 64 rounds in the second.
__global__ __launch_bounds__(kSelThreads) void deep_select_kernel(const uint64_t* __restrict__ slab, int64_t qcap,
                                                                  const int* __restrict__ n_keys, int KB, int k,
                                                                  float* __restrict__ out_s, int64_t* __restrict__ out_r) {
  __shared__ uint32_t hist[kSelWaves][256];
  __shared__ __attribute__((aligned(16))) uint64_t buf[kSelMaxKeys];
  __shared__ uint32_t s_bin, s_above, s_inbin;
  __shared__ int s_cnt;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t q = blockIdx.x;
  const int n = n_keys[q], N2 = 2 * KB;
  const u64x2* kv = (const u64x2*)(slab + q * qcap);  // q * qcap is even: 16-B aligned
  const int nv = (n + 1) / 2;                         // (an odd n: the last pair's second key is masked by 2 i + 1 < n)

  uint64_t lo = 0, pmask = 0;  // the prefix found so far and its bits; a key takes part when (key & pmask) == lo
  uint32_t above = 0;          // keys above the prefix
  if (n > N2) {
    for (int pass = 0; pass < 8; ++pass) {
      const int shift = 56 - 8 * pass;
      for (int i = tid; i < kSelWaves * 256; i += kSelThreads) (&hist[0][0])[i] = 0;
      __syncthreads();
      for (int i0 = 0; i0 < nv; i0 += kSelThreads) {  // (uniform trip count: the ballots below)
        const int i = i0 + tid;
        u64x2 v = {0ull, 0ull};
        if (i < nv) v = pass == 0 ? __builtin_nontemporal_load(kv + i) : kv[i];  // read once, then from L2
        const uint64_t two[2] = {v.x, 2 * i + 1 < n ? v.y : 0ull};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint64_t key = two[h];
          const bool part = key != 0 && (key & pmask) == lo;
          const int bin = (int)(key >> shift) & 255;
          const uint64_t act = __ballot(part);
          if (act) {
            const int first = __builtin_ctzll(act);
            const int b0 = __builtin_amdgcn_readlane(bin, first);
            if (__ballot(part && bin == b0) == act) {
              if (lane == first) atomicAdd(&hist[w][b0], (uint32_t)__popcll(act));
            } else if (part) {
              atomicAdd(&hist[w][bin], 1u);
            }
          }
        }
      }
      __syncthreads();
      if (tid < 256) {
        uint32_t c = 0;
#pragma unroll
        for (int ww = 0; ww < kSelWaves; ++ww) c += hist[ww][tid];
        hist[0][tid] = c;  // (thread tid alone reads and writes column tid)
      }
      __syncthreads();
      if (w == 0) {
        // suffix scan of the 256 bins, 4 per lane: sfx[j] = keys in the bins >= 4 lane + j.  The k-th key of the
        // prefix (rank need = k - above) is in the highest bin whose suffix count reaches need; no such bin
        // (fewer keys than k, first pass only): bin 0, every key is taken.
        uint32_t c[4], sfx[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = hist[0][4 * lane + j];
        uint32_t run = c[0] + c[1] + c[2] + c[3];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t v = __shfl_down(run, d);
          if (lane + d < 64) run += v;
        }
        sfx[3] = run - (c[0] + c[1] + c[2]);
        sfx[2] = sfx[3] + c[2];
        sfx[1] = sfx[2] + c[1];
        sfx[0] = sfx[1] + c[0];
        const uint32_t need = (uint32_t)k - above;
        int reach = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) reach += (int)__popcll(__ballot(sfx[j] >= need));
        const int b = max(reach - 1, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (4 * lane + j == b) {
            s_bin = (uint32_t)b;
            s_inbin = c[j];
            s_above = sfx[j] - c[j];
          }
      }
      __syncthreads();
      lo |= (uint64_t)s_bin << shift;
      pmask |= 0xffull << shift;
      above += s_above;
      if (above + s_inbin <= (uint32_t)N2) break;  // (uniform; distinct rows: one key per bin after the 8th pass)
    }
  }
  // gather: the keys above the prefix and in its bin are the non-zero keys >= lo, at most 2 * KB of them
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (int i0 = 0; i0 < nv; i0 += kSelThreads) {
    const int i = i0 + tid;
    u64x2 v = {0ull, 0ull};
    if (i < nv) v = kv[i];
    const uint64_t two[2] = {v.x, 2 * i + 1 < n ? v.y : 0ull};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint64_t key = two[h];
      const bool take = key != 0 && key >= lo;
      const uint64_t m = __ballot(take);
      if (m) {
        const int leader = __builtin_ctzll(m);
        int base = 0;
        if (lane == leader) base = atomicAdd(&s_cnt, (int)__popcll(m));
        base = __builtin_amdgcn_readlane(base, leader);
        const int slot = base + (int)__popcll(m & ((1ull << lane) - 1));
        if (take && slot < N2) buf[slot] = key;
      }
    }
  }
  __syncthreads();
  for (int i = min(s_cnt, N2) + tid; i < N2; i += kSelThreads) buf[i] = 0;
  __syncthreads();
  lds_sort_desc(buf, N2);
  write_best(buf, q, k, out_s, out_r);
}

// ---- the order of the re-ranked candidates -----------------------------------------------------------------------
// One workgroup per question: its n (score, row) pairs as keys into LDS, NS = n rounded up to 128 .. 1,024 sorted.
__global__ __launch_bounds__(kSelThreads) void deep_order_kernel(const float* __restrict__ s, const int64_t* __restrict__ r,
                                                                 int n, int NS, int k, float* __restrict__ out_s,
                                                                 int64_t* __restrict__ out_r) {
  __shared__ uint64_t buf[kDeepMaxK];
  const int64_t q = blockIdx.x;
  for (int i = threadIdx.x; i < NS; i += kSelThreads) {
    uint64_t key = 0;
    if (i < n) {
      const float sc = s[q * n + i];
      const int64_t row = r[q * n + i];
      if (row >= 0 && sc == sc) key = cand_key(sc, (int)row);  // a NaN score: a tombstoned row
    }
    buf[i] = key;
  }
  __syncthreads();
  lds_sort_desc(buf, NS);
  write_best(buf, q, k, out_s, out_r);
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

int launch_deep_select(const uint64_t* slab, int64_t qcap, const int* n_keys, int64_t nq, int k, float* out_s,
                       int64_t* out_r, hipStream_t st) {
  if (k < kDeepMinK || k > kDeepMaxK || nq < 1 || (qcap & 1) || ((uintptr_t)slab & 15)) return -1;
  hipLaunchKernelGGL(deep_select_kernel, dim3((unsigned)nq), dim3(kSelThreads), 0, st, slab, qcap, n_keys, deep_kb(k), k,
                     out_s, out_r);
  return 0;
}

int launch_deep_order(const float* s, const int64_t* r, int64_t nq, int n, int k, float* out_s, int64_t* out_r,
                      hipStream_t st) {
  if (n < 1 || n > kDeepMaxK || k < 1 || k > n || nq < 1) return -1;
  hipLaunchKernelGGL(deep_order_kernel, dim3((unsigned)nq), dim3(kSelThreads), 0, st, s, r, n, deep_kb(n), k, out_s,
                     out_r);
  return 0;
}

}  // namespace ivf
}  // namespace rfx
