// k_ivf_scan.hip — the posting-list scan of the IVF-Flat int8 search (the steps before it, the numerics: k_ivf.hip).
// Block (L, s) takes the 64-row groups s*4 + w, s*4 + w + 4*S, ... of list L; the queries probing it (pairs) in batches
// of kQB; one top-K list per query and wave.  Candidates: cand[((q * nprobe + j) * S + s) * 4 + wave][K], every pair.
#include <tuple>

#include "rfx_device.h"
#include "rfx_kernels.h"

namespace rfx {
namespace ivf {

constexpr int kQB = 8, kSeedChunks = 2;

// The K best of a wave's kept candidates per query, exactly as the sorted list would hold them: (score desc,
// id asc), each query's K in lanes 0..K-1, sorted, and the list's threshold set (WaveList).  v = the K-th
// largest orderable score (bitwise search on ballot counts); ties at v are taken by the smallest ids (a second
// bitwise search over the tied ids), so the set is the list's set whatever the order the rows came in.
// Wave-local (LDS rows of this wave only).
template <int K, int QB, int NCH>
__device__ __forceinline__ void seed_lists(float (&ka)[QB][NCH], int (&kg)[NCH], WaveList<K> (&lst)[QB], int w) {
  __shared__ float ssa[4][K];
  __shared__ int ssr[4][K];
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int qi = 0; qi < QB; ++qi) {
    uint32_t key[NCH];
    int nvalid = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      // (+ 0.0f: -0.0 takes +0.0's key — a fine score is ±0.0 by its dot's sign once inv_r inv_q underflows, and
      // the rule compares scores as floats: equal, the row id decides.  The list keeps the score's own bits.)
      key[c] = ka[qi][c] == ka[qi][c] ? ord_f32(ka[qi][c] + 0.0f) : 0u;
      nvalid += (int)__popcll(__ballot(key[c] != 0u));
    }
    uint32_t v = 0u;
    if (nvalid > K)
      for (int bit = 31; bit >= 0; --bit) {
        const uint32_t c1 = v | (1u << bit);
        int cnt = 0;
#pragma unroll
        for (int c = 0; c < NCH; ++c) cnt += (int)__popcll(__ballot(key[c] >= c1));
        v = cnt >= K ? c1 : v;
      }
    int room = K;
#pragma unroll
    for (int c = 0; c < NCH; ++c) room -= (int)__popcll(__ballot(key[c] > v));
    // ties at v (v > 0 only): the room smallest ids, gid <= g2
    uint32_t g2 = 0u;
    if (v != 0u) {
      int ntie = 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c) ntie += (int)__popcll(__ballot(key[c] == v));
      if (ntie > room) {
        // g2 = the room-th smallest tied id: the largest value with fewer than room tied ids below it
        for (int bit = 31; bit >= 0; --bit) {
          const uint32_t c1 = g2 | (1u << bit);
          int cnt = 0;
#pragma unroll
          for (int c = 0; c < NCH; ++c) cnt += (int)__popcll(__ballot(key[c] == v && (uint32_t)kg[c] < c1));
          g2 = cnt < room ? c1 : g2;
        }
      } else {
        g2 = 0xffffffffu;
      }
    }
    int base = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const bool keep = key[c] > v || (v != 0u && key[c] == v && (uint32_t)kg[c] <= g2);
      const uint64_t kb = __ballot(keep);
      const int p =
          base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(kb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)kb, 0u));
      if (keep) {
        ssa[w][p] = ka[qi][c];
        ssr[w][p] = kg[c];
      }
      base += (int)__popcll(kb);
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float ls = lane < base ? ssa[w][lane] : -__builtin_inff();
    int lr = lane < base ? ssr[w][lane] : kEmptyRow;
    __builtin_amdgcn_wave_barrier();  // (read before the next query's compaction rewrites the rows)
#pragma unroll
    for (int kk = 2; kk <= K; kk <<= 1)
#pragma unroll
      for (int jj = kk >> 1; jj > 0; jj >>= 1) {
        const float ps = __shfl_xor(ls, jj);
        const int pr = __shfl_xor(lr, jj);
        const bool lower = (lane & jj) == 0, desc = (lane & kk) == 0;
        const bool mine = better(ls, lr, ps, pr);
        if (lower == desc ? !mine : mine) {
          ls = ps;
          lr = pr;
        }
      }
    lst[qi].ls = lane < K ? ls : -__builtin_inff();
    lst[qi].lr = lane < K ? lr : kEmptyRow;
    lst[qi].ts = readlane_f(ls, K - 1);
    lst[qi].tr = readlane_i(lr, K - 1);
  }
}

// Eligibility policy: the scans differ in three places of list_scan_kernel, each an `if constexpr` on E — how a batch
// of up to kQB pairs is staged, the lane's eligibility for a scored row, and the pair number the candidates go out
// under.  (The three are not member functions of policy types: a function is optimised before it is inlined, and the
// per-question kernels then come out as other, slower code than the body written in place.)  An ineligible row is
// treated exactly like a row past the end of its list: NaN among the seed chunks (seed_lists gives it key 0), valid
// = false in offer() after them, so it never takes a list slot and the K kept are the K best ELIGIBLE rows.
//   EveryRow     no mask is read (the kernel's mask argument is a null row_mask).
//   OneMask      DESIGN §4.15: row_mask, the store's row bitmap (bit r & 31 of word r >> 5 over insertion-order row
//                ids): one 4-byte vector load at the gid the lane holds anyway; gid < rows <= 32 * mask words (checked
//                by the caller), and a past-the-end lane reads its list's first row (cr = r0), so set bits past the
//                last row are never consulted.
//   PerQuestion  DESIGN §4.16: masks, a device table of such bitmaps, and mask_of[q], question q's index into it (-1:
//                no mask).  The staged mask indices are wave-uniform and the batch is put in ascending mask order
//                first (an odd-even transposition network over <= 8 scalars, once per batch), so the lane reloads its
//                mask word only where the index changes from one staged question to the next — a scalar branch; a
//                batch under one mask costs one 4-byte load per row, questions without a mask come first and cost
//                none.  Nothing depends on the order of a list's pairs (group_pairs_kernel's cursor is an atomic).
enum class Elig { EveryRow, OneMask, PerQuestion };

template <int K, int NC, Elig E, class... M>
__global__ __launch_bounds__(256) void list_scan_kernel(
    const int8_t* __restrict__ codes, const float* __restrict__ inv, const int* __restrict__ ids,
    const int64_t* __restrict__ off, const int* __restrict__ pair_off, const int* __restrict__ pairs, int nprobe,
    const int8_t* __restrict__ qq, const float* __restrict__ qinv, float* __restrict__ cand_s, int* __restrict__ cand_r,
    const M* __restrict__... mask) {
  // mask: row_mask, or masks and mask_of — __restrict__ parameters like the others (as members of a struct argument
  // they are not, and the per-question kernels then take 15 VGPRs more)
  const auto margs = std::make_tuple(mask...);
  constexpr int D = NC * 256, NCH = D / 16;  // 16-B chunks per row
  // Round 6: one lane per row.  The codes are in 64-row blocks, chunk-major (gather_rows_kernel), so a wave's
  // load of chunk c of its 64 rows is one 1-KB run; the batch's queries are wave-uniform and come through
  // scalar loads (SGPR operands of v_dot4), so no LDS reads, and every lane ends with its row's whole dot
  // for each query (no cross-lane sums).  Before, 16 lanes shared a row: per 4 rows a wave read 8 KB of
  // staged queries from LDS and summed 8 dots over 16 lanes (DPP), the list scan at 5.3 TB/s.
  constexpr int G = 4;  // chunks per load group (double-buffered)
  static_assert(NCH % G == 0, "chunk groups");
  constexpr int NG = NCH / G;
  __shared__ float qf[kQB];
  const int L = blockIdx.x, S = gridDim.y, sp = blockIdx.y;
  const int p0 = pair_off[L], p1 = pair_off[L + 1];
  if (p0 == p1) return;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int64_t r0 = off[L], r1 = off[L + 1];
  for (int pb = p0; pb < p1; pb += kQB) {
    const int nb = min(kQB, p1 - pb);
    const uint4* qv[kQB];
    int pr[kQB], mk[kQB];     // PerQuestion: the staged pairs and their mask indices (wave-uniform), in mask order
    const uint32_t* mp[kQB];  // and the masks' words (nullptr: no mask)
    if constexpr (E == Elig::PerQuestion) {
      const uint32_t* const* masks = std::get<0>(margs);
      const int* mask_of = std::get<1>(margs);
#pragma unroll
      for (int qi = 0; qi < kQB; ++qi) {
        pr[qi] = __builtin_amdgcn_readfirstlane(pairs[pb + (qi < nb ? qi : 0)]);
        mk[qi] = qi < nb ? __builtin_amdgcn_readfirstlane(mask_of[pr[qi] / nprobe]) : 0x7fffffff;
      }
#pragma unroll
      for (int r = 0; r < kQB; ++r)  // odd-even transposition: ascending mask index, the padding last
#pragma unroll
        for (int i = r & 1; i + 1 < kQB; i += 2)
          if (mk[i] > mk[i + 1]) {
            const int tm = mk[i], tp = pr[i];
            mk[i] = mk[i + 1], pr[i] = pr[i + 1];
            mk[i + 1] = tm, pr[i + 1] = tp;
          }
#pragma unroll
      for (int qi = 0; qi < kQB; ++qi) {
        mp[qi] = qi < nb && mk[qi] >= 0 ? masks[mk[qi]] : nullptr;
        qv[qi] = (const uint4*)(qq + (int64_t)(pr[qi] / nprobe) * D);
      }
      if (tid == 0) {
#pragma unroll
        for (int qi = 0; qi < kQB; ++qi) qf[qi] = qi < nb ? qinv[pr[qi] / nprobe] : 0.f;
      }
    } else {  // the pairs are read where they are used
#pragma unroll
      for (int qi = 0; qi < kQB; ++qi)
        qv[qi] = (const uint4*)(qq + (int64_t)(pairs[pb + (qi < nb ? qi : 0)] / nprobe) * D);
      if (tid < kQB) qf[tid] = tid < nb ? qinv[pairs[pb + tid] / nprobe] : 0.f;
    }
    __syncthreads();
    WaveList<K> lst[kQB];
#pragma unroll
    for (int qi = 0; qi < kQB; ++qi) lst[qi].init();
    // Round 6: a wave's first kSeedChunks 64-row chunks are kept in registers (score per lane, chunk and
    // query; the id per lane and chunk) and seed each query's sorted list by one selection (seed_lists), the
    // later chunks go through the list inserts.  A config-5 wave streams ~3 chunks of a list per batch, so the
    // inserts of its first chunks — nearly every candidate, the list still empty — were most of them.
    float ka[kQB][kSeedChunks];
    int kg[kSeedChunks];
    int nch = 0;  // chunks this wave has scored in this batch (wave-uniform)
#pragma unroll
    for (int c = 0; c < kSeedChunks; ++c) {
#pragma unroll
      for (int qi = 0; qi < kQB; ++qi) ka[qi][c] = __builtin_nanf("");
      kg[c] = kEmptyRow;
    }
    for (int64_t base = r0 + (int64_t)(sp * 4 + w) * 64; base < r1; base += 256 * S) {
      const int64_t crow = base + lane;
      const bool valid = crow < r1;
      const int64_t cr = valid ? crow : r0;  // in-list row (never past the list)
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
      float cand[kQB];  // |dot| <= 768 * 127 * 127 < 2^24: exact in f32, the value the 16-lane sum had
#pragma unroll
      for (int qi = 0; qi < kQB; ++qi) cand[qi] = (float)acc[qi];
      const float ir = inv[cr];
      const int gid = ids[cr];
      bool ok = valid;    // the row may take a list slot; PerQuestion: bit qi of okm = a slot of staged question qi's list
      uint32_t okm = 0u;
      if constexpr (E == Elig::OneMask) ok = valid && ((std::get<0>(margs)[(uint32_t)gid >> 5] >> (gid & 31)) & 1u);
      if constexpr (E == Elig::PerQuestion) {
        // gid < rows <= 32 * mask words of every table entry (checked by the caller); a past-the-end lane
        // looks up its list's first row and is cleared below
        const uint32_t wi = (uint32_t)gid >> 5, bi = (uint32_t)gid & 31u;
        uint32_t word = 0xffffffffu;  // mask index -1: every row
        int cur = -1;
#pragma unroll
        for (int qi = 0; qi < kQB; ++qi)
          if (qi < nb) {
            if (mk[qi] != cur) {  // wave-uniform
              cur = mk[qi];
              word = mp[qi][wi];
            }
            okm |= ((word >> bi) & 1u) << qi;
          }
        okm = valid ? okm : 0u;
      }
      auto okq = [&](int qi) { return E == Elig::PerQuestion ? ((okm >> qi) & 1u) != 0u : ok; };
      if (nch < kSeedChunks) {
#pragma unroll
        for (int c = 0; c < kSeedChunks; ++c)
          if (c == nch) {
#pragma unroll
            for (int qi = 0; qi < kQB; ++qi)
              ka[qi][c] = okq(qi) && qi < nb ? __fmul_rn(cand[qi], __fmul_rn(ir, qf[qi])) : __builtin_nanf("");
            kg[c] = gid;
          }
        if (++nch == kSeedChunks) seed_lists<K, kQB, kSeedChunks>(ka, kg, lst, w);
      } else {
#pragma unroll
        for (int qi = 0; qi < kQB; ++qi)
          if (qi < nb) lst[qi].offer(__fmul_rn(cand[qi], __fmul_rn(ir, qf[qi])), gid, okq(qi));
      }
    }
    if (nch < kSeedChunks) seed_lists<K, kQB, kSeedChunks>(ka, kg, lst, w);  // (fewer chunks than kept)
    if (lane < K) {
#pragma unroll
      for (int qi = 0; qi < kQB; ++qi)
        if (qi < nb) {
          const int64_t o = (((int64_t)(E == Elig::PerQuestion ? pr[qi] : pairs[pb + qi]) * S + sp) * 4 + w) * K + lane;
          cand_s[o] = lst[qi].ls;
          cand_r[o] = lst[qi].lr;
        }
    }
    __syncthreads();  // qf is rewritten by the next batch
  }
}

int list_k(int k) { return k <= 4 ? 4 : (k <= 16 ? 16 : (k <= 64 ? 64 : -1)); }

template <Elig E, class... A>  // the one (K, NC) table of the three policies; a = the kernel's arguments
static int launch_scan(int K, int D, int m, int splits, hipStream_t st, A... a) {
#define RFX_LS(KV, NCV)                                                                             \
  if (K == KV && D == NCV * 256) {                                                                  \
    hipLaunchKernelGGL((list_scan_kernel<KV, NCV, E>), dim3(m, splits), dim3(256), 0, st, a...); \
    return 0;                                                                                       \
  }
  RFX_LS(4, 1) RFX_LS(4, 2) RFX_LS(4, 3) RFX_LS(4, 4) RFX_LS(16, 1) RFX_LS(16, 2) RFX_LS(16, 3) RFX_LS(16, 4)
  RFX_LS(64, 1) RFX_LS(64, 2) RFX_LS(64, 3) RFX_LS(64, 4)
#undef RFX_LS
  return -1;
}

int launch_list_scan(int K, int D, int m, int splits, const int8_t* codes, const float* inv, const int* ids, const int64_t* off,
                     const int* pair_off, const int* pairs, int nprobe, const int8_t* qq, const float* qinv,
                     float* cs, int* cr, const uint32_t* row_mask, hipStream_t st) {
  return row_mask ? launch_scan<Elig::OneMask>(K, D, m, splits, st, codes, inv, ids, off, pair_off, pairs, nprobe, qq, qinv, cs,
                                         cr, row_mask)
                  : launch_scan<Elig::EveryRow>(K, D, m, splits, st, codes, inv, ids, off, pair_off, pairs, nprobe, qq, qinv, cs,
                                          cr, row_mask);
}

int launch_list_scan_multi(int K, int D, int m, int splits, const int8_t* codes, const float* inv, const int* ids,
                           const int64_t* off, const int* pair_off, const int* pairs, int nprobe, const int8_t* qq,
                           const float* qinv, float* cs, int* cr, const uint32_t* const* masks, const int* mask_of,
                           hipStream_t st) {
  return launch_scan<Elig::PerQuestion>(K, D, m, splits, st, codes, inv, ids, off, pair_off, pairs, nprobe, qq, qinv, cs,
                                      cr, masks, mask_of);
}

}  // namespace ivf
}  // namespace rfx
