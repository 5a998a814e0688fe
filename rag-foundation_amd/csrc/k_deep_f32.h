// k_deep_f32.h — deep search on f32 stores: the exact top-k of a flat f32 store for k in 65..1,024
// (rfx_search_deep on an RFX_F32 index).  Host plan: deep_plan.h, the same numbers as the bf16 / f16 scan;
// buffers and meeting: k_deep_buf.h; merge: launch_deep_merge of k_deep.h.  Design: DESIGN §4.23.
//
// Path: the retrieval slice of ask_stream (gemini_rag.py:517-551) at the depth a re-ranker, rank fusion or a
// recall@100 evaluation reads, on an f32 store (RFX_DTYPE=f32; BASELINE configs 1-2 are f32).
//
// deep_scan_f32_kernel: grid (ranges, question groups), 256 threads, one wave per SIMD.  The frame is k_deep.h's:
// u64 candidate keys, per-question LDS buffers of 2 * KB keys, a threshold in a register, meetings every
// check_rounds rounds.  What differs is how rows and questions move.  The group's questions stay in registers as
// the B operands of v_mfma_f32_16x16x4_f32: lane (n = lane & 15, g = lane >> 4) holds, of question n and every
// 32-column block, columns 8 g .. 8 g + 7 (dim / 4 registers).  A whole f32 tile does not fit beside them, so rows
// stream as a ring over (tile, 32-column block): per step a lane loads the two 16-B vectors at bytes 32 g of the
// block of row r0 + n (non-temporal; a wave's pair of loads reads whole 128-B lines of 16 rows), and the step's 8
// MFMAs pair register j of the row with register j of the question, so A and B share one column permutation.
// The ring is kDeepF32Ring steps deep and runs across tile boundaries.  Every row is summed in the same order, so
// bit-identical rows get bit-identical scores and a tie goes to the lower row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "deep_plan.h"

namespace rfx {

constexpr int kDeepF32Ring = 8;  // ring steps in flight: 64 VGPRs, 16 KiB per wave

// Arguments as launch_deep_search (k_deep.h); X and Q are f32.  Returns 0, or -1 for arguments no kernel serves
// (nothing launched).
int launch_deep_search_f32(const DeepPlan& p, const void* X, int64_t nrows, int D, const void* Q, int64_t nq, int k,
                           const uint32_t* mask, uint64_t* ws, float* out_s, int64_t* out_r, hipStream_t st);

}  // namespace rfx
