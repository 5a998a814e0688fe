// k_deep_sampled.h — deep search with a sampled threshold (rfx_search_deep_sampled): the exact top-k of a flat
// bf16 / f16 store for k in 65..1,024, one pass over the rows per 64 or 128 questions.  Plan: deep_sampled_plan.h;
// design and measurements: DESIGN §4.20.  The deep search of k_deep.h answers the questions that overflow.
//
// Path: the retrieval slice of ask_stream (gemini_rag.py:517-551) at the depth a re-ranker or rank fusion reads.
//
// deep_sampled_scan_kernel<DT, NDS, WAVES>: grid (ranges, question groups), 64 * WAVES threads.  The workgroup
// stages 64 rows x 256 columns at a time in LDS (two slots of 32 KiB: the next stage's loads, non-temporal, are
// in flight under the current stage's MFMAs and land in the other slot; one barrier per stage).  A 16-B chunk c of
// row r sits at chunk c ^ (r & 15) of its 512-B line, so the 16 rows of a fragment read hit 16 different bank
// groups.  Every wave keeps 16 questions resident as the B fragments of v_mfma_f32_16x16x32 and reads the A
// fragments of all 4 row tiles from that one image: a row is read from HBM once per 16 * WAVES questions.  With
// nq <= 16 (narrow) the 4 waves hold the SAME 16 questions and take one tile each.  LDS holds rows only.
//
// The kernel visits ordinals o of [0, n_ord): row o * stride.  A lane ends a round with 4 rows of ONE question in
// each accumulator.  DENSE epilogue: key of ordinal o to slab[q][o] (0 for a row the mask clears or a tombstone's
// NaN), 32 B per lane and 128 B per question and tile, no atomics.  THRESH epilogue (stride 1): compare with the
// question's tau in a register (>=; -inf passes every eligible row; NaN fails), one ballot per tile, and a passing
// row takes slot atomicAdd(count[q]) of the slab, stored while the slot is under cap; the counter keeps counting.
// The mode is an argument, not a template parameter: the sample pass and the main pass run the same code object,
// so a sample row's score in the main pass has the bits of the score that set tau.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "deep_sampled_plan.h"

namespace rfx {

// The whole call on stream st; nothing waits on the host.  ws: deep_sampled_ws_bytes, 256-B aligned.  Afterwards
// int32[0] of ws holds the number of questions the deep search of k_deep.h answered (their slab overflowed).
// Returns 0, or -1 for arguments no kernel serves.
int launch_deep_sampled_search(const DeepSampledPlan& p, const void* X, int64_t nrows, int D, int dtype, const void* Q,
                               int64_t nq, int k, const uint32_t* mask, uint8_t* ws, float* out_s, int64_t* out_r,
                               hipStream_t st);

}  // namespace rfx
