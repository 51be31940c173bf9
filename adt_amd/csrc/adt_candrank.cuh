// Candidate scores, and the fused score + rank + histogram of the device-side sampled evaluation (include/adt_hip.h: adt_score_rank,
// adt_cand_rank_hist; adt_amd/sasrec/utils.py:evaluate_device).
//
// cand_score16 is THE score of a (feature row, item) pair: k_score (adt_misc.cuh) and k_cand_rank_hist both call it, so a rank counted
// here is the rank k_rank counts over k_score's logits, ties included.  16 lanes share a candidate: lane `sub` multiplies the float4
// columns 4 * sub + 64 k of the two rows, the partial sums are added by the xor-shuffle tree 8, 4, 2, 1 (all 16 lanes end up with the
// sum), then the bias is added.
//
// k_cand_rank_hist: one wave per feature row, four candidates per pass.  Row r belongs to group r / rows_per_group and reads candidate
// row r % rows_per_group (P stacked search candidates share one (rows_per_group, C) slice of the resident table: nothing is repeated).
// rank = #{c > 0 : s_c > s_0}, strict as k_rank; one integer atomicAdd per row into hist[group][rank].  No float atomics and no logit
// matrix: the result does not depend on scheduling.
#pragma once
#include "adt_common.cuh"

namespace adt {

// f, e: the two rows (16-byte aligned, d % 4 == 0).  Every lane of the 16 returns the dot product.
ADT_DEVICE_INLINE float cand_dot16(const float* f, const float* e, int d, int sub) {
  float s = 0.f;
  for (int c4 = 4 * sub; c4 < d; c4 += 64) {
    const float4 fv = *reinterpret_cast<const float4*>(f + c4);
    const float4 ev = *reinterpret_cast<const float4*>(e + c4);
    s += fv.x * ev.x + fv.y * ev.y + fv.z * ev.z + fv.w * ev.w;
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}
ADT_DEVICE_INLINE float cand_score16(const float* f, const float* E, const float* bias, int item, int d, int sub) {
  return cand_dot16(f, E + (size_t)item * d, d, sub) + (bias ? bias[item] : 0.f);
}

struct CandRankArgs {
  const float* F; int ldf;       // n_rows feature rows, d wide
  const float* E;                // item table, d wide
  const float* bias;             // per item, or null
  const int32_t* cand;           // (rows_per_group, C) item ids
  int n_rows, rows_per_group, C, d;
  unsigned long long* hist;      // (n_rows / rows_per_group, C), accumulated into
  int32_t* rank;                 // (n_rows,), may be null
};

static __global__ __launch_bounds__(256) void k_cand_rank_hist(CandRankArgs a) {
  const int lane = threadIdx.x & 63, sub = lane & 15, quad = lane >> 4;
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < a.n_rows; r += gridDim.x * 4) {      // uniform over the wave
    const int g = r / a.rows_per_group;
    const int32_t* crow = a.cand + (size_t)(r - g * a.rows_per_group) * (size_t)a.C;
    const float* f = a.F + (size_t)r * (size_t)a.ldf;
    float s0 = 0.f;
    int cnt = 0;
    for (int c0 = 0; c0 < a.C; c0 += 4) {
      const int cidx = c0 + quad;
      const bool live = cidx < a.C;
      const float s = cand_score16(f, a.E, a.bias, crow[live ? cidx : 0], a.d, sub);      // past the row: the target again, not counted
      if (c0 == 0) s0 = __shfl(s, 0, 64);
      cnt += __popcll(__ballot(live && cidx > 0 && sub == 0 && s > s0));
    }
    if (lane == 0) {
      atomicAdd(&a.hist[(size_t)g * (size_t)a.C + (size_t)cnt], 1ull);      // cnt <= C - 1
      if (a.rank) a.rank[r] = cnt;
    }
  }
}

}  // namespace adt
