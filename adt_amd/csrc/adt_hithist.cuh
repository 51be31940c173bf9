// Hit-position histogram of a full sort (include/adt_hip.h: adt_hit_hist; the device side of adt_amd/stosa/trainer.py:scores_from_hist).
// Every STOSA answer list has one item, so HIT@k, NDCG@k and MRR of a set of users are functions of one integer histogram: at which
// position 0 .. K-1 of its top-K list each user's held-out item stands, or K for "not in the list".
//
// One wave per list row.  Lane l reads top_idx[r][l] (one coalesced K * 4 byte read; a second read covers K > 64), the comparison is
// balloted -- the mask is 64 bits wide on gfx950 -- and its first set bit is the position.  A workgroup serves one group only: it counts
// into a (K + 1)-bin LDS histogram with integer LDS atomics and adds its non-zero bins to the int64 bins in HBM once, at the end.  Only
// integer atomics: the result does not depend on the order of execution.
//
// Block b serves group b / chunks, and of that group the rows i = (b % chunks) * 4 + wave, stepping by chunks * 4 (a grid-stride over
// the group's rows).  Row i of group g is list row g * rows_per_group + i, and its answer is answers[i].
#pragma once
#include "adt_common.cuh"

#define ADT_HITHIST_MAX_K 128
#define ADT_HITHIST_WAVES 4

namespace adt {

struct HitHistArgs {
  const int32_t* top_idx; int ld;      // (n_rows, K) at row stride ld
  int K, rows_per_group, chunks;
  const int32_t* answers;              // (rows_per_group,)
  unsigned long long* hist;            // (groups, K + 1), accumulated into
  int32_t* hit_pos;                    // (n_rows,), may be null
};

static __global__ __launch_bounds__(64 * ADT_HITHIST_WAVES) void k_hit_hist(HitHistArgs a) {
  __shared__ unsigned int bins[ADT_HITHIST_MAX_K + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = tid; j <= a.K; j += 64 * ADT_HITHIST_WAVES) bins[j] = 0u;
  __syncthreads();
  const int g = (int)(blockIdx.x / (unsigned)a.chunks), c = (int)(blockIdx.x % (unsigned)a.chunks);
  const int64_t row0 = (int64_t)g * (int64_t)a.rows_per_group;
  const bool wide = a.K > 64;          // uniform over the launch
  for (int64_t i = (int64_t)c * ADT_HITHIST_WAVES + wave; i < (int64_t)a.rows_per_group; i += (int64_t)a.chunks * ADT_HITHIST_WAVES) {
    const int64_t r = row0 + i;
    const int32_t* row = a.top_idx + r * (int64_t)a.ld;
    const int32_t ans = a.answers[i];
    const int32_t v0 = lane < a.K ? row[lane] : -1;
    const int32_t v1 = (wide && lane + 64 < a.K) ? row[lane + 64] : -1;
    const unsigned long long m0 = __ballot(v0 >= 0 && v0 == ans);       // a -1 (the tail of a short list) never matches
    int pos;
    if (m0) {
      pos = __ffsll((unsigned long long)m0) - 1;
    } else {
      const unsigned long long m1 = wide ? __ballot(v1 >= 0 && v1 == ans) : 0ull;
      pos = m1 ? 64 + __ffsll((unsigned long long)m1) - 1 : a.K;
    }
    if (lane == 0) {
      atomicAdd(&bins[pos], 1u);       // at most rows_per_group < 2^31 per bin
      if (a.hit_pos) a.hit_pos[r] = pos;
    }
  }
  __syncthreads();
  unsigned long long* out = a.hist + (int64_t)g * (int64_t)(a.K + 1);
  for (int j = tid; j <= a.K; j += 64 * ADT_HITHIST_WAVES) {
    const unsigned int n = bins[j];
    if (n) atomicAdd(&out[j], (unsigned long long)n);
  }
}

}  // namespace adt
