// Additive statistics of full-catalogue ranks (include/adt_hip.h: adt_full_rank_stats; the device side of
// adt_amd/sasrec/utils.py:full_rank_stats).  HR@k and NDCG@k of a set of users are functions of one integer histogram of their ranks,
// clipped at kh; the AUC is the mean of (n_elig - rank) / max(n_elig, 1), a float64 sum.  DESIGN.md section 31.
//
// One workgroup of 256 threads per group, so every output word has a single writer and nothing in HBM is touched by an atomic.  The
// ranks are counted into a (kh + 1)-bin LDS histogram with integer LDS atomics.  The float64 sum is the only order-dependent quantity
// and its order is fixed: thread t adds the terms of rows t, t + 256, t + 512, ... of its group in ascending order, the 256 partial
// sums meet in a binary tree over LDS (stride 128, 64, ..., 1), and thread 0 adds the root to auc[g].  Two runs give the same bits.
#pragma once
#include "adt_common.cuh"

#define ADT_FULLSTATS_MAX_KH 1024
#define ADT_FULLSTATS_NTH 256

namespace adt {

struct FullStatsArgs {
  const int32_t* rank; const int32_t* n_elig;      // (groups * rows_per_group,), group-major
  int rows_per_group, kh;
  int64_t* hist;                                    // (groups, kh + 1), accumulated into
  double* auc;                                      // (groups,), accumulated into
};

static __global__ __launch_bounds__(ADT_FULLSTATS_NTH) void k_full_rank_stats(FullStatsArgs a) {
  __shared__ unsigned int bins[ADT_FULLSTATS_MAX_KH + 1];
  __shared__ double part[ADT_FULLSTATS_NTH];
  const int tid = threadIdx.x, g = blockIdx.x;
  for (int j = tid; j <= a.kh; j += ADT_FULLSTATS_NTH) bins[j] = 0u;
  __syncthreads();
  const int64_t row0 = (int64_t)g * (int64_t)a.rows_per_group;
  double s = 0.0;
  for (int i = tid; i < a.rows_per_group; i += ADT_FULLSTATS_NTH) {
    const int rk = a.rank[row0 + i], ne = a.n_elig[row0 + i];
    if (rk < 0) continue;                           // no target: the row counts nowhere
    atomicAdd(&bins[rk < a.kh ? rk : a.kh], 1u);    // at most rows_per_group < 2^31 per bin
    s += (double)(ne - rk) / (double)(ne > 1 ? ne : 1);
  }
  part[tid] = s;
  __syncthreads();
  for (int o = ADT_FULLSTATS_NTH / 2; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  int64_t* out = a.hist + (int64_t)g * (int64_t)(a.kh + 1);
  for (int j = tid; j <= a.kh; j += ADT_FULLSTATS_NTH) {
    const unsigned int n = bins[j];
    if (n) out[j] += (int64_t)n;
  }
  if (tid == 0) a.auc[g] += part[0];
}

}  // namespace adt
