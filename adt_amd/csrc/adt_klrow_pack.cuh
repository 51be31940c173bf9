// STOSA-ADT full-catalogue ranking under distance_metric='kl': the row images that turn the ROW-WISE KL divergence -- kl_distance
// (stosa/modules.py:45-50), the function bpr_optimization trains on, of the user's Gaussian (mu, cu) from the item's (mi, ci) -- into
// the dot-product score of adt_fullrank.cuh.  With ci = w_elu1(Ec[v]):
//
//   KL[u][v] = 0.5 (sum cu / ci + sum (mi - mu)^2 / ci - d + sum log ci - sum log cu) = nu[u] - (A[u] . W[v] + bias[v])
//
//   A[u] = [mu^2 + cu | mu]      W[v] = [-0.5 / ci | mi / ci]      bias[v] = -0.5 (sum log ci + sum mi^2 / ci)      nu[u] = -0.5 (d + sum log cu)
//
// k_klrow_pack writes, per row r of a (mean, covariance) pair of tables, one of the two images and its offset:
//   items = 1   c = w_elu1(C[r]);  img[r] = [-0.5 / c | M[r] / c];  off[r] = -0.5 (sum logf(c) + sum M[r]^2 / c)      -> (W, bias)
//   items = 0   c = C[r];          img[r] = [M[r]^2 + c | M[r]];    off[r] = -0.5 (d + sum logf(c))                    -> (A, nu)
// w_elu1 of adt_common.cuh is the function the KL loss and full-sort kernels apply to the same table entries; the user covariances are
// the rows _last_state returns, the rows k_kldist_full takes logf of.  DESIGN.md section 20.
//
// The layout and the reduction of k_wdist_pack: 16 lanes per row, lane `sub` owns the float4 column groups sub, sub + 16, ... (16-byte
// loads and stores); the two partial sums (logs, squared means over the covariance) are accumulated in ascending column order per lane
// and meet in four xor-shuffles (8, 4, 2, 1), the same order for every row wherever it lands in the grid: the output is
// bit-reproducible.  No atomics.
#pragma once
#include "adt_common.cuh"

namespace adt {

struct KlRowPackArgs {
  const float* M; const float* C; int ld;      // rows x d each, row stride ld
  int rows, d, items;
  float* img; int ldi;                         // rows x 2d, row stride ldi
  float* off;                                  // rows
  Lanes ln;                                    // k_klrow_pack<true> only: d = H * hd_pad; pad lanes of both halves of the image are +0.0
};

// LN: padded rows.  A pad lane holds ELU(0) + 1 = 1 on the item side and a covariance 0 (log 0) on the user side: it is left out of both
// sums by its index, both image halves are +0.0 there (selects, not products) and nu takes the true d, so the ranking kernel, which knows
// nothing of lanes, sees zero columns on both sides.
template <bool LN>
__global__ __launch_bounds__(256) void k_klrow_pack(KlRowPackArgs a) {
  const int sub = threadIdx.x & 15;
  for (int r = blockIdx.x * 16 + (threadIdx.x >> 4); r < a.rows; r += gridDim.x * 16) {      // the 16 lanes of a row share r
    const float* m = a.M + (size_t)r * a.ld;
    const float* c = a.C + (size_t)r * a.ld;
    float* o = a.img + (size_t)r * a.ldi;
    float pl = 0.f, pq = 0.f;
    for (int c4 = 4 * sub; c4 < a.d; c4 += 64) {
      const float4 mv = *reinterpret_cast<const float4*>(m + c4);
      float4 cv = *reinterpret_cast<const float4*>(c + c4);
      bool l0 = true, l1 = true, l2 = true, l3 = true;
      if constexpr (LN) { l0 = a.ln.live(c4); l1 = a.ln.live(c4 + 1); l2 = a.ln.live(c4 + 2); l3 = a.ln.live(c4 + 3); }
      float4 lo, hi;
      if (a.items) {
        cv = make_float4(w_elu1(cv.x), w_elu1(cv.y), w_elu1(cv.z), w_elu1(cv.w));
        const float4 q = make_float4(mv.x / cv.x, mv.y / cv.y, mv.z / cv.z, mv.w / cv.w);
        if (l0) pq += mv.x * q.x;
        if (l1) pq += mv.y * q.y;
        if (l2) pq += mv.z * q.z;
        if (l3) pq += mv.w * q.w;
        lo = make_float4(-0.5f / cv.x, -0.5f / cv.y, -0.5f / cv.z, -0.5f / cv.w);
        hi = q;
      } else {
        lo = make_float4(mv.x * mv.x + cv.x, mv.y * mv.y + cv.y, mv.z * mv.z + cv.z, mv.w * mv.w + cv.w);
        hi = mv;
      }
      if constexpr (LN) {
        lo = make_float4(l0 ? lo.x : 0.f, l1 ? lo.y : 0.f, l2 ? lo.z : 0.f, l3 ? lo.w : 0.f);
        hi = make_float4(l0 ? hi.x : 0.f, l1 ? hi.y : 0.f, l2 ? hi.z : 0.f, l3 ? hi.w : 0.f);
      }
      *reinterpret_cast<float4*>(o + c4) = lo;
      *reinterpret_cast<float4*>(o + a.d + c4) = hi;
      if (l0) pl += logf(cv.x);
      if (l1) pl += logf(cv.y);
      if (l2) pl += logf(cv.z);
      if (l3) pl += logf(cv.w);
    }
#pragma unroll
    for (int s = 8; s > 0; s >>= 1) {
      pl += __shfl_xor(pl, s, 64);
      pq += __shfl_xor(pq, s, 64);
    }
    if (sub == 0) a.off[r] = -0.5f * (a.items ? pl + pq : (float)(LN ? a.ln.H * a.ln.hd : a.d) + pl);
  }
}

}  // namespace adt
