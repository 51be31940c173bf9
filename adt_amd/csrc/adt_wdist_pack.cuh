// STOSA-ADT full-catalogue ranking: the row images that turn the Wasserstein distance into the dot-product score of adt_fullrank.cuh.
//
//   dist[b][j] = sum (sm - em)^2 + sum (sqrt sc - sqrt ec)^2 = na[b] + nb[j] - 2 ([sm | sqrt sc] . [em | sqrt ec])
//
// k_wdist_pack writes, per row r of a (mean, covariance) pair of tables, img[r] = [M[r] | w_sqrt_cov(c)] (2d columns) and
// nrm[r] = nrm_scale * (sum M[r]^2 + sum c), c = elu ? w_elu1(C[r]) : C[r]: w_elu1 / w_sqrt_cov of adt_common.cuh, the functions
// k_wdist_full applies to the same entries, so the image holds exactly the operands that kernel multiplies.  Items: elu = 1,
// nrm_scale = -0.5 (the bias of adt_full_rank); user states: elu = 0, nrm_scale = 1 (na).  DESIGN.md section 12, "STOSA".
//
// 16 lanes per row, lane `sub` owns the float4 column groups sub, sub + 16, ... (16-byte loads and stores); the two partial sums
// (squares of the mean, covariance) are accumulated in ascending column order per lane and meet in four xor-shuffles (8, 4, 2, 1), the
// same order for every row wherever it lands in the grid: the output is bit-reproducible.  No atomics.
#pragma once
#include "adt_common.cuh"

namespace adt {

struct WPackArgs {
  const float* M; const float* C; int ld;      // rows x d each, row stride ld
  int rows, d, elu;
  float* img; int ldi;                         // rows x 2d, row stride ldi
  float* nrm; float nrm_scale;                 // rows
  Lanes ln;                                    // k_wdist_pack<true> only: d = H * hd_pad; pad lanes of both halves of the image are +0.0
};

// LN: padded rows.  ELU(0) + 1 = 1 and sqrt(max(0, 1e-24)) = 1e-12 on a pad lane; the image and the norm take live lanes only, so the
// ranking kernel, which knows nothing of lanes, sees zeros there.
template <bool LN>
__global__ __launch_bounds__(256) void k_wdist_pack(WPackArgs a) {
  const int sub = threadIdx.x & 15;
  for (int r = blockIdx.x * 16 + (threadIdx.x >> 4); r < a.rows; r += gridDim.x * 16) {      // the 16 lanes of a row share r
    const float* m = a.M + (size_t)r * a.ld;
    const float* c = a.C + (size_t)r * a.ld;
    float* o = a.img + (size_t)r * a.ldi;
    float pm = 0.f, pc = 0.f;
    for (int c4 = 4 * sub; c4 < a.d; c4 += 64) {
      const float4 mv = *reinterpret_cast<const float4*>(m + c4);
      float4 cv = *reinterpret_cast<const float4*>(c + c4);
      if (a.elu) cv = make_float4(w_elu1(cv.x), w_elu1(cv.y), w_elu1(cv.z), w_elu1(cv.w));
      float4 sv = make_float4(w_sqrt_cov(cv.x), w_sqrt_cov(cv.y), w_sqrt_cov(cv.z), w_sqrt_cov(cv.w));
      if constexpr (LN) {
        const bool l0 = a.ln.live(c4), l1 = a.ln.live(c4 + 1), l2 = a.ln.live(c4 + 2), l3 = a.ln.live(c4 + 3);
        cv = make_float4(l0 ? cv.x : 0.f, l1 ? cv.y : 0.f, l2 ? cv.z : 0.f, l3 ? cv.w : 0.f);
        sv = make_float4(l0 ? sv.x : 0.f, l1 ? sv.y : 0.f, l2 ? sv.z : 0.f, l3 ? sv.w : 0.f);
      }
      pm += mv.x * mv.x; pm += mv.y * mv.y; pm += mv.z * mv.z; pm += mv.w * mv.w;
      pc += cv.x; pc += cv.y; pc += cv.z; pc += cv.w;
      *reinterpret_cast<float4*>(o + c4) = mv;
      *reinterpret_cast<float4*>(o + a.d + c4) = sv;
    }
#pragma unroll
    for (int s = 8; s > 0; s >>= 1) {
      pm += __shfl_xor(pm, s, 64);
      pc += __shfl_xor(pc, s, 64);
    }
    if (sub == 0) a.nrm[r] = a.nrm_scale * (pm + pc);
  }
}

}  // namespace adt
