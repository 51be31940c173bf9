// STOSA-ADT with distance_metric='kl' at a padded width: the grouped KL full sort of adt_kldist_groups.cuh on rows of d_pad = H * hd_pad
// columns, head h at [h * hd_pad, h * hd_pad + hd), the rest pad lanes.  DESIGN.md section 30.
//
// The score is kl_predict_full's at the TRUE width d = H * hd: for item v = cE + j and a = cE + u
//
//   dist[u][v] = 0.5 (sum log ci_v - sum log cu_u + sum (mu_u - mi_a)^2 / ci_v + sum cu_j / ci_a - d)
//
// with every sum over the live lanes.  A pad lane of a state covariance is +0.0 (log 0 = -inf) and of an item covariance ELU(0) + 1 = 1:
//
//   k_kldist_pack_lanes         k_kldist_pack's layout and reduction.  On a pad lane both halves of the image are +0.0 (selects, not
//                               products) and the lane is left out of lv by its index: no logf and no divide is taken of it.
//   k_kldist_full_groups_lanes  k_kldist_full_groups' decomposition, products and write pattern.  The staged operand
//                               A[u] = [(mu_u - mi_a)^2 | 1 / ci_a] is +0.0 on the pad lanes of both halves by the lane index (a padding
//                               item a >= V has 1 on the live lanes only), so whatever finite value the B operand [1 / ci_v | cu_j] holds
//                               there multiplies an exact zero; lu[u] sums logf over the live lanes; the subtracted dimension is H * hd.
//                               Exact fp32 (v_mfma_f32_16x16x4_f32 through mma16<PREC_F32>), one writer per entry, no atomics, fixed
//                               summation order.
//
// A translation unit of its own (adt_kldist_lanes.hip): the code objects of adt_fullrank.hip do not change.
#pragma once
#include "adt_common.cuh"

namespace adt {

struct KlPackLanesArgs {
  const float* Em; const float* Ec; int ld;      // V x d each, row stride ld
  int V, d;                                      // d = H * hd_pad
  float* img; int ldi;                           // V x 2d, row stride ldi
  float* lv;                                     // V
  Lanes ln;
};

__global__ __launch_bounds__(256) void k_kldist_pack_lanes(KlPackLanesArgs a) {
  const int sub = threadIdx.x & 15;
  for (int v = blockIdx.x * 16 + (threadIdx.x >> 4); v < a.V; v += gridDim.x * 16) {      // the 16 lanes of a row share v
    const float* m = a.Em + (size_t)v * a.ld;
    const float* c = a.Ec + (size_t)v * a.ld;
    float* o = a.img + (size_t)v * a.ldi;
    float pl = 0.f;
    for (int c4 = 4 * sub; c4 < a.d; c4 += 64) {
      const float4 mv = *reinterpret_cast<const float4*>(m + c4);
      const float4 cv = *reinterpret_cast<const float4*>(c + c4);
      const float mm[4] = {mv.x, mv.y, mv.z, mv.w}, cc[4] = {cv.x, cv.y, cv.z, cv.w};
      float om[4], orv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        om[i] = 0.f;
        orv[i] = 0.f;
        if (a.ln.live(c4 + i)) {
          const float ci = w_elu1(cc[i]);
          pl += logf(ci);
          om[i] = mm[i];
          orv[i] = 1.0f / ci;
        }
      }
      *reinterpret_cast<float4*>(o + c4) = make_float4(om[0], om[1], om[2], om[3]);
      *reinterpret_cast<float4*>(o + a.d + c4) = make_float4(orv[0], orv[1], orv[2], orv[3]);
    }
#pragma unroll
    for (int s = 8; s > 0; s >>= 1) pl += __shfl_xor(pl, s, 64);
    if (sub == 0) a.lv[v] = pl;
  }
}

struct KlGroupsLanesArgs {
  const float* Sm; const float* Sc; int lds;      // rows x d each, row stride lds
  const float* img; int ldi; const float* lv;     // k_kldist_pack_lanes' image of the V items
  int rows, E, V, d;                              // rows = P * E; d = H * hd_pad, a multiple of 64
  int nt, nch;                                    // user tiles per group, chunks: the grid is P * nch * nt workgroups
  float* dist; int ldo;                           // rows x V
  Lanes ln;
};

static inline size_t kldist_groups_lanes_lds_bytes(int d) { return ((size_t)16 * (2 * d + 4) + 16) * 4; }

// the B operand of one half: 8 floats of a row at columns col0 .. col0 + 7 (col0 + 8 <= d), zero for a row that is not there
ADT_DEVICE_INLINE Frag8 klgl_frag(const float* row, bool live, int col0) {
  float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
  if (live) {
    x = *reinterpret_cast<const float4*>(row + col0);
    y = *reinterpret_cast<const float4*>(row + col0 + 4);
  }
  Frag8 f;
  f.v[0] = x.x; f.v[1] = x.y; f.v[2] = x.z; f.v[3] = x.w;
  f.v[4] = y.x; f.v[5] = y.y; f.v[6] = y.z; f.v[7] = y.w;
  return f;
}

__global__ __launch_bounds__(256) void k_kldist_full_groups_lanes(KlGroupsLanesArgs a) {
  extern __shared__ __attribute__((aligned(16))) float klgl_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  const int d = a.d, ars = 2 * d + 4;
  float* A = klgl_lds;
  float* lus = A + 16 * ars;
  const int ut = blockIdx.x % a.nt, rest = blockIdx.x / a.nt, ch = rest % a.nch, grp = rest / a.nch;
  const int u0 = ut * 16, row0 = grp * a.E, v0 = ch * a.E;

  // A[u] = [(mu_u - mi_a)^2 | 1 / ci_a], a = v0 + u; +0.0 on the pad lanes and beyond E
  const int q = d / 4;
  for (int idx = tid; idx < 16 * q; idx += 256) {
    const int r = idx / q, c4 = (idx - r * q) * 4, u = u0 + r;
    float4 dv = make_float4(0.f, 0.f, 0.f, 0.f), rv = dv;
    if (u < a.E) {
      const float4 sm = *reinterpret_cast<const float4*>(a.Sm + (size_t)(row0 + u) * a.lds + c4);
      float4 ma = make_float4(0.f, 0.f, 0.f, 0.f);
      rv = make_float4(1.f, 1.f, 1.f, 1.f);
      if (v0 + u < a.V) {
        const float* ia = a.img + (size_t)(v0 + u) * a.ldi;
        ma = *reinterpret_cast<const float4*>(ia + c4);
        rv = *reinterpret_cast<const float4*>(ia + d + c4);
      }
      const bool l0 = a.ln.live(c4), l1 = a.ln.live(c4 + 1), l2 = a.ln.live(c4 + 2), l3 = a.ln.live(c4 + 3);
      dv = make_float4(l0 ? (sm.x - ma.x) * (sm.x - ma.x) : 0.f, l1 ? (sm.y - ma.y) * (sm.y - ma.y) : 0.f,
                       l2 ? (sm.z - ma.z) * (sm.z - ma.z) : 0.f, l3 ? (sm.w - ma.w) * (sm.w - ma.w) : 0.f);
      rv = make_float4(l0 ? rv.x : 0.f, l1 ? rv.y : 0.f, l2 ? rv.z : 0.f, l3 ? rv.w : 0.f);
    }
    *reinterpret_cast<float4*>(A + r * ars + c4) = dv;
    *reinterpret_cast<float4*>(A + r * ars + d + c4) = rv;
  }
  // lu[u]: 16 lanes per user, k_kldist_pack's reduction over the live lanes
  {
    const int sub = tid & 15, r = tid >> 4, u = u0 + r;
    float pl = 0.f;
    if (u < a.E) {
      const float* sc = a.Sc + (size_t)(row0 + u) * a.lds;
      for (int c4 = 4 * sub; c4 < d; c4 += 64) {
        const float4 cv = *reinterpret_cast<const float4*>(sc + c4);
        if (a.ln.live(c4)) pl += logf(cv.x);
        if (a.ln.live(c4 + 1)) pl += logf(cv.y);
        if (a.ln.live(c4 + 2)) pl += logf(cv.z);
        if (a.ln.live(c4 + 3)) pl += logf(cv.w);
      }
    }
#pragma unroll
    for (int s = 8; s > 0; s >>= 1) pl += __shfl_xor(pl, s, 64);
    if (sub == 0) lus[r] = pl;
  }
  __syncthreads();

  const int ntj = (a.E + 15) / 16, nk = d / 32;
  const float fd = (float)(a.ln.H * a.ln.hd);
  for (int jt = 2 * w; jt < ntj; jt += 8) {
    int v[2];
    bool live[2];
    const float* ri[2];
    const float* sc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int j = (jt + t) * 16 + c;
      v[t] = v0 + j;
      live[t] = j < a.E && v[t] < a.V;
      ri[t] = a.img + (size_t)(live[t] ? v[t] : 0) * a.ldi + d;
      sc[t] = a.Sc + (size_t)(row0 + (live[t] ? j : 0)) * a.lds;
    }
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int kk = 0; kk < nk; ++kk) {
      const int col0 = kk * 32 + 8 * g;
      const Frag8 fa = frag_contig(A + c * ars + col0);
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[t] = mma16<PREC_F32>(acc[t], fa, klgl_frag(ri[t], live[t], col0));
    }
    for (int kk = 0; kk < nk; ++kk) {
      const int col0 = kk * 32 + 8 * g;
      const Frag8 fa = frag_contig(A + c * ars + d + col0);
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[t] = mma16<PREC_F32>(acc[t], fa, klgl_frag(sc[t], live[t], col0));
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (!live[t]) continue;
      const float lvv = a.lv[v[t]];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int u = u0 + 4 * g + r;
        if (u < a.E) a.dist[(size_t)(row0 + u) * a.ldo + v[t]] = 0.5f * (((lvv - lus[4 * g + r]) + acc[t][r]) - fd);
      }
    }
  }
}

}  // namespace adt
