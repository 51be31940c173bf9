// STOSA-ADT with distance_metric='kl': the full-sort scores of P stacked candidate groups of E users each, on a packed item image.
// DESIGN.md section 19.
//
// kl_predict_full (stosa/trainer.py:481-511) pads the item table to a multiple of the eval batch E and scores the E users against each
// E-item chunk; with kl_distance_matmul's broadcasts, for item v = cE + j and a = cE + u (adt_klattn.cuh, above k_kldist_full):
//
//   dist[u][v] = 0.5 (sum log ci_v - sum log cu_u + sum (mu_u - mi_a)^2 / ci_v + sum cu_j / ci_a - d)
//
// Row r of a stack of P groups is user u = r % E of group g = r / E: cu_j is row gE + j, never another group's.  A padding item
// a >= V has zero mean and unit covariance.
//
//   k_kldist_pack         per item v: img[v] = [Em[v] | 1 / ci_v] (2d columns), lv[v] = sum_c logf(ci_v[c]), ci = w_elu1(Ec): everything
//                         of the item tables that costs an expf, a logf or a divide, once per evaluation.  The layout and the reduction
//                         of k_wdist_pack: 16 lanes per row, 16-byte accesses, per-lane sums in ascending column order, four
//                         xor-shuffles.  Bit-reproducible, no atomics.
//   k_kldist_full_groups  one workgroup per (group, chunk, tile of 16 users), 4 waves.  It stages A[u] = [(mu_u - mi_a)^2 | 1 / ci_a]
//                         (2 * d32 columns, zero beyond d and beyond E) and lu[u] = sum_c logf(cu_u[c]) in LDS; wave w takes the
//                         16-item tiles 2w, 2w + 1, 2w + 8, ... of the chunk and multiplies A with B[j] = [1 / ci_v | cu_j], read from
//                         the image and the state rows: ONE 16 x 16 x 2d product per tile holds both sums, in exact fp32
//                         (v_mfma_f32_16x16x4_f32 through mma16<PREC_F32>).  Every entry is one fmaf chain over the columns in a fixed
//                         order and is written by exactly one lane: no atomics, nothing depends on the order of execution.  Lanes
//                         0..15 of a row group write 16 consecutive v.
#pragma once
#include "adt_common.cuh"

namespace adt {

struct KlPackArgs {
  const float* Em; const float* Ec; int ld;      // V x d each, row stride ld
  int V, d;
  float* img; int ldi;                           // V x 2d, row stride ldi
  float* lv;                                     // V
};

__global__ __launch_bounds__(256) void k_kldist_pack(KlPackArgs a) {
  const int sub = threadIdx.x & 15;
  for (int v = blockIdx.x * 16 + (threadIdx.x >> 4); v < a.V; v += gridDim.x * 16) {      // the 16 lanes of a row share v
    const float* m = a.Em + (size_t)v * a.ld;
    const float* c = a.Ec + (size_t)v * a.ld;
    float* o = a.img + (size_t)v * a.ldi;
    float pl = 0.f;
    for (int c4 = 4 * sub; c4 < a.d; c4 += 64) {
      const float4 mv = *reinterpret_cast<const float4*>(m + c4);
      float4 cv = *reinterpret_cast<const float4*>(c + c4);
      cv = make_float4(w_elu1(cv.x), w_elu1(cv.y), w_elu1(cv.z), w_elu1(cv.w));
      pl += logf(cv.x); pl += logf(cv.y); pl += logf(cv.z); pl += logf(cv.w);
      *reinterpret_cast<float4*>(o + c4) = mv;
      *reinterpret_cast<float4*>(o + a.d + c4) = make_float4(1.0f / cv.x, 1.0f / cv.y, 1.0f / cv.z, 1.0f / cv.w);
    }
#pragma unroll
    for (int s = 8; s > 0; s >>= 1) pl += __shfl_xor(pl, s, 64);
    if (sub == 0) a.lv[v] = pl;
  }
}

struct KlGroupsArgs {
  const float* Sm; const float* Sc; int lds;      // rows x d each, row stride lds
  const float* img; int ldi; const float* lv;     // k_kldist_pack's image of the V items
  int rows, E, V, d;                              // rows = P * E
  int nt, nch;                                    // user tiles per group, chunks: the grid is P * nch * nt workgroups
  float* dist; int ldo;                           // rows x V
};

static inline size_t kldist_groups_lds_bytes(int d) {
  const int d32 = (d + 31) & ~31;
  return ((size_t)16 * (2 * d32 + 4) + 16) * 4;
}

// the B operand of one half: 8 floats of a row at columns col0 .. col0 + 7, zero beyond d (d % 4 == 0) and for a row that is not there
ADT_DEVICE_INLINE Frag8 klg_frag(const float* row, bool live, int col0, int d) {
  float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
  if (live && col0 < d) x = *reinterpret_cast<const float4*>(row + col0);
  if (live && col0 + 4 < d) y = *reinterpret_cast<const float4*>(row + col0 + 4);
  Frag8 f;
  f.v[0] = x.x; f.v[1] = x.y; f.v[2] = x.z; f.v[3] = x.w;
  f.v[4] = y.x; f.v[5] = y.y; f.v[6] = y.z; f.v[7] = y.w;
  return f;
}

__global__ __launch_bounds__(256) void k_kldist_full_groups(KlGroupsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float klg_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  const int d32 = (a.d + 31) & ~31, ars = 2 * d32 + 4;
  float* A = klg_lds;
  float* lus = A + 16 * ars;
  const int ut = blockIdx.x % a.nt, rest = blockIdx.x / a.nt, ch = rest % a.nch, grp = rest / a.nch;
  const int u0 = ut * 16, row0 = grp * a.E, v0 = ch * a.E;

  // A[u] = [(mu_u - mi_a)^2 | 1 / ci_a], a = v0 + u; zero beyond d and beyond E
  const int q = d32 / 4;
  for (int idx = tid; idx < 16 * q; idx += 256) {
    const int r = idx / q, c4 = (idx - r * q) * 4, u = u0 + r;
    float4 dv = make_float4(0.f, 0.f, 0.f, 0.f), rv = dv;
    if (u < a.E && c4 < a.d) {
      const float4 sm = *reinterpret_cast<const float4*>(a.Sm + (size_t)(row0 + u) * a.lds + c4);
      float4 ma = make_float4(0.f, 0.f, 0.f, 0.f);
      rv = make_float4(1.f, 1.f, 1.f, 1.f);
      if (v0 + u < a.V) {
        const float* ia = a.img + (size_t)(v0 + u) * a.ldi;
        ma = *reinterpret_cast<const float4*>(ia + c4);
        rv = *reinterpret_cast<const float4*>(ia + a.d + c4);
      }
      dv = make_float4((sm.x - ma.x) * (sm.x - ma.x), (sm.y - ma.y) * (sm.y - ma.y), (sm.z - ma.z) * (sm.z - ma.z), (sm.w - ma.w) * (sm.w - ma.w));
    }
    *reinterpret_cast<float4*>(A + r * ars + c4) = dv;
    *reinterpret_cast<float4*>(A + r * ars + d32 + c4) = rv;
  }
  // lu[u]: 16 lanes per user, k_kldist_pack's reduction
  {
    const int sub = tid & 15, r = tid >> 4, u = u0 + r;
    float pl = 0.f;
    if (u < a.E) {
      const float* sc = a.Sc + (size_t)(row0 + u) * a.lds;
      for (int c4 = 4 * sub; c4 < a.d; c4 += 64) {
        const float4 cv = *reinterpret_cast<const float4*>(sc + c4);
        pl += logf(cv.x); pl += logf(cv.y); pl += logf(cv.z); pl += logf(cv.w);
      }
    }
#pragma unroll
    for (int s = 8; s > 0; s >>= 1) pl += __shfl_xor(pl, s, 64);
    if (sub == 0) lus[r] = pl;
  }
  __syncthreads();

  const int ntj = (a.E + 15) / 16, nk = d32 / 32;
  const float fd = (float)a.d;
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
      ri[t] = a.img + (size_t)(live[t] ? v[t] : 0) * a.ldi + a.d;
      sc[t] = a.Sc + (size_t)(row0 + (live[t] ? j : 0)) * a.lds;
    }
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int kk = 0; kk < nk; ++kk) {
      const int col0 = kk * 32 + 8 * g;
      const Frag8 fa = frag_contig(A + c * ars + col0);
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[t] = mma16<PREC_F32>(acc[t], fa, klg_frag(ri[t], live[t], col0, a.d));
    }
    for (int kk = 0; kk < nk; ++kk) {
      const int col0 = kk * 32 + 8 * g;
      const Frag8 fa = frag_contig(A + c * ars + d32 + col0);
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[t] = mma16<PREC_F32>(acc[t], fa, klg_frag(sc[t], live[t], col0, a.d));
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
