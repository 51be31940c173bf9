// Row kernels for widths that are not multiples of 64 (SASRec-ADT at hidden_units 50, 100, ...).  Activations and parameters keep a
// PADDED layout: H heads of hd live lanes each, head h at columns [h * hd_pad, h * hd_pad + hd) of a row of d_pad = H * hd_pad floats
// (hd_pad a power of two), every pad lane exactly zero.  Dense layers, attention, the head classifier and the logits are invariant under
// zero padding and run on the padded shapes unchanged; what is NOT invariant lives here:
//   * LayerNorm statistics over the d = H * hd live lanes (pad lanes of y / dx / dgamma / dbeta written or left as exact zeros);
//   * dropout, whose counter RNG (oracle/rng.py) indexes the elements of the TRUE-width tensor: element (row, live lane c) has index
//     row * d + true_col(c); four consecutive indices share one hash, but at a true width such as 50 a register quad straddles rows, so
//     every element hashes for itself (adt_keep);
//   * the reference-shaped <-> padded copy of the parameters (an index map, one element per thread).
// HBM-bound: float4 accesses, 16 lanes per row, block reduction in LDS and one atomic per column and block.
#pragma once
#include "adt_common.cuh"

namespace adt {

// struct Lanes {H, hd, hd_pad, sh; live(col); true_col(col)}: adt_common.cuh

struct LnLanesArgs {
  const float* X; int ldx;
  const float* gamma; const float* beta;
  float eps;
  float* Y; int ldy;
  int T;
  Lanes ln;
  const float* dY; int lddy;
  float* dX; int lddx; int acc;
  float* dgamma; float* dbeta;
};

constexpr int LN_LANES_THREADS = 256;

// KP = d_pad (64, 128, 192, 256): lane `sub` of a 16-lane group holds the float4s at columns q * 64 + 4 * sub.
template <int KP>
__global__ __launch_bounds__(LN_LANES_THREADS) void k_ln_lanes_fwd(LnLanesArgs a) {
  constexpr int E = KP / 16;
  const int sub = threadIdx.x & 15;
  constexpr int rows_per_block = LN_LANES_THREADS / 16;
  const float inv_d = 1.0f / (float)(a.ln.H * a.ln.hd);
  bool lv[E];
#pragma unroll
  for (int e = 0; e < E; ++e) lv[e] = a.ln.live((e / 4) * 64 + 4 * sub + (e & 3));
  for (int row = blockIdx.x * rows_per_block + (threadIdx.x >> 4); row < a.T; row += gridDim.x * rows_per_block) {
    float x[E];
#pragma unroll
    for (int e = 0; e < E; e += 4)
      *reinterpret_cast<float4*>(x + e) = *reinterpret_cast<const float4*>(a.X + (size_t)row * a.ldx + (e / 4) * 64 + 4 * sub);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) s += lv[e] ? x[e] : 0.f;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mu = s * inv_d;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) { x[e] = lv[e] ? x[e] - mu : 0.f; q += x[e] * x[e]; }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const float rstd = 1.0f / sqrtf(q * inv_d + a.eps);
#pragma unroll
    for (int e = 0; e < E; e += 4) {
      const int col = (e / 4) * 64 + 4 * sub;
      float gm[4], bt[4], y[4];
      *reinterpret_cast<float4*>(gm) = *reinterpret_cast<const float4*>(a.gamma + col);
      *reinterpret_cast<float4*>(bt) = *reinterpret_cast<const float4*>(a.beta + col);
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = lv[e + j] ? x[e + j] * rstd * gm[j] + bt[j] : 0.f;
      *reinterpret_cast<float4*>(a.Y + (size_t)row * a.ldy + col) = *reinterpret_cast<float4*>(y);
    }
  }
}

template <int KP>
__global__ __launch_bounds__(LN_LANES_THREADS) void k_ln_lanes_bwd(LnLanesArgs a) {
  constexpr int E = KP / 16;
  constexpr int rows_per_block = LN_LANES_THREADS / 16;
  __shared__ float sred[2][rows_per_block][KP];
  const int sub = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const float inv_d = 1.0f / (float)(a.ln.H * a.ln.hd);
  float dg[E] = {}, dbt[E] = {};
  float gm[E];
  bool lv[E];
#pragma unroll
  for (int e = 0; e < E; e += 4) *reinterpret_cast<float4*>(gm + e) = *reinterpret_cast<const float4*>(a.gamma + (e / 4) * 64 + 4 * sub);
#pragma unroll
  for (int e = 0; e < E; ++e) lv[e] = a.ln.live((e / 4) * 64 + 4 * sub + (e & 3));
  for (int row = blockIdx.x * rows_per_block + rg; row < a.T; row += gridDim.x * rows_per_block) {
    float x[E], dy[E];
#pragma unroll
    for (int e = 0; e < E; e += 4) {
      const int col = (e / 4) * 64 + 4 * sub;
      *reinterpret_cast<float4*>(x + e) = *reinterpret_cast<const float4*>(a.X + (size_t)row * a.ldx + col);
      *reinterpret_cast<float4*>(dy + e) = *reinterpret_cast<const float4*>(a.dY + (size_t)row * a.lddy + col);
    }
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) s += lv[e] ? x[e] : 0.f;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mu = s * inv_d;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) { x[e] = lv[e] ? x[e] - mu : 0.f; q += x[e] * x[e]; }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const float rstd = 1.0f / sqrtf(q * inv_d + a.eps);
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      x[e] *= rstd;                              // xhat (0 on pad lanes)
      dy[e] = lv[e] ? dy[e] : 0.f;
      dg[e] += dy[e] * x[e];
      dbt[e] += dy[e];
      dy[e] *= gm[e];                            // dxhat
      m1 += dy[e];
      m2 += dy[e] * x[e];
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) { m1 += __shfl_xor(m1, o, 64); m2 += __shfl_xor(m2, o, 64); }
    m1 *= inv_d;
    m2 *= inv_d;
#pragma unroll
    for (int e = 0; e < E; e += 4) {
      const int col = (e / 4) * 64 + 4 * sub;
      float* dst = a.dX + (size_t)row * a.lddx + col;
      float r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = lv[e + j] ? rstd * (dy[e + j] - m1 - x[e + j] * m2) : 0.f;
      if (a.acc) {                                 // pad lanes are written as +0.0 whatever the old dX held there
        float o[4];
        *reinterpret_cast<float4*>(o) = *reinterpret_cast<const float4*>(dst);
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] += lv[e + j] ? o[j] : 0.f;
      }
      *reinterpret_cast<float4*>(dst) = *reinterpret_cast<float4*>(r);
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int col = (e / 4) * 64 + 4 * sub + (e & 3);
    sred[0][rg][col] = dg[e];
    sred[1][rg][col] = dbt[e];
  }
  __syncthreads();
  for (int col = threadIdx.x; col < KP; col += LN_LANES_THREADS) {
    if (!a.ln.live(col)) continue;               // pad entries of dgamma / dbeta are never touched: they stay exact zeros
    float s0 = 0.f, s1 = 0.f;
    for (int r = 0; r < rows_per_block; ++r) { s0 += sred[0][r][col]; s1 += sred[1][r][col]; }
    atomicAdd(a.dgamma + col, s0);
    atomicAdd(a.dbeta + col, s1);
  }
}

// out[t][c] = live(c) ? (ids == NULL || ids[t] != 0) * (R[t][c] + R2[t][c] + keep(t, c) / (1 - p) * S[t][c]) : 0, keep indexed at the true
// width: (t + row_offset) * d + true_col(c).  Forward of a dropout site with its residuals and row mask (S = the layer's output), and --
// without residuals -- the gradient pulled back through the same site (S = dY).
struct DropLanesArgs {
  const float* S; int lds;
  const float* R; int ldr; const float* R2; int ldr2;
  const int* ids;
  float* out; int ldo;
  int T; Lanes ln; DropCfg drop; uint32_t row_offset;
};

__global__ __launch_bounds__(256) void k_drop_lanes(DropLanesArgs a) {
  const uint32_t key = drop_key(a.drop);
  const int dp = a.ln.H * a.ln.hd_pad, d = a.ln.H * a.ln.hd, V = dp / 4;
  const size_t n = (size_t)a.T * V;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int t = (int)(i / V), c4 = (int)(i % V) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (!a.ids || a.ids[t] != 0) {
      float s[4];
      *reinterpret_cast<float4*>(s) = *reinterpret_cast<const float4*>(a.S + (size_t)t * a.lds + c4);
      const uint32_t base = (uint32_t)(t + a.row_offset) * (uint32_t)d;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = c4 + j;
        if (!a.ln.live(c)) continue;
        float ks = 1.0f;
        if (a.drop.thr) ks = adt_keep(key, base + (uint32_t)a.ln.true_col(c), a.drop.thr) ? a.drop.scale : 0.f;
        v[j] = s[j] * ks;
      }
      if (a.R) {
        const float4 r = *reinterpret_cast<const float4*>(a.R + (size_t)t * a.ldr + c4);
        v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
      }
      if (a.R2) {
        const float4 r = *reinterpret_cast<const float4*>(a.R2 + (size_t)t * a.ldr2 + c4);
        v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = a.ln.live(c4 + j) ? v[j] : 0.f;
    }
    *reinterpret_cast<float4*>(a.out + (size_t)t * a.ldo + c4) = *reinterpret_cast<float4*>(v);
  }
}

// Fused drop-residual-normalise on padded lanes (BERT4Rec-ADT's repeating unit LN(dropout(dense(x)) + residual)), one pass per direction
// instead of k_drop_lanes + k_ln_lanes_*.  Geometry of k_ln_lanes_*: 16 lanes per row, float4 accesses, grid-stride over rows.
//   forward:  Z = live ? R + keep * scale * S : 0 (kept for the backward; may alias S), Y = LN_live(Z) * gamma + beta, pad lanes +0.0;
//   backward: dZ = LN backward of dY at Z, written (or accumulated) into dR; dS = keep * scale * dZ; dgamma / dbeta as k_ln_lanes_bwd.
// keep is indexed at the TRUE width, (t + row_offset) * d + true_col(c), every element hashing for itself (see the head of this file).
struct DrnLanesArgs {
  const float* S; int lds;
  const float* R; int ldr;
  const float* gamma; const float* beta;
  float eps;
  float* Z; int ldz;
  float* Y; int ldy;
  int T; Lanes ln; DropCfg drop; uint32_t row_offset;
  const float* dY; int lddy;
  float* dR; int lddr; int acc;
  float* dS; int ldds;
  float* dgamma; float* dbeta;
};

template <int KP>
__global__ __launch_bounds__(LN_LANES_THREADS) void k_drn_lanes_fwd(DrnLanesArgs a) {
  constexpr int E = KP / 16;
  constexpr int rows_per_block = LN_LANES_THREADS / 16;
  const int sub = threadIdx.x & 15;
  const int d = a.ln.H * a.ln.hd;
  const float inv_d = 1.0f / (float)d;
  const uint32_t key = drop_key(a.drop);
  bool lv[E];
  uint32_t tc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int col = (e / 4) * 64 + 4 * sub + (e & 3);
    lv[e] = a.ln.live(col);
    tc[e] = (uint32_t)a.ln.true_col(col);
  }
  for (int row = blockIdx.x * rows_per_block + (threadIdx.x >> 4); row < a.T; row += gridDim.x * rows_per_block) {
    float x[E], r[E];
#pragma unroll
    for (int e = 0; e < E; e += 4) {
      const int col = (e / 4) * 64 + 4 * sub;
      *reinterpret_cast<float4*>(x + e) = *reinterpret_cast<const float4*>(a.S + (size_t)row * a.lds + col);
      *reinterpret_cast<float4*>(r + e) = *reinterpret_cast<const float4*>(a.R + (size_t)row * a.ldr + col);
    }
    const uint32_t base = ((uint32_t)row + a.row_offset) * (uint32_t)d;
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      float ks = 1.0f;
      if (a.drop.thr) ks = (lv[e] && adt_keep(key, base + tc[e], a.drop.thr)) ? a.drop.scale : 0.f;
      x[e] = lv[e] ? r[e] + ks * x[e] : 0.f;
      s += x[e];
    }
#pragma unroll
    for (int e = 0; e < E; e += 4)
      *reinterpret_cast<float4*>(a.Z + (size_t)row * a.ldz + (e / 4) * 64 + 4 * sub) = *reinterpret_cast<float4*>(x + e);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mu = s * inv_d;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) { x[e] = lv[e] ? x[e] - mu : 0.f; q += x[e] * x[e]; }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const float rstd = 1.0f / sqrtf(q * inv_d + a.eps);
#pragma unroll
    for (int e = 0; e < E; e += 4) {
      const int col = (e / 4) * 64 + 4 * sub;
      float gm[4], bt[4], y[4];
      *reinterpret_cast<float4*>(gm) = *reinterpret_cast<const float4*>(a.gamma + col);
      *reinterpret_cast<float4*>(bt) = *reinterpret_cast<const float4*>(a.beta + col);
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = lv[e + j] ? x[e + j] * rstd * gm[j] + bt[j] : 0.f;
      *reinterpret_cast<float4*>(a.Y + (size_t)row * a.ldy + col) = *reinterpret_cast<float4*>(y);
    }
  }
}

template <int KP>
__global__ __launch_bounds__(LN_LANES_THREADS) void k_drn_lanes_bwd(DrnLanesArgs a) {
  constexpr int E = KP / 16;
  constexpr int rows_per_block = LN_LANES_THREADS / 16;
  __shared__ float sred[2][rows_per_block][KP];
  const int sub = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int d = a.ln.H * a.ln.hd;
  const float inv_d = 1.0f / (float)d;
  const uint32_t key = drop_key(a.drop);
  float dg[E] = {}, dbt[E] = {};
  float gm[E];
  bool lv[E];
#pragma unroll
  for (int e = 0; e < E; e += 4) *reinterpret_cast<float4*>(gm + e) = *reinterpret_cast<const float4*>(a.gamma + (e / 4) * 64 + 4 * sub);
#pragma unroll
  for (int e = 0; e < E; ++e) lv[e] = a.ln.live((e / 4) * 64 + 4 * sub + (e & 3));
  for (int row = blockIdx.x * rows_per_block + rg; row < a.T; row += gridDim.x * rows_per_block) {
    float x[E], dy[E];
#pragma unroll
    for (int e = 0; e < E; e += 4) {
      const int col = (e / 4) * 64 + 4 * sub;
      *reinterpret_cast<float4*>(x + e) = *reinterpret_cast<const float4*>(a.Z + (size_t)row * a.ldz + col);
      *reinterpret_cast<float4*>(dy + e) = *reinterpret_cast<const float4*>(a.dY + (size_t)row * a.lddy + col);
    }
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) s += lv[e] ? x[e] : 0.f;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mu = s * inv_d;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) { x[e] = lv[e] ? x[e] - mu : 0.f; q += x[e] * x[e]; }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const float rstd = 1.0f / sqrtf(q * inv_d + a.eps);
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      x[e] *= rstd;                              // xhat (0 on pad lanes)
      dy[e] = lv[e] ? dy[e] : 0.f;
      dg[e] += dy[e] * x[e];
      dbt[e] += dy[e];
      dy[e] *= gm[e];                            // dxhat
      m1 += dy[e];
      m2 += dy[e] * x[e];
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) { m1 += __shfl_xor(m1, o, 64); m2 += __shfl_xor(m2, o, 64); }
    m1 *= inv_d;
    m2 *= inv_d;
    const uint32_t base = ((uint32_t)row + a.row_offset) * (uint32_t)d;
#pragma unroll
    for (int e = 0; e < E; e += 4) {
      const int col = (e / 4) * 64 + 4 * sub;
      float* dst = a.dR + (size_t)row * a.lddr + col;
      float r[4], ds[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r[j] = lv[e + j] ? rstd * (dy[e + j] - m1 - x[e + j] * m2) : 0.f;      // dZ
        float ks = 1.0f;
        if (a.drop.thr) ks = (lv[e + j] && adt_keep(key, base + (uint32_t)a.ln.true_col(col + j), a.drop.thr)) ? a.drop.scale : 0.f;
        ds[j] = lv[e + j] ? ks * r[j] : 0.f;
      }
      *reinterpret_cast<float4*>(a.dS + (size_t)row * a.ldds + col) = *reinterpret_cast<float4*>(ds);
      if (a.acc) {                                 // pad lanes are written as +0.0 whatever the old dR held there
        float o[4];
        *reinterpret_cast<float4*>(o) = *reinterpret_cast<const float4*>(dst);
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] += lv[e + j] ? o[j] : 0.f;
      }
      *reinterpret_cast<float4*>(dst) = *reinterpret_cast<float4*>(r);
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int col = (e / 4) * 64 + 4 * sub + (e & 3);
    sred[0][rg][col] = dg[e];
    sred[1][rg][col] = dbt[e];
  }
  __syncthreads();
  for (int col = threadIdx.x; col < KP; col += LN_LANES_THREADS) {
    if (!a.ln.live(col)) continue;               // pad entries of dgamma / dbeta are never touched
    float s0 = 0.f, s1 = 0.f;
    for (int r = 0; r < rows_per_block; ++r) { s0 += sred[0][r][col]; s1 += sred[1][r][col]; }
    atomicAdd(a.dgamma + col, s0);
    atomicAdd(a.dbeta + col, s1);
  }
}

// Activation on padded lanes (STOSA-ADT: ELU after the embedding LayerNorm, ELU + 1 on every covariance -- and ELU(0) + 1 = 1, so the
// whole-row k_dropact would turn every pad lane into 1):
//   forward:  Y[t][c] = live(c) ? act(keep(t, c) / (1 - p) * X[t][c]) : +0.0           (act(dropout(x)), the order of k_dropact)
//   backward: dX[t][c] (+)= live(c) ? dY[t][c] * act'(u) * keep / (1 - p) : +0.0, pad lanes WRITTEN as +0.0 whatever dX or dY held there.
// keep is indexed at the true width, (t + row_offset) * d + true_col(c), every element hashing for itself (see the head of this file).
// Elementwise and HBM-bound as k_drop_lanes: one float4 per thread, any d_pad; a (T, n * d_pad) tensor of n padded rows side by side
// (the q / k / v projections) is n * T rows to this kernel when p = 0.
struct ActLanesArgs {
  const float* X; int ldx;
  const float* dY; int lddy;
  float* out; int ldo;          // Y, or dX
  int T; Lanes ln; DropCfg drop; uint32_t row_offset; int act; int acc;
};

template <bool BWD>
__global__ __launch_bounds__(256) void k_act_lanes(ActLanesArgs a) {
  const uint32_t key = drop_key(a.drop);
  const int dp = a.ln.H * a.ln.hd_pad, d = a.ln.H * a.ln.hd, V = dp / 4;
  const size_t n = (size_t)a.T * V;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int t = (int)(i / V), c4 = (int)(i % V) * 4;
    float x[4], dy[4] = {0.f, 0.f, 0.f, 0.f}, o[4] = {0.f, 0.f, 0.f, 0.f}, v[4];
    *reinterpret_cast<float4*>(x) = *reinterpret_cast<const float4*>(a.X + (size_t)t * a.ldx + c4);
    if constexpr (BWD) {
      *reinterpret_cast<float4*>(dy) = *reinterpret_cast<const float4*>(a.dY + (size_t)t * a.lddy + c4);
      if (a.acc) *reinterpret_cast<float4*>(o) = *reinterpret_cast<const float4*>(a.out + (size_t)t * a.ldo + c4);
    }
    const uint32_t base = (uint32_t)(t + a.row_offset) * (uint32_t)d;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c4 + j;
      v[j] = 0.f;
      if (!a.ln.live(c)) continue;
      float ks = 1.0f;
      if (a.drop.thr) ks = adt_keep(key, base + (uint32_t)a.ln.true_col(c), a.drop.thr) ? a.drop.scale : 0.f;
      const float u = x[j] * ks;
      if constexpr (BWD) v[j] = o[j] + dy[j] * act_grad(a.act, u) * ks;
      else v[j] = act_apply(a.act, u);
    }
    *reinterpret_cast<float4*>(a.out + (size_t)t * a.ldo + c4) = *reinterpret_cast<float4*>(v);
  }
}

// compact[i] = padded[map[i]] (gather) / padded[map[i]] = compact[i] (scatter; the map is injective): the reference-shaped copy of the
// parameters or of an optimizer moment against the padded flat buffer the kernels compute on.
struct LaneMapArgs { float* padded; float* compact; const int* map; size_t n; int scatter; };

__global__ __launch_bounds__(256) void k_lane_map(LaneMapArgs a) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (size_t)gridDim.x * 256) {
    if (a.scatter) a.padded[a.map[i]] = a.compact[i];
    else a.compact[i] = a.padded[a.map[i]];
  }
}

}  // namespace adt
