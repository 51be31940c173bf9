// STOSA-ADT with distance_metric='kl': KL-divergence attention (stosa/modules.py:52-70 kl_distance_matmul as used at :244-248
// and :333-337), the BPR / positive-vs-negative loss on row-wise KL divergences (stosa/trainer.py:358-391 with kl_distance,
// modules.py:45-50) and the chunked full-sort score (kl_predict_full, trainer.py:481-511).  Exact fp32 on the vector ALUs,
// organised like the Wasserstein kernels of adt_stosa.cuh (one workgroup per (sequence, head), one wave per query row in the
// forward and pass A, one wave per key row in pass B), which it shares its LDS layout, dead-row rule and dropout indices with.
//
// kl_distance_matmul broadcasts elementwise where the shapes allow it, and Lq == Lk, so per (sequence, head):
//   KL_ij = 0.5 (sum_d log ck_jd - sum_d log cq_id + sum_d (mq_id - mk_id)^2 / ck_jd + sum_d cq_jd / ck_id - hd)
// i.e. the MEAN term takes the key row i (not j) and the TRACE term is transposed.  The cross terms are one inner product of a
// row image and a column image:
//   X_i = [(mq_i - mk_i)^2 | 1/ck_i]  (built from key row i even where key i is padding: the mask acts on columns only)
//   Y_j = [1/ck_j | cq_j]
//   s_ij = -(0.5 ((colbias_j - rowbias_i) + X_i.Y_j - hd)) / sqrt(hd) + A_ij,  colbias = sum log ck, rowbias = sum log cq
// log(prod c) is taken as sum(log c): equal to 3e-6 at the fixture shapes, and free of the product's fp32 overflow.
// Covered shapes: exactly those of k_wattn_fwd / k_wattn_bwd (hd 16/32/64, L <= 256, LDS <= 160 KB): the log-det biases live in
// the padding column (index hd) of the [L][hd+1] image rows, so the LDS footprint is wattn_lds_bytes().  These are the fallback of the
// matrix-core KL kernels (adt_wattn_mfma.cuh, MET = WM_KL: hd 16 / 32, L <= 128), like k_wattn_fwd / k_wattn_bwd for Wasserstein.
#pragma once
#include "adt_stosa.cuh"

namespace adt {

// sum_d log c[d] over one row, by the 16 lanes that share (lane & 15) and in one fixed order (per-lane strided partial sums,
// then an xor tree): the forward, pass A and pass B all obtain the row bias from this function, so that every recomputation
// of a score is bit-identical (see w_pair_x on why that matters for fully masked rows).  hl: the live lanes of the head (hd, or hd_live of
// a padded head, whose pad lanes hold cov = 0 and stay out of the sum: log 0 = -inf).
ADT_DEVICE_INLINE float kl_row_logsum(const float* g, int hl, int sub) {
  float part = 0.f;
  for (int c = sub; c < hl; c += 16) part += logf(g[c]);
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  return part;
}

// 1 / c on a live lane, +0.0 on a pad lane (c = 0 there): a select on the lane index, never a product with zero (0 * inf = NaN)
ADT_DEVICE_INLINE float kl_inv(float c, bool live) { return live ? 1.0f / c : 0.f; }

// stage the column images of a head slice: y1[r] = 1/ck_r (+ colbias_r at index hd), y2[r] = cq_r
ADT_DEVICE_INLINE void kl_stage_y(float* y1, float* y2, const float* Kc, int ldkc, const float* Qc, int ldqc, int L, int hd, int hl) {
  const int RS = hd + 1, sub = threadIdx.x & 15;
  for (int r = threadIdx.x >> 4; r < L; r += 16) {
    for (int c = sub; c < hd; c += 16) {
      y1[r * RS + c] = kl_inv(Kc[(size_t)r * ldkc + c], c < hl);
      y2[r * RS + c] = Qc[(size_t)r * ldqc + c];
    }
    const float lb = kl_row_logsum(Kc + (size_t)r * ldkc, hl, sub);
    if (sub == 0) y1[r * RS + hd] = lb;
  }
}

// stage the row images: x1[r] = (mq_r - mk_r)^2 (+ rowbias_r at index hd), x2[r] = 1/ck_r
ADT_DEVICE_INLINE void kl_stage_x(float* x1, float* x2, const float* Qm, int ldqm, const float* Km, int ldkm, const float* Qc, int ldqc,
                                  const float* Kc, int ldkc, int L, int hd, int hl) {
  const int RS = hd + 1, sub = threadIdx.x & 15;
  for (int r = threadIdx.x >> 4; r < L; r += 16) {
    for (int c = sub; c < hd; c += 16) {
      const float df = Qm[(size_t)r * ldqm + c] - Km[(size_t)r * ldkm + c];
      x1[r * RS + c] = df * df;
      x2[r * RS + c] = kl_inv(Kc[(size_t)r * ldkc + c], c < hl);
    }
    const float lb = kl_row_logsum(Qc + (size_t)r * ldqc, hl, sub);
    if (sub == 0) x1[r * RS + hd] = lb;
  }
}

// one wave's own row image (lanes < hd write the features; every lane returns the row bias)
ADT_DEVICE_INLINE float kl_wave_x(float* x1, float* x2, const float* qm, const float* km, const float* qc, const float* kc, int hd, int hl, int lane) {
  for (int c = lane; c < hd; c += 64) {
    const float df = qm[c] - km[c];
    x1[c] = df * df;
    x2[c] = kl_inv(kc[c], c < hl);
  }
  return kl_row_logsum(qc, hl, lane & 15);
}

ADT_DEVICE_INLINE float kl_wave_y(float* y1, float* y2, const float* kc, const float* qc, int hd, int hl, int lane) {
  for (int c = lane; c < hd; c += 64) {
    y1[c] = kl_inv(kc[c], c < hl);
    y2[c] = qc[c];
  }
  return kl_row_logsum(kc, hl, lane & 15);
}

// the scaled negative KL of one (query, key) pair: one fixed sequence of operations for the forward and both backward passes.
// hl: the true head size the divergence subtracts (the pad lanes of a padded head add fmaf(0, 0, t) = t to both sums).
ADT_DEVICE_INLINE float kl_pair_x(const float* x1, const float* x2, const float* y1, const float* y2, float rowb, float colb, int hd, int hl,
                                  float sq_hd) {
  float t = 0.f, u = 0.f;
  for (int d0 = 0; d0 < hd; ++d0) {
    t = fmaf(x1[d0], y1[d0], t);
    u = fmaf(x2[d0], y2[d0], u);
  }
  const float kl = 0.5f * ((((colb - rowb) + t) + u) - (float)hl);
  return (-kl) / sq_hd;
}

// LN: padded heads (the adt_klattn_scaled_* entry points): hl = hd_live live lanes and the given scale.  <false> is the kernel as it
// always was (hl = hd and sqrt(hd) fold into it: 86 / 128 VGPRs, 5 / 4 waves per SIMD).  <true> carries (256, 5) / (256, 4): the two
// extra scalars tip the allocator's occupancy heuristic one step down without the bound (112 / 129 VGPRs); with it the kernels stay at
// 85 / 128 and scratch 0.  The LDS footprint decides how many workgroups are resident, not this.
template <bool LN>
__global__ __launch_bounds__(256, LN ? 5 : 1) void k_klattn_fwd(WAttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int L = a.L, hd = a.hd, hl = LN ? a.hd_live : hd, RS = hd + 1, Lp = (L + 63) / 64 * 64;
  float* sY1 = smem;                 // [L][RS] 1/ck_j, colbias_j at [hd]
  float* sY2 = sY1 + L * RS;         // cq_j
  float* sVm = sY2 + L * RS;
  float* sVc = sVm + L * RS;
  float* sDead = sVc + L * RS;       // [Lp]
  float* sKv = sDead + Lp;           // [Lp]
  float* sWave = sKv + Lp;           // per wave: P row [Lp], P^2 row [Lp], (unused) [Lp], X1 [hd], X2 [hd], 2*hd spare
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t row_b = (size_t)b * L;
  for (int i = threadIdx.x; i < Lp; i += 256) sKv[i] = (i < L && a.kid[row_b + i] > 0) ? 1.f : 0.f;
  __syncthreads();
  w_mark_dead(sDead, sKv, L, Lp);
  kl_stage_y(sY1, sY2, a.Kc + row_b * a.ldkc + h * hd, a.ldkc, a.Qc + row_b * a.ldqc + h * hd, a.ldqc, L, hd, hl);
  w_stage<false, false>(sVm, a.Vm + row_b * a.ldvm + h * hd, a.ldvm, L, hd, nullptr);
  w_stage<false, false>(sVc, a.Vc + row_b * a.ldvc + h * hd, a.ldvc, L, hd, nullptr);
  __syncthreads();
  float* sP = sWave + w * (3 * Lp + 4 * hd);
  float* sP2 = sP + Lp;
  float* sX1 = sP + 3 * Lp;
  float* sX2 = sX1 + hd;
  const uint32_t key_rng = drop_key(a.drop);
  const float sq_hd = LN ? w_sq_hd(a) : sqrtf((float)hd);
  const int nd = 64 / hd >= 1 ? hd : 64;
  const int nparts = 64 / nd;
  for (int i = w; i < L; i += 4) {
    const size_t r = row_b + i;
    const float rowb = kl_wave_x(sX1, sX2, a.Qm + r * a.ldqm + h * hd, a.Km + r * a.ldkm + h * hd, a.Qc + r * a.ldqc + h * hd,
                                 a.Kc + r * a.ldkc + h * hd, hd, hl, lane);
    const bool dead_i = sDead[i] != 0.f;
    float s[W_KPL];
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < W_KPL; ++t) {
      const int j = lane + 64 * t;
      s[t] = -INFINITY;
      if (j < L) {
        s[t] = w_score(kl_pair_x(sX1, sX2, sY1 + j * RS, sY2 + j * RS, rowb, sY1[j * RS + hd], hd, hl, sq_hd), j > i || sKv[j] == 0.f, dead_i);
        m = fmaxf(m, s[t]);
      }
    }
    m = wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < W_KPL; ++t) {
      const int j = lane + 64 * t;
      if (j < L) { s[t] = expf(s[t] - m); sum += s[t]; }
    }
    sum = wave_sum(sum);
    const float inv = 1.0f / sum;
    if (lane == 0) a.LSE[(size_t)bh * L + i] = m + logf(sum);
    const uint32_t idx_q = ((uint32_t)(bh + a.bh_offset) * (uint32_t)L + (uint32_t)i) * (uint32_t)L;
#pragma unroll
    for (int t = 0; t < W_KPL; ++t) {
      const int j = lane + 64 * t;
      if (j < Lp) {
        float p = 0.f;
        if (j < L) {
          p = s[t] * inv;
          if (a.drop.thr) p = adt_keep(key_rng, idx_q + (uint32_t)j, a.drop.thr) ? p * a.drop.scale : 0.f;
        }
        sP[j] = p;
        sP2[j] = p * p;
      }
    }
    const int part = lane / nd;
    for (int d0 = lane % nd; d0 < hd; d0 += nd) {
      float cm = 0.f, cc = 0.f;
      for (int j = part; j < L; j += nparts) {
        cm += sP[j] * sVm[j * RS + d0];
        cc += sP2[j] * sVc[j * RS + d0];
      }
      for (int o = nd; o < 64; o <<= 1) { cm += __shfl_xor(cm, o, 64); cc += __shfl_xor(cc, o, 64); }
      if (part == 0) {
        a.Om[r * a.ldom + h * hd + d0] = cm;
        a.Oc[r * a.ldoc + h * hd + d0] = cc;
      }
    }
  }
}

// Backward.  g_ij = dloss/dKL_ij = -dS_ij / sqrt(hd).  Pass A (column images resident, wave owns query row i):
//   dmq_i = (mq_i - mk_i) * sum_j g_ij / ck_j,   dmk_i = -dmq_i         (the mean term reads key row i)
//   dck_i = -0.5 / ck_i^2 * sum_j g_ij cq_j      (trace term, row side)
//   dcq_i = -0.5 / cq_i * sum_j g_ij             (row log-det; sum_j g_ij vanishes up to rounding)
// pass B (row images resident, wave owns key j):
//   dck_j += 0.5 / ck_j * sum_i g_ij - 0.5 / ck_j^2 * sum_i g_ij (mq_i - mk_i)^2   (column log-det, mean term)
//   dcq_j += 0.5 * sum_i g_ij / ck_i                                              (trace term, column side)
//   dVm_j, dVc_j as in k_wattn_bwd.
// Row i of pass A and row j = i of pass B are handled by the same wave and lane, so the pass-B read-add-write of dKc / dQc
// sees pass A's value in program order: a fixed summation order, no atomics.
template <bool LN>
__global__ __launch_bounds__(256, LN ? 4 : 1) void k_klattn_bwd(WAttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int L = a.L, hd = a.hd, hl = LN ? a.hd_live : hd, RS = hd + 1, Lp = (L + 63) / 64 * 64;      // lanes at and above hl: zero padding, +0.0 gradients
  float* sA0 = smem;                 // phase A: Y1 (colbias at [hd]) | phase B: X1 (rowbias at [hd])
  float* sA1 = sA0 + L * RS;         // phase A: Y2                   | phase B: X2
  float* sA2 = sA1 + L * RS;         // phase A: Vm                   | phase B: dOm
  float* sA3 = sA2 + L * RS;         // phase A: Vc                   | phase B: dOc
  float* sKv = sA3 + L * RS;
  float* sDelta = sKv + Lp;
  float* sLse = sDelta + Lp;
  float* sDead = sLse + Lp;
  float* sWave = sDead + Lp;
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t row_b = (size_t)b * L;
  const float sq_hd = LN ? w_sq_hd(a) : sqrtf((float)hd);
  const uint32_t key_rng = drop_key(a.drop);
  const uint32_t idx_bh = (uint32_t)(bh + a.bh_offset) * (uint32_t)L;
  const int nd = 64 / hd >= 1 ? hd : 64;
  const int nparts = 64 / nd;
  float* sR0 = sWave + w * (3 * Lp + 4 * hd);
  float* sR1 = sR0 + Lp;
  float* sR2 = sR1 + Lp;
  float* sV0 = sR0 + 3 * Lp;
  float* sV1 = sV0 + hd;
  float* sV2 = sV1 + hd;
  float* sV3 = sV2 + hd;
  const int co = h * hd;

  for (int i = threadIdx.x; i < Lp; i += 256) {
    sKv[i] = (i < L && a.kid[row_b + i] > 0) ? 1.f : 0.f;
    sLse[i] = i < L ? a.LSE[(size_t)bh * L + i] : INFINITY;
    sDelta[i] = 0.f;
  }
  kl_stage_y(sA0, sA1, a.Kc + row_b * a.ldkc + co, a.ldkc, a.Qc + row_b * a.ldqc + co, a.ldqc, L, hd, hl);
  w_stage<false, false>(sA2, a.Vm + row_b * a.ldvm + co, a.ldvm, L, hd, nullptr);
  w_stage<false, false>(sA3, a.Vc + row_b * a.ldvc + co, a.ldvc, L, hd, nullptr);
  __syncthreads();
  w_mark_dead(sDead, sKv, L, Lp);
  __syncthreads();

  // ---- pass A ---------------------------------------------------------------------------------------------------
  for (int i = w; i < L; i += 4) {
    const size_t r = row_b + i;
    const float rowb = kl_wave_x(sV0, sV1, a.Qm + r * a.ldqm + co, a.Km + r * a.ldkm + co, a.Qc + r * a.ldqc + co, a.Kc + r * a.ldkc + co,
                                 hd, hl, lane);
    for (int d0 = lane; d0 < hd; d0 += 64) {
      sV2[d0] = a.dOm[r * a.lddom + co + d0];
      sV3[d0] = a.dOc[r * a.lddoc + co + d0];
    }
    const float lse = sLse[i];
    const bool dead_i = sDead[i] != 0.f;
    const uint32_t idx_q = (idx_bh + (uint32_t)i) * (uint32_t)L;
    float p[W_KPL], dp[W_KPL];
    float delta = 0.f;
#pragma unroll
    for (int t = 0; t < W_KPL; ++t) {
      const int j = lane + 64 * t;
      p[t] = 0.f; dp[t] = 0.f;
      if (j < L) {
        float gm = 0.f, gc = 0.f;
        for (int d0 = 0; d0 < hd; ++d0) {
          gm += sV2[d0] * sA2[j * RS + d0];
          gc += sV3[d0] * sA3[j * RS + d0];
        }
        const float sv = w_score(kl_pair_x(sV0, sV1, sA0 + j * RS, sA1 + j * RS, rowb, sA0[j * RS + hd], hd, hl, sq_hd), j > i || sKv[j] == 0.f, dead_i);
        const float pr = expf(sv - lse);
        float ks_ = 1.0f;
        if (a.drop.thr) ks_ = adt_keep(key_rng, idx_q + (uint32_t)j, a.drop.thr) ? a.drop.scale : 0.f;
        const float pd = pr * ks_;
        p[t] = pr;
        dp[t] = (gm + 2.0f * pd * gc) * ks_;
        delta += pr * dp[t];
      }
    }
    delta = wave_sum(delta);
    if (lane == 0) sDelta[i] = delta;
    float gsum = 0.f;
#pragma unroll
    for (int t = 0; t < W_KPL; ++t) {
      const int j = lane + 64 * t;
      if (j < Lp) {
        const float gv = j < L ? -(p[t] * (dp[t] - delta)) / sq_hd : 0.f;
        sR0[j] = gv;
        gsum += gv;
      }
    }
    gsum = wave_sum(gsum);
    const int part = lane / nd;
    for (int d0 = lane % nd; d0 < hd; d0 += nd) {
      float am = 0.f, as = 0.f;
      for (int j = part; j < L; j += nparts) {
        am += sR0[j] * sA0[j * RS + d0];
        as += sR0[j] * sA1[j * RS + d0];
      }
      for (int o = nd; o < 64; o <<= 1) { am += __shfl_xor(am, o, 64); as += __shfl_xor(as, o, 64); }
      if (part == 0) {
        const float df = a.Qm[r * a.ldqm + co + d0] - a.Km[r * a.ldkm + co + d0];
        const float x2 = sV1[d0];
        const bool lv = d0 < hl;
        a.dQm[r * a.ldd + co + d0] = lv ? df * am : 0.f;
        a.dKm[r * a.ldd + co + d0] = lv ? -(df * am) : 0.f;
        a.dKc[r * a.ldd + co + d0] = lv ? -0.5f * x2 * x2 * as : 0.f;
        a.dQc[r * a.ldd + co + d0] = lv ? -0.5f * gsum / a.Qc[r * a.ldqc + co + d0] : 0.f;      // cq = 0 on a pad lane
      }
    }
  }

  // ---- phase B staging: the row images and dO over the same LDS ------------------------------------------------------
  __syncthreads();
  kl_stage_x(sA0, sA1, a.Qm + row_b * a.ldqm + co, a.ldqm, a.Km + row_b * a.ldkm + co, a.ldkm, a.Qc + row_b * a.ldqc + co, a.ldqc,
             a.Kc + row_b * a.ldkc + co, a.ldkc, L, hd, hl);
  w_stage<false, false>(sA2, a.dOm + row_b * a.lddom + co, a.lddom, L, hd, nullptr);
  w_stage<false, false>(sA3, a.dOc + row_b * a.lddoc + co, a.lddoc, L, hd, nullptr);
  __syncthreads();

  // ---- pass B: wave owns key j, lanes over queries i ------------------------------------------------------------------
  for (int j = w; j < L; j += 4) {
    const size_t r = row_b + j;
    const float colb = kl_wave_y(sV0, sV1, a.Kc + r * a.ldkc + co, a.Qc + r * a.ldqc + co, hd, hl, lane);
    for (int d0 = lane; d0 < hd; d0 += 64) {
      sV2[d0] = a.Vm[r * a.ldvm + co + d0];
      sV3[d0] = a.Vc[r * a.ldvc + co + d0];
    }
    const bool key_pad = sKv[j] == 0.f;
    float gsum = 0.f;
#pragma unroll
    for (int t = 0; t < W_KPL; ++t) {
      const int i = lane + 64 * t;
      if (i < Lp) {
        float gv = 0.f, pd = 0.f;
        if (i < L) {
          float gm = 0.f, gc = 0.f;
          for (int d0 = 0; d0 < hd; ++d0) {
            gm += sA2[i * RS + d0] * sV2[d0];
            gc += sA3[i * RS + d0] * sV3[d0];
          }
          const float sv = w_score(kl_pair_x(sA0 + i * RS, sA1 + i * RS, sV0, sV1, sA0[i * RS + hd], colb, hd, hl, sq_hd), j > i || key_pad,
                                   sDead[i] != 0.f);
          const float pr = expf(sv - sLse[i]);
          float ks_ = 1.0f;
          if (a.drop.thr) ks_ = adt_keep(key_rng, (idx_bh + (uint32_t)i) * (uint32_t)L + (uint32_t)j, a.drop.thr) ? a.drop.scale : 0.f;
          pd = pr * ks_;
          const float dpr = (gm + 2.0f * pd * gc) * ks_;
          gv = -(pr * (dpr - sDelta[i])) / sq_hd;
        }
        sR0[i] = gv;
        sR1[i] = pd;
        sR2[i] = pd * pd;
        gsum += gv;
      }
    }
    gsum = wave_sum(gsum);
    const int part = lane / nd;
    for (int d0 = lane % nd; d0 < hd; d0 += nd) {
      float bm = 0.f, bs = 0.f, vm = 0.f, vc = 0.f;
      for (int i = part; i < L; i += nparts) {
        bm += sR0[i] * sA0[i * RS + d0];
        bs += sR0[i] * sA1[i * RS + d0];
        vm += sR1[i] * sA2[i * RS + d0];
        vc += sR2[i] * sA3[i * RS + d0];
      }
      for (int o = nd; o < 64; o <<= 1) {
        bm += __shfl_xor(bm, o, 64); bs += __shfl_xor(bs, o, 64);
        vm += __shfl_xor(vm, o, 64); vc += __shfl_xor(vc, o, 64);
      }
      if (part == 0) {
        const float y1 = sV0[d0];
        const bool lv = d0 < hl;
        a.dKc[r * a.ldd + co + d0] = lv ? a.dKc[r * a.ldd + co + d0] + (0.5f * gsum * y1 - 0.5f * bm * y1 * y1) : 0.f;
        a.dQc[r * a.ldd + co + d0] = lv ? a.dQc[r * a.ldd + co + d0] + 0.5f * bs : 0.f;
        a.dVm[r * a.ldd + co + d0] = lv ? vm : 0.f;
        a.dVc[r * a.ldd + co + d0] = lv ? vc : 0.f;
      }
    }
  }
}

// ---- BPR + positive-vs-negative loss on row-wise KL divergences (stosa/trainer.py:358-391, kl_distance modules.py:45-50) ----
//   KL(a||b) = 0.5 (sum c_a / c_b + sum (m_b - m_a)^2 / c_b - d + sum log c_b - sum log c_a)
//   pos = KL(seq||pos), neg = KL(seq||neg), pvn = KL(pos||neg); item covariances through ELU(.)+1.  Arguments as k_wdist_bpr.
// LN: rows and tables are padded (a.ln, d = H * hd_pad).  A pad lane holds a sequence covariance 0 (1 / sc, log sc) and an item covariance
// ELU(0) + 1 = 1, so it is skipped by its index in every sum and log, the divergences subtract the true d, dSm / dSc get +0.0 there and the
// tables' pad lanes receive no atomic.
template <bool LN>
__global__ __launch_bounds__(256) void k_kldist_bpr(WBprArgs a) {
  const int lane = threadIdx.x & 63;
  const float wgt = *a.inv_count;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  const float fd = LN ? (float)(a.ln.H * a.ln.hd) : (float)a.d;
  float l_bpr = 0.f, l_pvn = 0.f, l_auc = 0.f;
  for (int t = wave; t < a.T; t += nwaves) {
    const int ip = a.pos[t], in = a.neg[t];
    const bool tgt = ip > 0;
    float tp = 0.f, mp = 0.f, tn = 0.f, mn = 0.f, tpn = 0.f, mpn = 0.f, ls = 0.f, lp = 0.f, ln = 0.f;
    if (tgt) {
      for (int c = lane; c < a.d; c += 64) {
        if (LN && !a.ln.live(c)) continue;
        const float sm = a.Sm[(size_t)t * a.lds + c], sc = a.Sc[(size_t)t * a.lds + c];
        const float pm = a.Em[(size_t)ip * a.d + c], pc = w_elu1(a.Ec[(size_t)ip * a.d + c]);
        const float nm = a.Em[(size_t)in * a.d + c], nc = w_elu1(a.Ec[(size_t)in * a.d + c]);
        tp += sc / pc; mp += (pm - sm) / pc * (pm - sm);
        tn += sc / nc; mn += (nm - sm) / nc * (nm - sm);
        tpn += pc / nc; mpn += (nm - pm) / nc * (nm - pm);
        ls += logf(sc); lp += logf(pc); ln += logf(nc);
      }
    }
    tp = wave_sum(tp); mp = wave_sum(mp); tn = wave_sum(tn); mn = wave_sum(mn); tpn = wave_sum(tpn); mpn = wave_sum(mpn);
    ls = wave_sum(ls); lp = wave_sum(lp); ln = wave_sum(ln);
    const float dp = (tp + mp - fd + (lp - ls)) * 0.5f;
    const float dn = (tn + mn - fd + (ln - ls)) * 0.5f;
    const float dpn = (tpn + mpn - fd + (ln - lp)) * 0.5f;
    float g_pos = 0.f, g_neg = 0.f, g_pvn = 0.f;
    if (tgt) {
      const float x = dn - dp + 1e-24f;
      const float sg = 1.0f / (1.0f + expf(-x));
      l_bpr += -logf(sg) * wgt;
      const float hinge = dp - dpn;
      l_pvn += a.pvn_weight * fmaxf(hinge, 0.f) * wgt;
      l_auc += ((dn - dp) > 0.f ? 1.f : ((dn - dp) == 0.f ? 0.5f : 0.f)) * wgt;
      const float gx = -(1.0f - sg) * wgt;
      const float gh = hinge >= 0.f ? a.pvn_weight * wgt : 0.f;
      g_neg = gx;
      g_pos = -gx + gh;
      g_pvn = -gh;
    }
    for (int c = lane; c < a.d; c += 64) {
      float dsm = 0.f, dsc = 0.f;
      if (tgt && (!LN || a.ln.live(c))) {
        const float sm = a.Sm[(size_t)t * a.lds + c], sc = a.Sc[(size_t)t * a.lds + c];
        const float pe = a.Ec[(size_t)ip * a.d + c], ne = a.Ec[(size_t)in * a.d + c];
        const float pm = a.Em[(size_t)ip * a.d + c], pc = w_elu1(pe);
        const float nm = a.Em[(size_t)in * a.d + c], nc = w_elu1(ne);
        const float ipc = 1.0f / pc, inc = 1.0f / nc, isc = 1.0f / sc;
        const float dps = pm - sm, dns = nm - sm, dnp = nm - pm;
        // d KL(a||b): dm_a = -(m_b - m_a)/c_b, dm_b = (m_b - m_a)/c_b, dc_a = 0.5 (1/c_b - 1/c_a),
        //             dc_b = 0.5 (1/c_b - c_a/c_b^2 - (m_b - m_a)^2/c_b^2)
        dsm = -g_pos * dps * ipc - g_neg * dns * inc;
        dsc = 0.5f * g_pos * (ipc - isc) + 0.5f * g_neg * (inc - isc);
        const float dpm = g_pos * dps * ipc - g_pvn * dnp * inc;
        const float dpc = 0.5f * g_pos * (ipc - sc * ipc * ipc - dps * dps * ipc * ipc) + 0.5f * g_pvn * (inc - ipc);
        const float dnm = g_neg * dns * inc + g_pvn * dnp * inc;
        const float dnc = 0.5f * g_neg * (inc - sc * inc * inc - dns * dns * inc * inc) + 0.5f * g_pvn * (inc - pc * inc * inc - dnp * dnp * inc * inc);
        atomicAdd(a.dEm + (size_t)ip * a.d + c, dpm);
        atomicAdd(a.dEc + (size_t)ip * a.d + c, dpc * w_elu_grad(pe));
        if (in > 0) {
          atomicAdd(a.dEm + (size_t)in * a.d + c, dnm);
          atomicAdd(a.dEc + (size_t)in * a.d + c, dnc * w_elu_grad(ne));
        }
      }
      a.dSm[(size_t)t * a.ldds + c] = dsm;
      a.dSc[(size_t)t * a.ldds + c] = dsc;
    }
  }
  if (lane == 0) {
    const int slot = wave & 63;
    if (l_bpr != 0.f) atomicAdd(a.loss3 + slot, l_bpr);
    if (l_pvn != 0.f) atomicAdd(a.loss3 + 64 + slot, l_pvn);
    if (l_auc != 0.f) atomicAdd(a.loss3 + 128 + slot, l_auc);
  }
}

// ---- full-sort scores of one eval batch (kl_predict_full, stosa/trainer.py:481-511) ---------------------------------------
// The reference pads the item table to a multiple of the batch size E = B (zero means, unit covariances) and calls
// kl_distance_matmul on the B users against each B-item chunk; with its broadcasts, for item v = cE + j and a = cE + u:
//   dist[u][v] = 0.5 (sum log ci_v - sum log cu_u + sum (mu_u - mi_a)^2 / ci_v + sum cu_j / ci_a - d)
// (item a >= V is a padding item).  16 lanes per (user, item) pair.  LN: padded rows and tables (a.ln), the pad lanes skipped by their
// index (cu = 0 there, and ELU(0) + 1 = 1 on the item side) and the true d subtracted.
template <bool LN>
__global__ __launch_bounds__(256) void k_kldist_full(WFullArgs a) {
  const int sub = threadIdx.x & 15;
  const size_t n = (size_t)a.B * a.V;
  for (size_t i = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4); i < n; i += (size_t)gridDim.x * 16) {
    const int u = (int)(i / a.V), v = (int)(i % a.V);
    const int ch = v / a.B, j = v - ch * a.B, ia = ch * a.B + u;
    const bool real_a = ia < a.V;
    float lv = 0.f, lu = 0.f, mc = 0.f, tr = 0.f;
    for (int c = sub; c < a.d; c += 16) {
      if (LN && !a.ln.live(c)) continue;
      const float cv = w_elu1(a.Ec[(size_t)v * a.d + c]);
      const float ma = real_a ? a.Em[(size_t)ia * a.d + c] : 0.f;
      const float ca = real_a ? w_elu1(a.Ec[(size_t)ia * a.d + c]) : 1.f;
      const float mu = a.Sm[(size_t)u * a.lds + c], cu = a.Sc[(size_t)u * a.lds + c], cj = a.Sc[(size_t)j * a.lds + c];
      lv += logf(cv);
      lu += logf(cu);
      mc += (mu - ma) * (mu - ma) / cv;
      tr += cj / ca;
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      lv += __shfl_xor(lv, o, 64); lu += __shfl_xor(lu, o, 64);
      mc += __shfl_xor(mc, o, 64); tr += __shfl_xor(tr, o, 64);
    }
    if (sub == 0) a.dist[(size_t)u * a.ldo + v] = 0.5f * ((((lv - lu) + mc) + tr) - (LN ? (float)(a.ln.H * a.ln.hd) : (float)a.d));
  }
}

}  // namespace adt
