// STOSA-ADT distance attention (Wasserstein and KL divergence) for sequences of 1 <= L <= 1024 rows at head size 16 / 32 / 64, on the matrix
// cores in either precision.  The scheme is adt_attn_long.cuh's: grid (B*H, groups of four 16-row tiles), one tile per wave; the forward
// streams key chunks past the query tiles with an online softmax; the backward streams key chunks past the dQ tiles (pass A), then query
// chunks past the dK / dV tiles (pass B), P recomputed from the forward's LSE; every gradient element has one writer, no atomics.  The
// arithmetic is adt_wattn_mfma.cuh's, through its own staging and fragment helpers applied to a chunk instead of the whole sequence: one
// cross term of inner width 2 hd over [m | sqrt S] (KL: the X / Y images with their log-det biases), contexts P~ Vm and (P~ * P~) Vc,
// dP~ = dOm Vm^T + 2 P~ (dOc Vc^T), the sqrt(clamp(cov, 1e-24)) chain, and the KL gradient split between pass A and pass B with the same
// lane (same workgroup, same wave: tile = blockIdx.y * 4 + wave in both passes) adding in the same order.  A separate header and
// translation unit: the kernels of the shorter lengths are not touched.  adt_wattn_hd128.hip instantiates the same templates at head size 128 (one wave per
// SIMD, the whole 512-entry register file).
//
// What streaming changes:
//  * Online softmax.  The dropout keep scale multiplies the unnormalised probability BEFORE the square, so when the running maximum
//    moves by alpha = exp(m_old - m_new) the mean accumulator is rescaled by alpha and the covariance accumulator by alpha^2, and the
//    final normalisation is 1 / sum and 1 / sum^2.
//  * Per-sequence state.  Key validity is one byte per key; the per-query dead flags become the index f of the sequence's first valid
//    key (L: none): the attention is causal, so query i has no attendable key exactly when i < f.
//  * The dead-row rule.  A dead query attends to ALL L keys with scores quantised by (x + W_MASK) - W_MASK (adt_stosa_args.cuh: w_score) and
//    keeps its gradient; a masked key of a live query contributes exp(x - 2^32 - lse) = 0 exactly.  So a 16-row tile none of whose
//    queries is dead (16 * tile >= f) skips the key tiles above its diagonal; a tile that holds a dead query visits every key.  Pass B's key
//    tile visits the query rows [0, f) (dead, they attend to it) and [16 * tile, L) and skips what lies between.  The staging loops skip a
//    chunk only when that rule lets every wave of the workgroup skip it.
//  * The score x of a pair is produced by the same instruction sequence on the same operand values in the forward, pass A and pass B (see
//    the head of adt_wattn_mfma.cuh): the chunk images go through wm_stage_cat / wm_kl_stage, the owned tiles through wm_cat_frag /
//    wm_kl_frag and wm_row_norm / wm_kl_logsum, exactly as in the resident kernels.
#pragma once
#include "adt_attn_long.cuh"      // attn_long_masks
#include "adt_wide_plan.h"       // ATTN_LONG_LMAX
#include "adt_wattn_mfma.cuh"

namespace adt {

template <int HD, int CH>
struct WattnLongLds {
  typedef WmShape<HD> S;
  static constexpr int RST = CH + 4, LPMAX = ATTN_LONG_LMAX;
  static constexpr size_t mask_bytes = LPMAX + 32;      // key validity bytes + one first-valid-key candidate per wave
  static constexpr size_t cat = (size_t)CH * S::RSK + CH, t = (size_t)HD * RST, nat = (size_t)CH * S::RSV;
  static constexpr size_t fwd_bytes = (cat + 2 * t) * sizeof(float) + mask_bytes;
  static constexpr size_t bwd_bytes = (cat + 2 * t + 2 * nat + 2 * t + 2 * LPMAX) * sizeof(float) + mask_bytes;
};

// Wasserstein dQm / dKm of features f0 .. f0 + 3.  On a pad lane the operands are zero and 2 * 0 * dwsum - 2 * 0 is -0.0 whenever dwsum is
// negative: head size 128 (adt_wattn_hd128.hip) selects +0.0 there by the lane index, as the covariance gradients always have.  Head sizes
// 16 / 32 / 64 store the value as it is: their code objects (adt_wattn_long.hip) do not change.
template <int HD>
ADT_DEVICE_INLINE float4 wl_mean_grad4(const WAttnArgs& a, int f0, float4 v) {
  if constexpr (HD > 64) return make_float4(wm_live(a, f0) ? v.x : 0.f, wm_live(a, f0 + 1) ? v.y : 0.f, wm_live(a, f0 + 2) ? v.z : 0.f, wm_live(a, f0 + 3) ? v.w : 0.f);
  else return v;
}

template <int PREC, int HD, int MET, int CH>
__global__ __launch_bounds__(WM_NW * 64) void k_wattn_long_fwd(WAttnArgs a) {
  typedef WmShape<HD> S;
  constexpr int KT = CH / 16, RST = CH + 4;
  static_assert(CH % 32 == 0 && ATTN_LONG_LMAX % CH == 0, "chunks hold whole tile pairs");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int hl = MET == WM_KLP ? a.hd_live : WM_ALL_LIVE;      // KL: the live lanes of a head (WM_ALL_LIVE: every lane test folds to true)
  const float fhl = MET == WM_KLP ? (float)a.hd_live : (float)HD;      // the dimension the divergence subtracts
  float* sK = smem;                          // [CH][RSK]  [mk | sqrt Sk] of keys k0 .. k0 + CH - 1     (KL: Y = [1/ck | cq])
  float* sNk = sK + CH * S::RSK;             // [CH]       norms                                         (KL: column bias sum log ck)
  float* sVmT = sNk + CH;                    // [HD][RST]
  float* sVcT = sVmT + HD * RST;
  unsigned char* sKv = reinterpret_cast<unsigned char*>(sVcT + HD * RST);
  int* sF = reinterpret_cast<int*>(sKv + ATTN_LONG_LMAX);
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int L = a.L, co = h * HD;
  const size_t row_b = (size_t)b * L;
  const int first = attn_long_masks<WM_NW * 64, ATTN_LONG_LMAX>(sKv, sF, a.kid, row_b, L);
  const int nt16 = (L + 15) / 16;
  const int qt = blockIdx.y * WM_NW + w;
  const bool active = qt < nt16;
  const int i = qt * 16 + c;
  const bool vi = active && i < L;
  const size_t qrow = row_b + (vi ? i : 0);
  Frag8 fq[S::KB];
  float nq;                                    // KL: the row bias sum log cq_i
  if constexpr (wm_kl(MET)) {
#pragma unroll
    for (int kb = 0; kb < S::KB; ++kb)
      fq[kb] = wm_kl_frag<HD, true>(a.Qm + qrow * a.ldqm + co, a.Km + qrow * a.ldkm + co, a.Qc + qrow * a.ldqc + co, a.Kc + qrow * a.ldkc + co, kb, g, vi, hl);
    nq = vi ? wm_kl_logsum<HD>(a.Qc + qrow * a.ldqc + co, hl) : 0.f;
  } else {
#pragma unroll
    for (int kb = 0; kb < S::KB; ++kb) fq[kb] = wm_cat_frag<HD>(a.Qm + qrow * a.ldqm + co, a.Qc + qrow * a.ldqc + co, kb, g, vi);
    nq = vi ? wm_row_norm<HD>(a.Qm + qrow * a.ldqm + co, a.Qc + qrow * a.ldqc + co) : 0.f;
  }
  const bool dead_i = vi && i < first;
  const bool tile_dead = qt * 16 < first;      // wave-uniform: the tile holds a dead query and visits every key
  const int g0 = blockIdx.y * WM_NW * 16;      // the group's first query
  const int kend = (g0 < first || g0 + WM_NW * 16 > L) ? L : g0 + WM_NW * 16;
  const uint32_t key_rng = drop_key(a.drop);
  const float rsq_hd = a.xscale > 0.f ? a.xscale : 1.0f / sqrtf((float)HD);      // xscale: the scaled entry points (padded heads)
  const uint32_t idx_q = ((uint32_t)(bh + a.bh_offset) * (uint32_t)L + (uint32_t)i) * (uint32_t)L;
  f32x4 om[S::NT], oc[S::NT];
#pragma unroll
  for (int nt = 0; nt < S::NT; ++nt) { om[nt] = f32x4{0.f, 0.f, 0.f, 0.f}; oc[nt] = om[nt]; }
  float m = -INFINITY, sum = 0.f;              // sum: this lane's share (keys 4g + r of every tile), folded over g at the end
#pragma unroll 1
  for (int k0 = 0; k0 < kend; k0 += CH) {
    const int Lc = L - k0 < CH ? L - k0 : CH;
    __syncthreads();
    wm_stage_t<false>(sVmT, a.Vm + (row_b + k0) * a.ldvm + co, a.ldvm, Lc, CH, HD);
    wm_stage_t<false>(sVcT, a.Vc + (row_b + k0) * a.ldvc + co, a.ldvc, Lc, CH, HD);
    if constexpr (wm_kl(MET))
      wm_kl_stage<HD, false>(sK, sNk, nullptr, 0, nullptr, 0, a.Qc + (row_b + k0) * a.ldqc + co, a.ldqc, a.Kc + (row_b + k0) * a.ldkc + co, a.ldkc, Lc, CH, hl);
    else
      wm_stage_cat<HD>(sK, sNk, a.Km + (row_b + k0) * a.ldkm + co, a.ldkm, a.Kc + (row_b + k0) * a.ldkc + co, a.ldkc, Lc, CH);
    __syncthreads();
    if (!active) continue;
    if (!tile_dead && k0 > qt * 16 + 15) continue;      // every key of the chunk lies above the diagonal of a tile without dead rows
    f32x4 s[KT];
    float cm = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      s[kt] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      const int j0 = k0 + kt * 16;
      if (j0 < L && (tile_dead || j0 <= qt * 16 + 15)) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < S::KB; ++kb) acc = mma16<PREC>(acc, frag_contig(sK + (kt * 16 + c) * S::RSK + 32 * kb + 8 * g), fq[kb]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int jl = kt * 16 + 4 * g + r, j = k0 + jl;
          if (j < L) {
            const float x = wm_kl(MET) ? wm_kl_x(sNk[jl], nq, acc[r], fhl, rsq_hd) : -((sNk[jl] + nq) - 2.0f * acc[r]) * rsq_hd;
            const bool masked = j > i || sKv[j] == 0;
            if (!masked || dead_i) {           // masked keys of a live row: exp(x - 2^32 - m) == 0, left at -inf
              s[kt][r] = w_score(x, masked, dead_i);
              cm = fmaxf(cm, s[kt][r]);
            }
          }
        }
      }
    }
    cm = wm_colmax(cm);
    const float mn = fmaxf(m, cm);
    const float mu = mn == -INFINITY ? 0.f : mn;      // no finite score yet: every exponential below is exp(-inf) = 0
    const float alpha = __expf(m - mu), alpha2 = alpha * alpha;
    m = mn;
    sum *= alpha;
#pragma unroll
    for (int nt = 0; nt < S::NT; ++nt) { om[nt] = om[nt] * alpha; oc[nt] = oc[nt] * alpha2; }
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      const f32x4 ks4 = wm_keep_scale4(a.drop, key_rng, idx_q + (uint32_t)(k0 + kt * 16 + 4 * g));
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = s[kt][r] != -INFINITY ? __expf(s[kt][r] - mu) : 0.f;
        sum += e;
        s[kt][r] = e * ks4[r];
      }
    }
    // contexts: O^T[feature][query] += sum_key V^T[feature][key] P~^T[key][query]
#pragma unroll
    for (int kp = 0; kp < KT / 2; ++kp) {
      if (k0 + 32 * kp >= L || (!tile_dead && k0 + 32 * kp > qt * 16 + 15)) continue;
      const Frag8 bp = wm_acc_frag(s[2 * kp], s[2 * kp + 1]);
      Frag8 bp2;
#pragma unroll
      for (int j = 0; j < 8; ++j) bp2.v[j] = bp.v[j] * bp.v[j];
#pragma unroll
      for (int nt = 0; nt < S::NT; ++nt) {
        om[nt] = mma16<PREC>(om[nt], frag_slotc(sVmT + (16 * nt + c) * RST + 32 * kp, g), bp);
        oc[nt] = mma16<PREC>(oc[nt], frag_slotc(sVcT + (16 * nt + c) * RST + 32 * kp, g), bp2);
      }
    }
  }
  if (!vi) return;
  sum = wm_colsum(sum);
  const float inv = 1.0f / sum, inv2 = inv * inv;
  if (g == 0) a.LSE[(size_t)bh * L + i] = m + logf(sum);
#pragma unroll
  for (int nt = 0; nt < S::NT; ++nt) {
    *reinterpret_cast<float4*>(a.Om + (row_b + i) * a.ldom + co + 16 * nt + 4 * g) = make_float4(om[nt][0] * inv, om[nt][1] * inv, om[nt][2] * inv, om[nt][3] * inv);
    *reinterpret_cast<float4*>(a.Oc + (row_b + i) * a.ldoc + co + 16 * nt + 4 * g) = make_float4(oc[nt][0] * inv2, oc[nt][1] * inv2, oc[nt][2] * inv2, oc[nt][3] * inv2);
  }
}

// Backward.  Pass A (key chunks resident, wave owns a query tile) -> dQm, dQc (KL: dKm and the row parts of dKc, dQc too); pass B (query
// chunks resident, wave owns a key tile) -> dKm, dKc, dVm, dVc (KL: the column parts, added to pass A's by the lane that wrote them).
// delta_i = dOm_i . Om_i + 2 dOc_i . Oc_i from the saved contexts, as in k_wattn_mfma_bwd.
template <int PREC, int HD, int MET, int CH>
__global__ __launch_bounds__(WM_NW * 64) void k_wattn_long_bwd(WAttnArgs a) {
  typedef WmShape<HD> S;
  constexpr int KBV = (HD + 31) / 32, RST = CH + 4, NP = CH / 32;
  static_assert(CH % 32 == 0 && ATTN_LONG_LMAX % CH == 0, "chunks hold whole tile pairs");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int hl = MET == WM_KLP ? a.hd_live : WM_ALL_LIVE;      // KL: the live lanes of a head (WM_ALL_LIVE: every lane test folds to true)
  const float fhl = MET == WM_KLP ? (float)a.hd_live : (float)HD;      // the dimension the divergence subtracts
  float* sC = smem;                          // A: [mk | sqrt Sk] rows of the key chunk (KL: Y) | B: [mq | sqrt Sq] rows of the query chunk (KL: X)
  float* sN = sC + CH * S::RSK;              // A: key norms / column biases                     | B: query norms / row biases
  float* sCT = sN + CH;                      // [KC][RST] transposed image
  float* sX0 = sCT + S::KC * RST;            // A: Vm rows  | B: dOm rows      [CH][RSV]
  float* sX1 = sX0 + CH * S::RSV;            // A: Vc rows  | B: dOc rows
  float* sT0 = sX1 + CH * S::RSV;            // B only: dOm^T [HD][RST]
  float* sT1 = sT0 + HD * RST;               // B only: dOc^T
  float* sLse = sT1 + HD * RST;              // [1024]; +inf past L -> P = 0
  float* sDelta = sLse + ATTN_LONG_LMAX;     // [1024]
  unsigned char* sKv = reinterpret_cast<unsigned char*>(sDelta + ATTN_LONG_LMAX);
  int* sF = reinterpret_cast<int*>(sKv + ATTN_LONG_LMAX);
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int L = a.L, co = h * HD;
  const size_t row_b = (size_t)b * L;
  const float rsq_hd = a.xscale > 0.f ? a.xscale : 1.0f / sqrtf((float)HD);      // xscale: the scaled entry points (padded heads)
  const uint32_t key_rng = drop_key(a.drop);
  const uint32_t idx_bh = (uint32_t)(bh + a.bh_offset) * (uint32_t)L;
  for (int i = threadIdx.x; i < ATTN_LONG_LMAX; i += WM_NW * 64) {
    float dl = 0.f;
    if (i < L) {
      const float* dm = a.dOm + (row_b + i) * a.lddom + co; const float* om = a.Om + (row_b + i) * a.ldom + co;
      const float* dc = a.dOc + (row_b + i) * a.lddoc + co; const float* oc = a.Oc + (row_b + i) * a.ldoc + co;
      for (int k = 0; k < HD; k += 4) {
        const float4 x0 = *reinterpret_cast<const float4*>(dm + k), y0 = *reinterpret_cast<const float4*>(om + k);
        const float4 x1 = *reinterpret_cast<const float4*>(dc + k), y1 = *reinterpret_cast<const float4*>(oc + k);
        dl += (x0.x * y0.x + x0.y * y0.y + x0.z * y0.z + x0.w * y0.w) + 2.0f * (x1.x * y1.x + x1.y * y1.y + x1.z * y1.z + x1.w * y1.w);
      }
    }
    sDelta[i] = dl;
    sLse[i] = i < L ? a.LSE[(size_t)bh * L + i] : INFINITY;
  }
  const int first = attn_long_masks<WM_NW * 64, ATTN_LONG_LMAX>(sKv, sF, a.kid, row_b, L);      // ends with the workgroup in step
  const int nt16 = (L + 15) / 16;
  const int tile = blockIdx.y * WM_NW + w;     // the wave's query tile (pass A) / key tile (pass B)
  const bool active = tile < nt16;
  const int g0 = blockIdx.y * WM_NW * 16;      // first query (pass A) / key (pass B) row of the group

  // ---- pass A: wave owns query tile ; tiles T[key 4g+r][query c] -------------------------------------------------------------------
  {
    const int i = tile * 16 + c;
    const bool vi = active && i < L;
    const size_t qrow = row_b + (vi ? i : 0);
    Frag8 fq[S::KB], fdm[KBV], fdc[KBV];
    float nq;
    if constexpr (wm_kl(MET)) {
#pragma unroll
      for (int kb = 0; kb < S::KB; ++kb)
        fq[kb] = wm_kl_frag<HD, true>(a.Qm + qrow * a.ldqm + co, a.Km + qrow * a.ldkm + co, a.Qc + qrow * a.ldqc + co, a.Kc + qrow * a.ldkc + co, kb, g, vi, hl);
      nq = vi ? wm_kl_logsum<HD>(a.Qc + qrow * a.ldqc + co, hl) : 0.f;
    } else {
#pragma unroll
      for (int kb = 0; kb < S::KB; ++kb) fq[kb] = wm_cat_frag<HD>(a.Qm + qrow * a.ldqm + co, a.Qc + qrow * a.ldqc + co, kb, g, vi);
      nq = vi ? wm_row_norm<HD>(a.Qm + qrow * a.ldqm + co, a.Qc + qrow * a.ldqc + co) : 0.f;
    }
#pragma unroll
    for (int kb = 0; kb < KBV; ++kb) {
      fdm[kb] = frag_contig_hd<HD>(a.dOm + qrow * a.lddom + co, kb, g);
      fdc[kb] = frag_contig_hd<HD>(a.dOc + qrow * a.lddoc + co, kb, g);
      if (!vi) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { fdm[kb].v[j] = 0.f; fdc[kb].v[j] = 0.f; }
      }
    }
    const float lse = vi ? sLse[i] : INFINITY, delta = vi ? sDelta[i] : 0.f;
    const bool dead_i = vi && i < first;
    const bool tile_dead = tile * 16 < first;
    const int kend = (g0 < first || g0 + WM_NW * 16 > L) ? L : g0 + WM_NW * 16;
    const uint32_t idx_q = (idx_bh + (uint32_t)i) * (uint32_t)L;
    f32x4 accq[S::KC / 16];
#pragma unroll
    for (int ft = 0; ft < S::KC / 16; ++ft) accq[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dwsum = 0.f;
#pragma unroll 1
    for (int k0 = 0; k0 < kend; k0 += CH) {
      const int Lc = L - k0 < CH ? L - k0 : CH;
      __syncthreads();
      wm_stage_nat<HD>(sX0, a.Vm + (row_b + k0) * a.ldvm + co, a.ldvm, Lc, CH);
      wm_stage_nat<HD>(sX1, a.Vc + (row_b + k0) * a.ldvc + co, a.ldvc, Lc, CH);
      if constexpr (wm_kl(MET)) {      // Y = [1/ck | cq] rows and column biases; the transpose after the barrier
        wm_kl_stage<HD, false>(sC, sN, nullptr, 0, nullptr, 0, a.Qc + (row_b + k0) * a.ldqc + co, a.ldqc, a.Kc + (row_b + k0) * a.ldkc + co, a.ldkc, Lc, CH, hl);
        __syncthreads();
        wm_kl_transpose<HD>(sCT, sC, CH);
      } else {
        wm_stage_t<false>(sCT, a.Km + (row_b + k0) * a.ldkm + co, a.ldkm, Lc, CH, HD);
        wm_stage_t<true>(sCT + HD * RST, a.Kc + (row_b + k0) * a.ldkc + co, a.ldkc, Lc, CH, HD);
        wm_stage_cat<HD>(sC, sN, a.Km + (row_b + k0) * a.ldkm + co, a.ldkm, a.Kc + (row_b + k0) * a.ldkc + co, a.ldkc, Lc, CH);
      }
      __syncthreads();
      if (!active) continue;
#pragma unroll 1
      for (int kp = 0; kp < NP; ++kp) {
        const int p0 = k0 + 32 * kp;
        if (p0 >= L) break;
        if (!tile_dead && p0 > tile * 16 + 15) break;      // every key of the pair lies above the diagonal of a tile without dead rows
        f32x4 dwt[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int ktl = 2 * kp + t;
          dwt[t] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (k0 + ktl * 16 < L) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f}, gm = acc, gc = acc;
#pragma unroll
            for (int kb = 0; kb < S::KB; ++kb) acc = mma16<PREC>(acc, frag_contig(sC + (ktl * 16 + c) * S::RSK + 32 * kb + 8 * g), fq[kb]);
#pragma unroll
            for (int kb = 0; kb < KBV; ++kb) {
              gm = mma16<PREC>(gm, frag_contig_hd<HD>(sX0 + (ktl * 16 + c) * S::RSV, kb, g), fdm[kb]);
              gc = mma16<PREC>(gc, frag_contig_hd<HD>(sX1 + (ktl * 16 + c) * S::RSV, kb, g), fdc[kb]);
            }
            const f32x4 ks4 = wm_keep_scale4(a.drop, key_rng, idx_q + (uint32_t)(k0 + ktl * 16 + 4 * g));
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int jl = ktl * 16 + 4 * g + r, j = k0 + jl;
              if (j < L && vi) {
                const float x = wm_kl(MET) ? wm_kl_x(sN[jl], nq, acc[r], fhl, rsq_hd) : -((sN[jl] + nq) - 2.0f * acc[r]) * rsq_hd;
                float dw, pd;
                wm_pair_bwd<HD>(x, j > i || sKv[j] == 0, dead_i, lse, ks4[r], gm[r], gc[r], delta, rsq_hd, dw, pd);
                dwt[t][r] = dw;
                dwsum += dw;
              }
            }
          }
        }
        const Frag8 bdw = wm_acc_frag(dwt[0], dwt[1]);        // dQcat^T[k][i] += sum_j Kcat^T[k][j] dW^T[j][i] over this pair's 32 keys
#pragma unroll
        for (int ft = 0; ft < S::KC / 16; ++ft) accq[ft] = mma16<PREC>(accq[ft], frag_slotc(sCT + (16 * ft + c) * RST + 32 * kp, g), bdw);
      }
    }
    dwsum = wm_colsum(dwsum);
    if (wm_kl(MET) && vi) {
      // dmq = (mq - mk) sum_j dW Y1, dmk = -dmq; row parts: dck = -0.5 / ck^2 sum_j dW Y2, dcq = -0.5 / cq sum_j dW
#pragma unroll
      for (int ft = 0; ft < S::KC / 16; ++ft) {
        const int k0 = 16 * ft + 4 * g;
        const f32x4& acc = accq[ft];
        if (k0 < HD) {
          const float4 q = *reinterpret_cast<const float4*>(a.Qm + qrow * a.ldqm + co + k0);
          const float4 k = *reinterpret_cast<const float4*>(a.Km + qrow * a.ldkm + co + k0);
          const float4 dq = make_float4((q.x - k.x) * acc[0], (q.y - k.y) * acc[1], (q.z - k.z) * acc[2], (q.w - k.w) * acc[3]);
          *reinterpret_cast<float4*>(a.dQm + qrow * a.ldd + co + k0) = wm_gate4(hl, k0, dq);
          *reinterpret_cast<float4*>(a.dKm + qrow * a.ldd + co + k0) = wm_gate4(hl, k0, make_float4(-dq.x, -dq.y, -dq.z, -dq.w));
        } else {
          const int f0 = k0 - HD;
          const float4 kc = *reinterpret_cast<const float4*>(a.Kc + qrow * a.ldkc + co + f0);
          const float4 qc = *reinterpret_cast<const float4*>(a.Qc + qrow * a.ldqc + co + f0);
          // a pad lane (kc = qc = 0) takes +0.0 by the select: 0 / 0 and dwsum / 0 are never stored
          *reinterpret_cast<float4*>(a.dKc + qrow * a.ldd + co + f0) = wm_gate4(hl, f0,
              make_float4(-0.5f * acc[0] / (kc.x * kc.x), -0.5f * acc[1] / (kc.y * kc.y), -0.5f * acc[2] / (kc.z * kc.z), -0.5f * acc[3] / (kc.w * kc.w)));
          *reinterpret_cast<float4*>(a.dQc + qrow * a.ldd + co + f0) = wm_gate4(hl, f0,
              make_float4(-0.5f * dwsum / qc.x, -0.5f * dwsum / qc.y, -0.5f * dwsum / qc.z, -0.5f * dwsum / qc.w));
        }
      }
    } else if (vi) {
#pragma unroll
      for (int ft = 0; ft < S::KC / 16; ++ft) {
        const int k0 = 16 * ft + 4 * g;          // features k0 .. k0+3 of the concatenation
        const f32x4& acc = accq[ft];
        if (k0 < HD) {
          const float4 q = *reinterpret_cast<const float4*>(a.Qm + qrow * a.ldqm + co + k0);
          *reinterpret_cast<float4*>(a.dQm + qrow * a.ldd + co + k0) = wl_mean_grad4<HD>(a, k0,
              make_float4(2.0f * q.x * dwsum - 2.0f * acc[0], 2.0f * q.y * dwsum - 2.0f * acc[1], 2.0f * q.z * dwsum - 2.0f * acc[2], 2.0f * q.w * dwsum - 2.0f * acc[3]));
        } else {
          const float4 qc = *reinterpret_cast<const float4*>(a.Qc + qrow * a.ldqc + co + k0 - HD);
          const float s0 = w_sqrt_cov(qc.x), s1 = w_sqrt_cov(qc.y), s2 = w_sqrt_cov(qc.z), s3 = w_sqrt_cov(qc.w);
          // clamp(min = 1e-24) gates the sqrt path (cov = 0 exactly -> no gradient)
          *reinterpret_cast<float4*>(a.dQc + qrow * a.ldd + co + k0 - HD) =
              make_float4(wm_live(a, k0 - HD) ? dwsum - (s0 > 1.00001e-12f ? acc[0] / s0 : 0.f) : 0.f, wm_live(a, k0 - HD + 1) ? dwsum - (s1 > 1.00001e-12f ? acc[1] / s1 : 0.f) : 0.f,
                          wm_live(a, k0 - HD + 2) ? dwsum - (s2 > 1.00001e-12f ? acc[2] / s2 : 0.f) : 0.f, wm_live(a, k0 - HD + 3) ? dwsum - (s3 > 1.00001e-12f ? acc[3] / s3 : 0.f) : 0.f);
        }
      }
    }
  }

  // ---- pass B: wave owns key tile ; tiles T[query 4g+r][key c] (operands swapped: the QUERY image rows are the A operand) ---------------
  {
    const int j = tile * 16 + c;
    const bool vj = active && j < L;
    const size_t krow = row_b + (vj ? j : 0);
    Frag8 fk[S::KB], fvm[KBV], fvc[KBV];
    float nk;                                  // KL: the column bias sum log ck_j
    if constexpr (wm_kl(MET)) {
#pragma unroll
      for (int kb = 0; kb < S::KB; ++kb) fk[kb] = wm_kl_frag<HD, false>(nullptr, nullptr, a.Qc + krow * a.ldqc + co, a.Kc + krow * a.ldkc + co, kb, g, vj, hl);
      nk = vj ? wm_kl_logsum<HD>(a.Kc + krow * a.ldkc + co, hl) : 0.f;
    } else {
#pragma unroll
      for (int kb = 0; kb < S::KB; ++kb) fk[kb] = wm_cat_frag<HD>(a.Km + krow * a.ldkm + co, a.Kc + krow * a.ldkc + co, kb, g, vj);
      nk = vj ? wm_row_norm<HD>(a.Km + krow * a.ldkm + co, a.Kc + krow * a.ldkc + co) : 0.f;
    }
#pragma unroll
    for (int kb = 0; kb < KBV; ++kb) {
      fvm[kb] = frag_contig_hd<HD>(a.Vm + krow * a.ldvm + co, kb, g);
      fvc[kb] = frag_contig_hd<HD>(a.Vc + krow * a.ldvc + co, kb, g);
      if (!vj) {
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) { fvm[kb].v[jj] = 0.f; fvc[kb].v[jj] = 0.f; }
      }
    }
    const bool key_pad = !vj || sKv[j] == 0;
    f32x4 acck[S::KC / 16], accvm[S::NT], accvc[S::NT];
#pragma unroll
    for (int ft = 0; ft < S::KC / 16; ++ft) acck[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nt = 0; nt < S::NT; ++nt) { accvm[nt] = f32x4{0.f, 0.f, 0.f, 0.f}; accvc[nt] = accvm[nt]; }
    float dwsum = 0.f;
#pragma unroll 1
    for (int q0 = 0; q0 < L; q0 += CH) {
      if (q0 >= first && q0 + CH <= g0) continue;      // live queries before the group's first key: every pair is masked and contributes 0
      const int Lc = L - q0 < CH ? L - q0 : CH;
      __syncthreads();
      wm_stage_nat<HD>(sX0, a.dOm + (row_b + q0) * a.lddom + co, a.lddom, Lc, CH);
      wm_stage_nat<HD>(sX1, a.dOc + (row_b + q0) * a.lddoc + co, a.lddoc, Lc, CH);
      wm_stage_t<false>(sT0, a.dOm + (row_b + q0) * a.lddom + co, a.lddom, Lc, CH, HD);
      wm_stage_t<false>(sT1, a.dOc + (row_b + q0) * a.lddoc + co, a.lddoc, Lc, CH, HD);
      if constexpr (wm_kl(MET)) {      // X = [(mq - mk)^2 | 1/ck] rows and row biases; the transpose after the barrier
        wm_kl_stage<HD, true>(sC, sN, a.Qm + (row_b + q0) * a.ldqm + co, a.ldqm, a.Km + (row_b + q0) * a.ldkm + co, a.ldkm,
                              a.Qc + (row_b + q0) * a.ldqc + co, a.ldqc, a.Kc + (row_b + q0) * a.ldkc + co, a.ldkc, Lc, CH, hl);
        __syncthreads();
        wm_kl_transpose<HD>(sCT, sC, CH);
      } else {
        wm_stage_t<false>(sCT, a.Qm + (row_b + q0) * a.ldqm + co, a.ldqm, Lc, CH, HD);
        wm_stage_t<true>(sCT + HD * RST, a.Qc + (row_b + q0) * a.ldqc + co, a.ldqc, Lc, CH, HD);
        wm_stage_cat<HD>(sC, sN, a.Qm + (row_b + q0) * a.ldqm + co, a.ldqm, a.Qc + (row_b + q0) * a.ldqc + co, a.ldqc, Lc, CH);
      }
      __syncthreads();
      if (!active) continue;
#pragma unroll 1
      for (int qp = 0; qp < NP; ++qp) {
        const int p0 = q0 + 32 * qp;
        if (p0 >= L) break;
        if (p0 >= first && p0 + 31 < tile * 16) continue;      // live queries, all before this key tile
        f32x4 dwt[2], pdt[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int itl = 2 * qp + t;
          dwt[t] = f32x4{0.f, 0.f, 0.f, 0.f};
          pdt[t] = dwt[t];
          if (q0 + itl * 16 < L) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f}, gm = acc, gc = acc;
#pragma unroll
            for (int kb = 0; kb < S::KB; ++kb) acc = mma16<PREC>(acc, frag_contig(sC + (itl * 16 + c) * S::RSK + 32 * kb + 8 * g), fk[kb]);
#pragma unroll
            for (int kb = 0; kb < KBV; ++kb) {
              gm = mma16<PREC>(gm, frag_contig_hd<HD>(sX0 + (itl * 16 + c) * S::RSV, kb, g), fvm[kb]);
              gc = mma16<PREC>(gc, frag_contig_hd<HD>(sX1 + (itl * 16 + c) * S::RSV, kb, g), fvc[kb]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int il = itl * 16 + 4 * g + r, i = q0 + il;
              if (i < L && vj) {
                const float x = wm_kl(MET) ? wm_kl_x(nk, sN[il], acc[r], fhl, rsq_hd)
                                             : -((nk + sN[il]) - 2.0f * acc[r]) * rsq_hd;      // nk + nq: the same two numbers as in the forward, addition commutes
                const float ks_ = wm_keep_scale(a.drop, key_rng, (idx_bh + (uint32_t)i) * (uint32_t)L + (uint32_t)j);
                float dw, pd;
                wm_pair_bwd<HD>(x, j > i || key_pad, i < first, sLse[i], ks_, gm[r], gc[r], sDelta[i], rsq_hd, dw, pd);
                dwt[t][r] = dw;
                pdt[t][r] = pd;
                dwsum += dw;
              }
            }
          }
        }
        // dKcat^T[k][j] += sum_i Qcat^T[k][i] dW[i][j] ; dVm^T[d][j] += sum_i dOm^T[d][i] P~[i][j] ; dVc^T[d][j] += sum_i dOc^T[d][i] P~^2[i][j]
        const Frag8 bdw = wm_acc_frag(dwt[0], dwt[1]), bp = wm_acc_frag(pdt[0], pdt[1]);
        Frag8 bp2;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) bp2.v[jj] = bp.v[jj] * bp.v[jj];
#pragma unroll
        for (int ft = 0; ft < S::KC / 16; ++ft) acck[ft] = mma16<PREC>(acck[ft], frag_slotc(sCT + (16 * ft + c) * RST + 32 * qp, g), bdw);
#pragma unroll
        for (int nt = 0; nt < S::NT; ++nt) {
          accvm[nt] = mma16<PREC>(accvm[nt], frag_slotc(sT0 + (16 * nt + c) * RST + 32 * qp, g), bp);
          accvc[nt] = mma16<PREC>(accvc[nt], frag_slotc(sT1 + (16 * nt + c) * RST + 32 * qp, g), bp2);
        }
      }
    }
    dwsum = wm_colsum(dwsum);
    if (wm_kl(MET) && vj) {
      // column parts, added to pass A's row parts (same wave, same lane): dck += 0.5 / ck sum_i dW - 0.5 / ck^2 sum_i dW X1,
      // dcq += 0.5 sum_i dW X2
#pragma unroll
      for (int ft = 0; ft < S::KC / 16; ++ft) {
        const int k0 = 16 * ft + 4 * g;
        const f32x4& acc = acck[ft];
        if (k0 < HD) {
          const float4 kc = *reinterpret_cast<const float4*>(a.Kc + krow * a.ldkc + co + k0);
          float4* dkc = reinterpret_cast<float4*>(a.dKc + krow * a.ldd + co + k0);
          const float4 y = make_float4(1.0f / kc.x, 1.0f / kc.y, 1.0f / kc.z, 1.0f / kc.w), o = *dkc;
          *dkc = wm_gate4(hl, k0, make_float4(o.x + (0.5f * dwsum * y.x - 0.5f * acc[0] * y.x * y.x), o.y + (0.5f * dwsum * y.y - 0.5f * acc[1] * y.y * y.y),
                                              o.z + (0.5f * dwsum * y.z - 0.5f * acc[2] * y.z * y.z), o.w + (0.5f * dwsum * y.w - 0.5f * acc[3] * y.w * y.w)));
        } else {
          float4* dqc = reinterpret_cast<float4*>(a.dQc + krow * a.ldd + co + k0 - HD);
          const float4 o = *dqc;
          *dqc = wm_gate4(hl, k0 - HD, make_float4(o.x + 0.5f * acc[0], o.y + 0.5f * acc[1], o.z + 0.5f * acc[2], o.w + 0.5f * acc[3]));
        }
      }
    } else if (vj) {
#pragma unroll
      for (int ft = 0; ft < S::KC / 16; ++ft) {
        const int k0 = 16 * ft + 4 * g;
        const f32x4& acc = acck[ft];
        if (k0 < HD) {
          const float4 k = *reinterpret_cast<const float4*>(a.Km + krow * a.ldkm + co + k0);
          *reinterpret_cast<float4*>(a.dKm + krow * a.ldd + co + k0) = wl_mean_grad4<HD>(a, k0,
              make_float4(2.0f * k.x * dwsum - 2.0f * acc[0], 2.0f * k.y * dwsum - 2.0f * acc[1], 2.0f * k.z * dwsum - 2.0f * acc[2], 2.0f * k.w * dwsum - 2.0f * acc[3]));
        } else {
          const float4 kc = *reinterpret_cast<const float4*>(a.Kc + krow * a.ldkc + co + k0 - HD);
          const float s0 = w_sqrt_cov(kc.x), s1 = w_sqrt_cov(kc.y), s2 = w_sqrt_cov(kc.z), s3 = w_sqrt_cov(kc.w);
          *reinterpret_cast<float4*>(a.dKc + krow * a.ldd + co + k0 - HD) =
              make_float4(wm_live(a, k0 - HD) ? dwsum - (s0 > 1.00001e-12f ? acc[0] / s0 : 0.f) : 0.f, wm_live(a, k0 - HD + 1) ? dwsum - (s1 > 1.00001e-12f ? acc[1] / s1 : 0.f) : 0.f,
                          wm_live(a, k0 - HD + 2) ? dwsum - (s2 > 1.00001e-12f ? acc[2] / s2 : 0.f) : 0.f, wm_live(a, k0 - HD + 3) ? dwsum - (s3 > 1.00001e-12f ? acc[3] / s3 : 0.f) : 0.f);
        }
      }
    }
    if (vj) {
#pragma unroll
      for (int nt = 0; nt < S::NT; ++nt) {
        *reinterpret_cast<float4*>(a.dVm + krow * a.ldd + co + 16 * nt + 4 * g) = make_float4(accvm[nt][0], accvm[nt][1], accvm[nt][2], accvm[nt][3]);
        *reinterpret_cast<float4*>(a.dVc + krow * a.ldd + co + 16 * nt + 4 * g) = make_float4(accvc[nt][0], accvc[nt][1], accvc[nt][2], accvc[nt][3]);
      }
    }
  }
}

}  // namespace adt
