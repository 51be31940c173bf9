// General masked attention with key / query chunks streamed through LDS, for the shapes whose whole-(b, h) images do not fit it: sequences of
// 1 <= L <= LMAX rows at head sizes 16 .. 256, either precision.  LMAX, the rows of per-sequence state, is 256 (adt_attn_masked_*: head size
// 256, and head size 128 in the exact-fp32 mode at L > 64) or 1024 (adt_attn_long_*, every head size).  Same semantics, fill rule, dropout
// indices and fragment interface as adt_attn_gen.cuh.
//
// One 264-element padded row per key is 135 KB (bf16) / 270 KB (fp32) at hd = 256, L = 256, before V^T: no (b, h) fits in LDS.  So:
//  * the grid is (B*H, query / key groups of NW 16-row tiles), one tile per wave;
//  * the forward streams key chunks (K row image + V^T image) through LDS with an online softmax: each wave keeps its
//    16 x HD fp32 output tile (64 registers at hd 256) and running row max / sum across chunks, rescaling the tile when the max moves;
//  * the backward streams key chunks (K, V, K^T) past the dQ tiles of the group (pass A), then query chunks (Q, dO, Q^T,
//    dO^T) past the dK / dV tiles (pass B), P recomputed from the forward's LSE as in k_attn_gen_bwd_chunked.
// Under a causal mask without key padding and fill <= -1e9 (csk) chunks and tile pairs entirely above the diagonal are skipped.
//
// Two int[1024] mask arrays do not fit beside the fp32 hd = 256 backward images (149,504 B of 163,840), so at either LMAX
//  * key validity is one byte per key;
//  * the per-query "no attendable key" flags are one number per sequence, the index f of its first attendable key (L: none):
//    query q is dead exactly when f >= (causal ? min(q + 1, L) : L), and the mask set-up is O(L);
//  * heads narrower than one 32-wide MFMA block read zero fragments past HD (rfrag_g, gfrag), as the resident kernels do.
#pragma once
#include "adt_attn_gen.cuh"

namespace adt {

template <int PREC, int HD, int KC, int LMAX>
struct AttnLongLds {
  typedef typename Img<PREC>::E E;
  static_assert(LMAX == 256 || LMAX == 1024, "rows of per-sequence state");
  static constexpr int RS = HD + 8, KCT = KC + 8;
  static constexpr size_t mask_bytes = LMAX + 32;      // key validity bytes + one first-attendable-key candidate per wave (<= 8 waves)
  static constexpr size_t fwd_bytes = (size_t)(KC * RS + HD * KCT) * sizeof(E) + mask_bytes;
  static constexpr size_t bwd_bytes = (size_t)(2 * KC * RS + 2 * HD * KCT) * sizeof(E) + 2 * LMAX * sizeof(float) + mask_bytes;
};

// Key validity of the sequence as bytes; returns the index of its first attendable key (L when there is none).  Each thread walks its keys in
// increasing order, the waves fold their minima with shuffles and exchange them through sF: no atomics.  Ends with the workgroup in step.
template <int NTH, int LMAX>
ADT_DEVICE_INLINE int attn_long_masks(unsigned char* sKv, int* sF, const int* kid, size_t row_b, int L) {
  static_assert(NTH % 64 == 0 && NTH / 64 <= 8, "one sF slot per wave");
  int first = L;
  for (int i = threadIdx.x; i < LMAX; i += NTH) {
    const bool ok = i < L && (!kid || kid[row_b + i] > 0);
    sKv[i] = ok ? 1 : 0;
    if (ok && i < first) first = i;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(first, off, 64);
    first = o < first ? o : first;
  }
  if ((threadIdx.x & 63) == 0) sF[threadIdx.x >> 6] = first;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < NTH / 64; ++w) first = sF[w] < first ? sF[w] : first;
  return first;
}

// the dead-row rule of mark_dead_rows from the first attendable key
ADT_DEVICE_INLINE bool attn_long_dead(int first, int q, int L, int causal) { return first >= (causal && q + 1 < L ? q + 1 : L); }

template <int PREC, int HD, int NW, int KC, int LMAX>
__global__ __launch_bounds__(NW * 64) void k_attn_long_fwd(AttnGenArgs ga) {
  typedef Img<PREC> I;
  typedef typename I::E E;
  typedef typename I::F F;
  const AttnArgs& a = ga.a;
  constexpr int KCT = KC + 8, NT = HD / 16, KB = (HD + 31) / 32, KT = KC / 16;
  static_assert(HD == 16 || HD == 32 || HD == 64 || HD == 128 || HD == 256, "head sizes");
  static_assert(KC % 32 == 0 && LMAX % KC == 0, "chunks hold whole tile pairs");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  E* sK = reinterpret_cast<E*>(smem_raw);    // [KC][RS]   keys k0 .. k0 + KC - 1
  E* sVT = sK + KC * (HD + 8);                // [HD][KCT]
  unsigned char* sKv = reinterpret_cast<unsigned char*>(sVT + HD * KCT);
  int* sF = reinterpret_cast<int*>(sKv + LMAX);
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int L = a.L;
  const size_t row_b = (size_t)b * L;
  const bool csk = a.causal && ga.kid == nullptr && ga.fill <= -1e9f;
  const int first = attn_long_masks<NW * 64, LMAX>(sKv, sF, ga.kid, row_b, L);
  const int nqt = (L + 15) / 16;
  const int qt = blockIdx.y * NW + w;
  const bool active = qt < nqt;
  const int q = qt * 16 + c;
  const float fill_q = attn_long_dead(first, q, L, a.causal) ? 0.f : ga.fill;
  const uint32_t key_rng = drop_key(a.drop);
  const uint32_t idx_q = ((uint32_t)(bh + a.bh_offset) * (uint32_t)L + (uint32_t)q) * (uint32_t)L;
  F fq[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) fq[kb] = gfrag<PREC, HD>(a.Q + row_b * a.ldq + h * HD, a.ldq, q, active && q < L, kb, g, a.scale);
  f32x4 o[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) o[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, sum = 0.f;
  int kend = L;                                // csk: keys after the group's last query are never attended
  if (csk && (blockIdx.y + 1) * NW * 16 < kend) kend = (blockIdx.y + 1) * NW * 16;
#pragma unroll 1
  for (int k0 = 0; k0 < kend; k0 += KC) {
    const int Lc = L - k0 < KC ? L - k0 : KC;
    __syncthreads();
    stage_img<PREC, HD, NW * 64>(sK, nullptr, KCT, a.K + (row_b + k0) * a.ldk + h * HD, a.ldk, Lc, KC, 1.0f);
    stage_img<PREC, HD, NW * 64>(nullptr, sVT, KCT, a.V + (row_b + k0) * a.ldv + h * HD, a.ldv, Lc, KC, 1.0f);
    __syncthreads();
    if (!active) continue;
    int ntile = (Lc + 15) / 16;               // tiles of this chunk that hold keys (and, under csk, are not above the diagonal)
    if (csk) {
      const int lastq = qt * 16 + 15;
      const int nd = lastq < k0 ? 0 : (lastq - k0) / 16 + 1;
      if (nd < ntile) ntile = nd;
    }
    if (ntile == 0) continue;
    f32x4 sc[KT];
    float cm = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      sc[kt] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      if (kt < ntile) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) s = I::mma(s, rfrag_g<PREC, HD>(sK, kt * 16 + c, kb, g), fq[kb]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + kt * 16 + 4 * g + r;   // < LMAX: k0 < L and chunks divide it
          const bool masked = (a.causal && key > q) || !sKv[key];
          const float v = masked ? fill_q : s[r];
          sc[kt][r] = key < L ? v : -INFINITY;
        }
        cm = fmaxf(cm, fmaxf(fmaxf(sc[kt][0], sc[kt][1]), fmaxf(sc[kt][2], sc[kt][3])));
      }
    }
    cm = fmaxf(cm, __shfl_xor(cm, 16, 64));
    cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
    const float mn = fmaxf(m, cm);
    const float mu = mn == -INFINITY ? 0.f : mn;     // no finite score yet: every exp below is exp(-inf) = 0
    const float alpha = __expf(m - mu);
    sum *= alpha;
    m = mn;
    float al_r[4];                                   // the output rows of this lane are queries 4g + r
#pragma unroll
    for (int r = 0; r < 4; ++r) al_r[r] = __shfl(alpha, (lane & 48) | (4 * g + r), 64);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[nt][r] *= al_r[r];
#pragma unroll
    for (int kp = 0; kp < KT / 2; ++kp) {
      if (2 * kp >= ntile) break;
      float pv[8];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int kt = 2 * kp + t;
        const uint32_t kbits = (a.drop.thr && kt < ntile) ? adt_keep4_any(key_rng, idx_q + (uint32_t)(k0 + kt * 16 + 4 * g), a.drop.thr, (L & 3) == 0) : 0u;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = __expf(sc[kt][r] - mu);
          sum += e;
          float p = e;
          if (a.drop.thr) p = ((kbits >> r) & 1u) ? e * a.drop.scale : 0.f;
          pv[4 * t + r] = p;
        }
      }
      const F fp = I::pack(pv);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) o[nt] = I::mma(o[nt], fp, I::slot8(sVT + (nt * 16 + c) * KCT + kp * 32, g));
    }
  }
  if (!active) return;
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  if (g == 0 && q < L) a.LSE[(size_t)bh * L + q] = m + __logf(sum);
  float inv_r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) inv_r[r] = 1.0f / __shfl(sum, (lane & 48) | (4 * g + r), 64);
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qq = qt * 16 + 4 * g + r;
      if (qq < L) a.O[(row_b + qq) * a.ldo + h * HD + nt * 16 + c] = o[nt][r] * inv_r[r];
    }
}

template <int PREC, int HD, int NW, int KC, int LMAX>
__global__ __launch_bounds__(NW * 64) void k_attn_long_bwd(AttnGenArgs ga) {
  typedef Img<PREC> I;
  typedef typename I::E E;
  typedef typename I::F F;
  const AttnArgs& a = ga.a;
  constexpr int RS = HD + 8, KCT = KC + 8, NT = HD / 16, KB = (HD + 31) / 32, V8 = HD / 8, TPC = KC / 16;
  static_assert(HD == 16 || HD == 32 || HD == 64 || HD == 128 || HD == 256, "head sizes");
  static_assert(KC % 32 == 0 && LMAX % KC == 0, "chunks hold whole tile pairs");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  E* sR0 = reinterpret_cast<E*>(smem_raw);   // pass A: K chunk   | pass B: Q chunk (scaled)
  E* sR1 = sR0 + KC * RS;                     // pass A: V chunk   | pass B: dO chunk
  E* sT0 = sR1 + KC * RS;                     // pass A: K^T chunk | pass B: Q^T chunk (scaled)
  E* sT1 = sT0 + HD * KCT;                    //                   | pass B: dO^T chunk
  float* sLse = reinterpret_cast<float*>(sT1 + HD * KCT);   // +inf for padded queries -> P = 0
  float* sDelta = sLse + LMAX;                     // rowsum(dO * O)
  unsigned char* sKv = reinterpret_cast<unsigned char*>(sDelta + LMAX);
  int* sF = reinterpret_cast<int*>(sKv + LMAX);
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int L = a.L;
  const size_t row_b = (size_t)b * L;
  const float* gQ = a.Q + row_b * a.ldq + h * HD;
  const float* gK = a.K + row_b * a.ldk + h * HD;
  const float* gV = a.V + row_b * a.ldv + h * HD;
  const float* gdO = a.dO + row_b * a.lddo + h * HD;
  const float* gO = a.O + row_b * a.ldo + h * HD;
  const bool csk = a.causal && ga.kid == nullptr && ga.fill <= -1e9f;
  const int g0 = blockIdx.y * NW * 16;        // first query (pass A) / key (pass B) row of this group
  const int g1 = g0 + NW * 16 < L ? g0 + NW * 16 : L;
  // delta / LSE of every query a pass can visit: under csk only queries >= g0 (pass B's keys start there, pass A's queries too); the rows
  // up to the end of the last tile pair are written, the passes read no further
  const int rlo = csk ? g0 : 0;
  const int rend = (L + 31) & ~31;
  for (int i = threadIdx.x; i < rend * V8; i += NW * 64) {
    const int r = i / V8, c8 = (i % V8) * 8;
    float part = 0.f;
    if (r >= rlo && r < L) {
      const float4 d0 = *reinterpret_cast<const float4*>(gdO + (size_t)r * a.lddo + c8), d1 = *reinterpret_cast<const float4*>(gdO + (size_t)r * a.lddo + c8 + 4);
      const float4 o0 = *reinterpret_cast<const float4*>(gO + (size_t)r * a.ldo + c8), o1 = *reinterpret_cast<const float4*>(gO + (size_t)r * a.ldo + c8 + 4);
      part = d0.x * o0.x + d0.y * o0.y + d0.z * o0.z + d0.w * o0.w + d1.x * o1.x + d1.y * o1.y + d1.z * o1.z + d1.w * o1.w;
    }
#pragma unroll
    for (int off = V8 / 2; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
    if ((i % V8) == 0) {
      sDelta[r] = part;
      sLse[r] = (r >= rlo && r < L) ? a.LSE[(size_t)bh * L + r] : INFINITY;
    }
  }
  const int first = attn_long_masks<NW * 64, LMAX>(sKv, sF, ga.kid, row_b, L);
  const uint32_t key_rng = drop_key(a.drop);
  const uint32_t idx_bh = (uint32_t)(bh + a.bh_offset) * (uint32_t)L;
  const int nqt = (L + 15) / 16;
  const int tile = blockIdx.y * NW + w;       // the wave's query tile (pass A) / key tile (pass B)
  const bool active = tile < nqt;

  // ---- pass A: dQ of the group's query tiles, key chunks resident ---------------------------------------------------------
  {
    const int q = tile * 16 + c;
    f32x4 dq[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) dq[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    F fq[KB], fdo[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      fq[kb] = gfrag<PREC, HD>(gQ, a.ldq, q, active && q < L, kb, g, a.scale);
      fdo[kb] = gfrag<PREC, HD>(gdO, a.lddo, q, active && q < L, kb, g, 1.0f);
    }
    const int kend = csk ? g1 : L;
    const uint32_t idx_q = (idx_bh + (uint32_t)q) * (uint32_t)L;
    const float fill_q = attn_long_dead(first, q, L, a.causal) ? 0.f : ga.fill;
#pragma unroll 1
    for (int k0 = 0; k0 < kend; k0 += KC) {
      __syncthreads();
      const int Lc = L - k0 < KC ? L - k0 : KC;
      stage_img<PREC, HD, NW * 64>(sR0, sT0, KCT, gK + (size_t)k0 * a.ldk, a.ldk, Lc, KC, 1.0f);
      stage_img<PREC, HD, NW * 64>(sR1, nullptr, KCT, gV + (size_t)k0 * a.ldv, a.ldv, Lc, KC, 1.0f);
      __syncthreads();
      if (!active) continue;
      const float lse_q = sLse[q], delta_q = sDelta[q];      // q < 16 * nqt <= rend
#pragma unroll 1
      for (int kp = 0; kp < TPC / 2; ++kp) {
        if (k0 + kp * 32 >= L) break;
        if (csk && k0 + kp * 32 > tile * 16 + 15) break;   // every key of the pair lies above the diagonal of this query tile
        float dsv[8];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          const int ktl = 2 * kp + tt;
          f32x4 sacc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kb = 0; kb < KB; ++kb) {
            sacc = I::mma(sacc, rfrag_g<PREC, HD>(sR0, ktl * 16 + c, kb, g), fq[kb]);
            dp = I::mma(dp, rfrag_g<PREC, HD>(sR1, ktl * 16 + c, kb, g), fdo[kb]);
          }
          const uint32_t kbits = a.drop.thr ? adt_keep4_any(key_rng, idx_q + (uint32_t)(k0 + ktl * 16 + 4 * g), a.drop.thr, (L & 3) == 0) : 0u;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = k0 + ktl * 16 + 4 * g + r;   // < rend <= LMAX
            const bool masked = (a.causal && key > q) || !sKv[key];
            const float sv = masked ? fill_q : sacc[r];
            const float p = key < L ? __expf(sv - lse_q) : 0.f;
            float d = dp[r];
            if (a.drop.thr) d = ((kbits >> r) & 1u) ? d * a.drop.scale : 0.f;
            dsv[4 * tt + r] = masked ? 0.f : p * (d - delta_q);
          }
        }
        const F fds = I::pack(dsv);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) dq[nt] = I::mma(dq[nt], fds, I::slot8(sT0 + (nt * 16 + c) * KCT + kp * 32, g));
      }
    }
    if (active) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qq = tile * 16 + 4 * g + r;
          if (qq < L) a.dQ[(row_b + qq) * a.lddq + h * HD + nt * 16 + c] = dq[nt][r] * a.scale;
        }
    }
  }

  // ---- pass B: dK, dV of the group's key tiles, query chunks resident -----------------------------------------------------
  {
    const int key = tile * 16 + c;
    const bool key_ok = active && key < L;
    const bool key_attend = key_ok && sKv[key] != 0;
    f32x4 dk[NT], dv[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      dk[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      dv[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    F fk[KB], fv[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      fk[kb] = gfrag<PREC, HD>(gK, a.ldk, key, key_ok, kb, g, 1.0f);
      fv[kb] = gfrag<PREC, HD>(gV, a.ldv, key, key_ok, kb, g, 1.0f);
    }
    const int qbeg = csk ? g0 / KC * KC : 0;     // NW * 16 is a multiple of KC: qbeg == g0 >= rlo
    static_assert((NW * 16) % KC == 0, "a group starts on a chunk boundary");
#pragma unroll 1
    for (int q0 = qbeg; q0 < L; q0 += KC) {
      __syncthreads();
      const int Lc = L - q0 < KC ? L - q0 : KC;
      stage_img<PREC, HD, NW * 64>(sR0, sT0, KCT, gQ + (size_t)q0 * a.ldq, a.ldq, Lc, KC, a.scale);
      stage_img<PREC, HD, NW * 64>(sR1, sT1, KCT, gdO + (size_t)q0 * a.lddo, a.lddo, Lc, KC, 1.0f);
      __syncthreads();
      if (!active) continue;
#pragma unroll 1
      for (int qp = 0; qp < TPC / 2; ++qp) {
        if (q0 + qp * 32 >= L) break;
        if (csk && q0 + qp * 32 + 31 < tile * 16) continue;   // every query of the pair lies before this key tile
        float pv[8], dsv[8];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          const int qtl = 2 * qp + tt;
          f32x4 sacc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kb = 0; kb < KB; ++kb) {
            sacc = I::mma(sacc, rfrag_g<PREC, HD>(sR0, qtl * 16 + c, kb, g), fk[kb]);
            dp = I::mma(dp, rfrag_g<PREC, HD>(sR1, qtl * 16 + c, kb, g), fv[kb]);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int qq = q0 + qtl * 16 + 4 * g + r;     // < rend
            const bool masked = (a.causal && key > qq) || !key_attend;
            const float sv = masked ? (attn_long_dead(first, qq, L, a.causal) ? 0.f : ga.fill) : sacc[r];
            const float p = key_ok ? __expf(sv - sLse[qq]) : 0.f;   // sLse = +inf for padded queries
            float ks = 1.0f;
            if (a.drop.thr) ks = adt_keep(key_rng, (idx_bh + (uint32_t)qq) * (uint32_t)L + (uint32_t)key, a.drop.thr) ? a.drop.scale : 0.f;
            pv[4 * tt + r] = p * ks;
            dsv[4 * tt + r] = masked ? 0.f : p * (dp[r] * ks - sDelta[qq]);
          }
        }
        const F fp = I::pack(pv), fds = I::pack(dsv);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          dv[nt] = I::mma(dv[nt], fp, I::slot8(sT1 + (nt * 16 + c) * KCT + qp * 32, g));
          dk[nt] = I::mma(dk[nt], fds, I::slot8(sT0 + (nt * 16 + c) * KCT + qp * 32, g));
        }
      }
    }
    if (active) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kk = tile * 16 + 4 * g + r;
          if (kk < L) {
            a.dK[(row_b + kk) * a.lddk + h * HD + nt * 16 + c] = dk[nt][r];
            a.dV[(row_b + kk) * a.lddv + h * HD + nt * 16 + c] = dv[nt][r];
          }
        }
    }
  }
}

}  // namespace adt
