// Decoder cross-attention BACKWARD and the token chains behind it in ONE launch per sequence: k_seq_attn_bwd (adt_seqattn.cuh) followed by
// phases A .. D of k_seqtt_mid_bwd (adt_seqpost_tt.cuh) without the trip of dq2 / dk2 / dv2 through HBM between them.
//
// The attention kernel leaves dq2 (pass A) and dk2 / dv2 (pass B) in each wave as transposed 16-token tiles, rounds them to bf16 and stores
// them as saved rows; the mid chain starts by reading exactly those rows back into the same layout (tt_load_bf16).  Here the tiles stay in
// registers -- rounded to bf16 and widened again, as the HBM stream rounds them -- and the mid phases run on them: A / B on the wave's
// pass-A tile, C / D on its pass-B tile.  A tile's result does not depend on which wave computes it, sb_dw_product16 has the same partial
// layout and accumulation order at any wave count, and no sum is reordered: every output is bit-equal to the two-launch path.
//
// 16 waves (one tile per wave and pass up to L = 224).  LDS: the four [R][64] row images of the attention passes in the order K, V, Q, dO,
// keep bits, log-sum-exp, delta, and the 256 bias sums of the mid chain.  R is 128 (L <= 128) or 224 rows, what sb_dw_product16 sweeps: the
// mid chain's token images ARE the Q and dO images (dead behind pass B; their rows beyond the sequence are zero since the prologue).  The four
// weight images of the mid chain (36 KB) land by LDS-DMA in the K / V images behind the barrier that ends pass A (pass B's own key / value
// rows are taken into registers in front of it) and stream under pass B, as does a1; o1, f and d log_feats are requested a phase ahead of their use.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; VGPRs / scratch bytes per lane), 16 waves = 4 per SIMD = at most 128 VGPRs:
//   <64, 0> 128 / 0   <64, 1> 128 / 0   <32, 0> 118 / 0   <32, 1> 128 / 20 (the flagship)   <16, 0> 128 / 0   <16, 1> 128 / 0
// dynamic LDS 147,968 B at L > 128 with two heads (84,992 B at L <= 128); four 16-wide heads fit up to L = 128 only (ADT_LDS_MAX).
// What made it fit: the hand-over tiles are held as packed bf16 operands (xm_put_rows), pass B's key / value operands of a 16-wide head as
// their low halves, and o1 / f / d log_feats are requested between the passes' barriers and not under pass B.
// Four 16-wide heads (HD == 16) have no eight registers to spare in pass B (20 B of scratch per lane with a1 in flight): there a1 is requested
// behind pass B and its round trip is exposed in front of phase A -- the one place where a mid phase does not start without a round trip.
#pragma once
#include "adt_seqattn.cuh"
#include "adt_seqpost_tt.cuh"

namespace adt {

constexpr int XM_NW = 16;

struct XattnMidArgs {
  // cross-attention core (AttnArgs on its lean path): q2, k2, v2, o2 saved as bf16 rows, dO fp32
  const __bf16* Q; const __bf16* K; const __bf16* V; const __bf16* O; int ldq, ldk, ldv, ldo;
  const float* LSE; const float* dO; int lddo; int L;
  const uint32_t* mask; float scale; DropCfg drop;      // MODE 1 reads the forward's keep bits: no RNG index, no batch offset
  // mid chain (BwdChainArgs): a1, o1, log_feats ; weights Wq, Wo1, Wk, Wv as pre-packed images ; out0 = dO1, out1 = d log_feats
  const float* xin; const float* o; const float* f; const float* wp_base; const void* wp_img;
  const float* W0; const float* W1; const float* W2; const float* W3;
  float* out0; float* out1; int acc1; int nrep; size_t rep_stride;
  float* db0; float* db1; float* db2; float* db3; float* vpart;
  float* part[4]; size_t part_stride;
  void* do_bf16; float* do_delta; float do_scale;      // hand-over of dO1 to the self-attention backward (BwdChainArgs: do_bf16 ; the head size is HD)
  const __bf16* dO_bf16; const float* dO_delta;        // hand-over of dO2 FROM k_seqtt_post_bwd<DEC> (AttnArgs: do_bf16, do_delta): dO and O are not read
  unsigned long long* stamps;      // timing experiments only (ADT_SEQ_STAMPS=6): s_memtime per wave of workgroup 0
  const int* pad_pre;              // pad prefix of every DECODER sequence (AttnArgs / BwdChainArgs::pad_pre; nullptr: none).  A query tile wholly inside it:
                                   // the handed-over dO2 rows and delta are exact zeros (k_seqtt_post_bwd<DEC> masks its gradient), hence dq2 = 0 and
                                   // a1 / o1 only multiply zeros -- none of the four is requested.  K, V, f (encoder rows) and the keys' gradients stay
};

__host__ __device__ inline int xm_rows(int L) { return (L + 31) / 32 <= 4 ? 128 : SB_R; }       // image rows = rows sb_dw_product16 sweeps
__host__ __device__ inline size_t xm_lds_bytes(int L, int H) {
  const size_t R = (size_t)xm_rows(L);
  return 4 * R * TT_RS * 2 + (size_t)H * R * 8 * 4 + 2 * (size_t)H * R * 4 + 256 * 4;
}

// The hand-over.  k_seq_attn_bwd rounds a gradient tile to bf16 for its store and k_seqtt_mid_bwd widens the loaded rows to fp32 only to round
// them again, unchanged, into its MFMA operands and image rows (tt_bfrags, tt_put_rows): the tile is kept as those operands, half the registers
// of the widened form.  Element (nt, r) of a TT tile is element 4 (nt & 1) + r of kb[nt >> 1].  Lanes without a token hold zeros, as
// tt_load_bf16 gives them.
ADT_DEVICE_INLINE TTB xm_zero() {
  TTB t;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int j = 0; j < 8; ++j) t.kb[kb][j] = (__bf16)0.f;
  return t;
}
ADT_DEVICE_INLINE void xm_put_rows(__bf16* img, int token, const TTB& t) {      // tt_put_rows of the widened tile
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    bf16x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = t.kb[nt >> 1][4 * (nt & 1) + r];
    *reinterpret_cast<bf16x4*>(img + token * TT_RS + 16 * nt + 4 * (int)((threadIdx.x & 63) >> 4)) = v;
  }
}

template <int HD, int MODE>
__global__ __launch_bounds__(XM_NW * 64) void k_seqtt_xattn_mid_bwd(XattnMidArgs a) {
  static_assert(sizeof(XattnMidArgs) <= 512, "kernel-argument prefetch covers 512 bytes");
  static_assert(MODE == 0 || MODE == 1, "no dropout, or keep bits saved by the forward");
  adt_prefetch_kernargs<sizeof(XattnMidArgs)>();      // adt_common.cuh
  constexpr int H = 64 / HD, NT = HD / 16, KB = (HD + 31) / 32, NF = H * KB, NW = XM_NW;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int L = a.L, R = xm_rows(L);
  __bf16* sK = reinterpret_cast<__bf16*>(smem_raw);
  __bf16* sV = sK + R * TT_RS;
  __bf16* sQ = sV + R * TT_RS;
  __bf16* sdO = sQ + R * TT_RS;
  uint32_t* sM = reinterpret_cast<uint32_t*>(sdO + R * TT_RS);     // [H][R][8] dropout keep bits of the forward, 0 beyond L
  float* sLse = reinterpret_cast<float*>(sM + (size_t)H * R * 8);   // [H][R] log2-domain log-sum-exp (+inf beyond L)
  float* sDelta = sLse + H * R;                                     // [H][R] rowsum(dO * O) per head
  float* sRed = sDelta + H * R;                                     // the four bias gradients of the mid chain
  __bf16* wimg = sK;                                                // behind pass A: Wq^T, Wo1^T, Wk^T, Wv^T (>= 36 KB: R >= 128)
  __bf16* img0 = sQ;                                                // behind pass B: the G and X token images of the weight-gradient products
  __bf16* img1 = sdO;
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const size_t row_b = (size_t)b * L;
  const float qmul = a.scale * 1.4426950408889634f;
  const int nqt = (L + 15) / 16, npair = (L + 31) / 32;
#define XM_STAMP(k) do { if (a.stamps && blockIdx.x == 0 && lane == 0) a.stamps[w * 16 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
  XM_STAMP(0);
  const int padn = (HD != 16 && a.pad_pre) ? a.pad_pre[b] : 0;      // (workgroup-uniform) requested first, consumed behind the keep-bit and log-sum-exp requests (not with 16-wide heads: StepPlan::pad_elide)
  if (a.nrep > 1) {      // bias-gradient replicas (vpart == nullptr): see sp_replica
    const size_t off = (size_t)(blockIdx.x % a.nrep) * a.rep_stride;
    if (a.db0) a.db0 += off;
    if (a.db1) a.db1 += off;
    if (a.db2) a.db2 += off;
    if (a.db3) a.db3 += off;
  }
  // ---- prologue: every load is unconditional (lanes without an element read a block of zeros), the small tables are requested first and
  // everything is in flight before the first LDS store that waits for a load (adt_seqbwd_tt.cuh: k_seqtt_attn_pre_bwd) -------------------
  constexpr int NTH = NW * 64;
  constexpr int MI = (H * SB_R * 2 + NTH - 1) / NTH, LI = (H * SB_R + NTH - 1) / NTH, II = (SB_R * 8 + NTH - 1) / NTH;
  typedef const tt_u4 __attribute__((address_space(1))) * gu4;
  typedef const float __attribute__((address_space(1))) * gf1;
  typedef const bf16x4 __attribute__((address_space(1))) * gb4;
  typedef const f32x4 __attribute__((address_space(1))) * gp4;
  tt_u4 mreg[MI];
  float lreg[LI];
  if constexpr (MODE == 1) {
    adt_static_for<MI>([&](auto k) {
      const int i = threadIdx.x + k * NTH, hr = i >> 1, h = hr / R, r = hr - h * R;
      const bool ok = i < H * R * 2 && r < L;
      const gu4 p = ok ? (gu4)(a.mask + ((size_t)(b * H + h) * L + r) * 8) + (i & 1) : (gu4)tt_zero_row;
      mreg[k] = *p;
    });
  }
  adt_static_for<LI>([&](auto k) {
    const int i = threadIdx.x + k * NTH, h = i / R, r = i - h * R;
    const bool ok = i < H * R && r < L;
    const float v = *(ok ? (gf1)(a.LSE + (size_t)(b * H + h) * L + r) : (gf1)tt_zero_row);
    lreg[k] = ok ? v * 1.4426950408889634f : INFINITY;
  });
  // images: 8 features per thread and step.  Saved rows are in the register order of a transposed tile (adt_tt.cuh: tt_store_bf16): features
  // c8 .. c8+3 and c8+4 .. c8+7 of a 64-feature row are two 8-byte pieces at 16 g + 4 nt and 16 (g + 1) + 4 nt, nt = c8 / 16, g = (c8 / 4) % 4
  bf16x4 qa[II], qc[II], ka[II], kc[II], va[II], vc[II], oa[II], oc[II], da[II], dc[II];
  f32x4 d0[II], d1[II];
  float dlt[II];
  const bool hand = a.dO_bf16 != nullptr;      // (workgroup-uniform) dO as bf16 operand rows + delta: no fp32 dO, no O
  adt_static_for<II>([&](auto k) {
    const int i = threadIdx.x + k * NTH, r = i >> 3, c8 = (i & 7) * 8;
    const bool ok = r < L;
    const int pa = 16 * ((c8 >> 2) & 3) + 4 * (c8 >> 4);
    const size_t row = row_b + r;
    // one selected base per tensor, the pieces at fixed offsets from it (tt_load_bf16's form: with a select per piece hipcc folded the loads of
    // the zero block away and put the real ones back inside branches, each with its wait)
    const gb4 zb = (gb4)tt_zero_row + (i & 7);
    const gb4 pq = ok ? (gb4)(a.Q + row * a.ldq + pa) : zb, pk = ok ? (gb4)(a.K + row * a.ldk + pa) : zb;
    const gb4 pv = ok ? (gb4)(a.V + row * a.ldv + pa) : zb, po = ok ? (gb4)(a.O + row * a.ldo + pa) : zb;
    qa[k] = pq[0]; qc[k] = pq[4]; ka[k] = pk[0]; kc[k] = pk[4]; va[k] = pv[0]; vc[k] = pv[4];      // pb = pa + 16 elements
    if (hand) {
      const bool okd = ok && !tt_pad_tile(r >> 4, padn, L);      // (wave-uniform: a wave holds eight whole rows of one tile) zeros, as stored
      const gb4 pdb = okd ? (gb4)(a.dO_bf16 + row * 64 + pa) : zb;
      da[k] = pdb[0]; dc[k] = pdb[4];
      dlt[k] = *(okd ? (gf1)(a.dO_delta + row * 4 + (i & 7) / (HD / 8)) : (gf1)tt_zero_row);      // the chunk's head
    } else {
      const gp4 pd = ok ? (gp4)(a.dO + row * a.lddo + c8) : (gp4)tt_zero_row + (i & 7);
      oa[k] = po[0]; oc[k] = po[4];
      d0[k] = pd[0]; d1[k] = pd[1];
    }
  });
  XM_STAMP(1);
  if constexpr (MODE == 1) {
    adt_static_for<MI>([&](auto k) {
      const int i = threadIdx.x + k * NTH;
      if (i < H * R * 2) reinterpret_cast<tt_u4*>(sM + (size_t)(i >> 1) * 8)[i & 1] = mreg[k];
    });
  }
  adt_static_for<LI>([&](auto k) {
    const int i = threadIdx.x + k * NTH;
    if (i < H * R) sLse[i] = lreg[k];
  });
  if (threadIdx.x < 256) sRed[threadIdx.x] = 0.f;
  // delta from the same dO / O chunks, in the order of k_seq_attn_bwd: the eight products of a chunk, then the chunks of a head (adjacent lanes)
  adt_static_for<II>([&](auto k) {
    const int i = threadIdx.x + k * NTH, r = i >> 3, c8 = (i & 7) * 8;
    float q[8], kk[8], v[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      q[j] = (float)qa[k][j]; q[4 + j] = (float)qc[k][j]; kk[j] = (float)ka[k][j]; kk[4 + j] = (float)kc[k][j];
      v[j] = (float)va[k][j]; v[4 + j] = (float)vc[k][j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] *= qmul;
    const bool in = i < R * 8;      // (wave-uniform)
    if (in) {
      *reinterpret_cast<bf16x8*>(sQ + r * TT_RS + c8) = pack8(q);
      *reinterpret_cast<bf16x8*>(sK + r * TT_RS + c8) = pack8(kk);
      *reinterpret_cast<bf16x8*>(sV + r * TT_RS + c8) = pack8(v);
    }
    float part;
    if (hand) {      // the rows already are bf16(dO * drop.scale), delta the head's sum in this kernel's order (adt_tt.cuh: tt_head_delta_chunks)
      bf16x8 db;
#pragma unroll
      for (int j = 0; j < 4; ++j) { db[j] = da[k][j]; db[4 + j] = dc[k][j]; }
      if (in) *reinterpret_cast<bf16x8*>(sdO + r * TT_RS + c8) = db;
      part = dlt[k];
    } else {
      float d[8], o[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) { o[j] = (float)oa[k][j]; o[4 + j] = (float)oc[k][j]; d[j] = d0[k][j]; d[4 + j] = d1[k][j]; }
      part = tt_chunk_delta(d, o);
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] *= a.drop.scale;      // the dO image carries 1 / (1 - p): see sab_pass_a
      if (in) *reinterpret_cast<bf16x8*>(sdO + r * TT_RS + c8) = pack8(d);
#pragma unroll
      for (int off = HD / 16; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);      // HD/8 adjacent lanes hold one head's chunks
    }
    if (in && ((i & 7) % (HD / 8)) == 0) sDelta[((i & 7) / (HD / 8)) * R + r] = part;
  });
  XM_STAMP(2);
  __syncthreads();
  XM_STAMP(3);
  const uint32_t key_rng = 0u;      // (MODE 2 only)
  const float ln2 = 0.6931471805599453f;
  // one tile per wave and pass: heaviest causal tile first, balanced over the SIMDs (sab_rank16); waves beyond the tile count idle in the
  // attention passes and the token phases, and take their share of the weight-gradient products
  const int rk = sab_rank16(w);
  const bool has = rk < nqt;
  const int qt = has ? nqt - 1 - rk : 0, kt = has ? rk : 0;
  const int lA = qt * 16 + c, lB = kt * 16 + c;
  const bool validA = has && lA < L, validB = has && lB < L;
  const size_t rowA = row_b + lA, rowB = row_b + lB;
  const bool liveA = validA && !(hand && tt_pad_tile(qt, padn, L));      // a1 / o1 of a padded query tile multiply dq2 = 0 and da1 = 0

  // ---- pass A: dQ (the wave owns query tile qt, keys on the accumulator rows) ------------------------------------------------------------
  TTB dq = xm_zero();
  bf16x4 fkl[NF], fkh[NF], fvl[NF], fvh[NF];      // halves of the sab_rowfrag operands: a 16-wide head has no high half (zeros) and holds none
  if (has) {
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const float lse_q = sLse[h * R + lA], delta_q = sDelta[h * R + lA];
      bf16x8 fq[KB], fdo[KB];
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        fq[kb] = sab_rowfrag<HD>(sQ, lA, h, kb, g);
        fdo[kb] = sab_rowfrag<HD>(sdO, lA, h, kb, g);
      }
      f32x4 t[NT];
      sab_pass_a<HD, MODE>(sK, sV, fq, fdo, lse_q, delta_q, sM + ((size_t)h * R + lA) * 8, qt, h, a.drop, key_rng, 0u, c, g, t);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) dq.kb[(h * NT + nt) >> 1][4 * ((h * NT + nt) & 1) + r] = (__bf16)(validA ? t[nt][r] * a.scale : 0.f);
    }
    // pass B's own key / value rows, while the K / V images are still there
#pragma unroll
    for (int h = 0; h < H; ++h)
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const bf16x8 k8 = sab_rowfrag<HD>(sK, lB, h, kb, g), v8 = sab_rowfrag<HD>(sV, lB, h, kb, g);
#pragma unroll
        for (int j = 0; j < 4; ++j) { fkl[h * KB + kb][j] = k8[j]; fkh[h * KB + kb][j] = k8[4 + j]; fvl[h * KB + kb][j] = v8[j]; fvh[h * KB + kb][j] = v8[4 + j]; }
      }
  }
  XM_STAMP(4);
  __syncthreads();          // nobody reads the K / V images any more
  XM_STAMP(5);
  // the mid chain's weight images into their place, and phase A / B's activations: they stream under pass B
  {
    const float* const ws4[4] = {a.W0, a.W1, a.W2, a.W3};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      adt_glds_block<NW>(reinterpret_cast<const __bf16*>(a.wp_img) + 6 * (ws4[j] - a.wp_base) + 3 * WPACK_IMG, wimg + j * TT_WIMG, TT_WIMG * 2);
  }
  // (four 16-wide heads: pass B has no eight registers to spare -- 20 bytes of scratch per lane -- and a1 is requested behind it)
  TTSaved a1req;
  if constexpr (HD != 16) a1req = tt_saved_request(a.xin, rowA, liveA, g, 1);

  // ---- pass B: dK, dV (the wave owns key tile kt, queries on the accumulator rows) -------------------------------------------------------
  TTB dk = xm_zero(), dv = xm_zero();
  if (has) {
#pragma unroll
    for (int h = 0; h < H; ++h) {
      f32x4 tk[NT], tv[NT];
      bf16x8 fk[KB], fv[KB];
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          fk[kb][j] = fkl[h * KB + kb][j]; fk[kb][4 + j] = HD == 16 ? (__bf16)0.f : fkh[h * KB + kb][j];
          fv[kb][j] = fvl[h * KB + kb][j]; fv[kb][4 + j] = HD == 16 ? (__bf16)0.f : fvh[h * KB + kb][j];
        }
      sab_pass_b<HD, MODE>(sQ, sdO, fk, fv, sLse + h * R, sDelta + h * R, sM + (size_t)h * R * 8, kt, nqt, h, a.drop, key_rng, 0u, L,
                           c, g, tk, tv);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // the Q image carries the factor log2(e) / sqrt(hd): dK = dS^T Q / sqrt(hd)
          dk.kb[(h * NT + nt) >> 1][4 * ((h * NT + nt) & 1) + r] = (__bf16)(validB ? tk[nt][r] * ln2 : 0.f);
          dv.kb[(h * NT + nt) >> 1][4 * ((h * NT + nt) & 1) + r] = (__bf16)(validB ? tv[nt][r] : 0.f);
        }
    }
  }
  if constexpr (HD == 16) a1req = tt_saved_request(a.xin, rowA, liveA, g, 1);
  XM_STAMP(6);
  adt_wait_vm0();           // the LDS-DMA of the weight images has landed: published by this barrier
  __syncthreads();          // nobody reads the Q / dO images any more: they become the token images (rows beyond the sequence are zero)
  XM_STAMP(7);
  // ---- A: cross-attention query projection: da1 = dq2 Wq ; dWq = dq2^T a1 ----------------------------------------------------------------
  TT da1 = tt_zero();
  // Every workgroup of the launch is in the same phase at the same time, so each phase's global loads and stores are one burst, and vmcnt
  // retires loads and stores in issue order.  o1 and f (consumed in B and C) are requested here, d log_feats (consumed in D) in front of phase
  // B's dO1 stores and not behind them.  (Stamps of single workgroups do not separate this order from k_seqtt_mid_bwd's, f in B and d log_feats
  // in C: 76.0k and 72.9k cycles for the kernel in two samples against 73.3k, the waits move between the phases -- profiles/r11_xattn_mid_fused.txt.)
  const TTSaved oreq = tt_saved_request(a.o, rowA, liveA, g, 1);
  const TT fx = tt_load(a.f + rowB * 64, validB, g);
  if (has) {
    xm_put_rows(img0, lA, dq);
    tt_put_rows(img1, lA, tt_saved_value(a1req, 1), validA, g);
    da1 = tt_gemm(dq, wimg, c, g);
  }
  __syncthreads();
  sb_dw_product16<NW>(img0, img1, npair, nullptr, a.part[0] + (size_t)blockIdx.x * a.part_stride, sRed, w, c, g);
  __syncthreads();
  XM_STAMP(8);
  // ---- B: self-attention out_proj: dO1 = da1 Wo1 ; dWo1 = da1^T o1 ------------------------------------------------------------------------
  const TT acc1v = tt_load(a.out1 + rowB * 64, validB && a.acc1, g);
  if (has) {
    tt_put_rows(img0, lA, da1, validA, g);
    const TT o1 = tt_saved_value(oreq, 1);
    tt_put_rows(img1, lA, o1, validA, g);
    sp_store_do1(a.out0, a.do_bf16, a.do_delta, a.do_scale, HD, rowA, tt_gemm(tt_bfrags(da1), wimg + TT_WIMG, c, g), o1, validA, g);
  }
  __syncthreads();
  sb_dw_product16<NW>(img0, img1, npair, nullptr, a.part[1] + (size_t)blockIdx.x * a.part_stride, sRed + 64, w, c, g);
  __syncthreads();
  XM_STAMP(9);
  // ---- C: cross-attention keys: df = dk2 Wk ; dWk = dk2^T f -----------------------------------------------------------------------------------
  TT df = tt_zero();
  if (has) {
    xm_put_rows(img0, lB, dk);
    tt_put_rows(img1, lB, fx, validB, g);
    df = tt_gemm(dk, wimg + 2 * TT_WIMG, c, g);
  }
  __syncthreads();
  sb_dw_product16<NW>(img0, img1, npair, nullptr, a.part[2] + (size_t)blockIdx.x * a.part_stride, sRed + 128, w, c, g);
  __syncthreads();
  XM_STAMP(10);
  // ---- D: cross-attention values (the X image still holds f) -------------------------------------------------------------------------------
  if (has) {
    xm_put_rows(img0, lB, dv);
    tt_add(df, tt_gemm(dv, wimg + 3 * TT_WIMG, c, g));
    tt_add(df, acc1v);                                                        // zeros unless a.acc1
    tt_store(a.out1 + rowB * 64, df, validB, g);
  }
  __syncthreads();
  sb_dw_product16<NW>(img0, img1, npair, nullptr, a.part[3] + (size_t)blockIdx.x * a.part_stride, sRed + 192, w, c, g);
  __syncthreads();          // the last product's bias sums
  XM_STAMP(11);
  {
    const int t = threadIdx.x;
    float* const dst[4] = {a.db0, a.db1, a.db2, a.db3};
    if (t < 256) {
      if (a.vpart) a.vpart[(size_t)blockIdx.x * 512 + t] = sRed[t];
      else atomicAdd(dst[t >> 6] + (t & 63), sRed[t]);
    }
  }
  XM_STAMP(12);
#undef XM_STAMP
}

}  // namespace adt
