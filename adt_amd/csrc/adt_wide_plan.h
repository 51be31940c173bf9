// Which kernel a call of the "wide" C ABI gets (adt_dense_fwd, adt_dense_bwd, adt_attn_masked_*), decided once into a struct.  Plain C++17:
// no HIP, no library state, no device pointers (and nothing exported: every function is static inline or constexpr), so the table is printed and checked by a host program (tests/test_wide_plan_cpu.py).
// adt_wide.hip fills the facts, asks for the plan and launches what it names; the tile constants the decisions need live here and the
// kernel headers include this file.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/adt_hip.h"

constexpr size_t ADT_LDS_MAX = 160 * 1024;      // per workgroup on gfx950

namespace adt {

// ---- tile constants (adt_gemm.cuh, adt_dense_rows.cuh) -------------------------------------------------------------------------------
constexpr int GBM = 128, GBK = 32, GTH = 256;   // BK = 64 measured slower at d = 256 (fewer waves per SIMD), faster only at d = 64
constexpr int DW64_ROWS = 128, DW64_NTH = 256;
constexpr int DW64_PART = 4096 + 64;
constexpr int DWP_TS = 32, DWP_NTH = 512, DWP_IMG = 32 * 256 * 2;
constexpr int DWP_PART_BYTES = 256 * 256 * 4;      // one workgroup's private 256 x 256 partial of k_dense_dw256
constexpr int ROWS_NW = 8;                  // waves per workgroup
constexpr int ROWS_PC = 256;                // output columns per weight panel
constexpr int DW_BN = 256, DW_BK = 128, DW_TS = 64, DW_NTH = 512;
constexpr size_t DW_LDS_BYTES = 2 * (size_t)(8 * DW_BN * 8 + 8 * DW_BK * 8) * 2;     // 96 KB of bf16

static inline int xcd_grid(int n_outer, int n_inner) { return n_outer < 16 ? n_outer * n_inner : (n_outer + 7) / 8 * 8 * n_inner; }
static inline size_t rows_lds_bytes(int contraction, int pc) { return (size_t)pc * (contraction + 8) * 2 + (size_t)pc * sizeof(float); }
// the 128 x BN + BN x 32 operand tiles of the tiled kernels: fp32 rows of 36, bf16 rows of 40 (adt_gemm.cuh: GemmLds, gemm_lds_bytes)
constexpr size_t gemm_tile_lds_bytes(bool bf16, int bn) { return (size_t)(GBM + bn) * (bf16 ? GBK + 8 : GBK + 4) * (bf16 ? 2 : 4); }

constexpr int plan_ceil(int a, int b) { return (a + b - 1) / b; }
constexpr int plan_round(int a, int b) { return plan_ceil(a, b) * b; }
constexpr int plan_max(int a, int b) { return a > b ? a : b; }
constexpr int plan_min(int a, int b) { return a < b ? a : b; }

// ---- dense layers --------------------------------------------------------------------------------------------------------------------
// *_ok: the operand's base is 16-byte aligned and its row stride a multiple of 4 floats (bias: the base only).  Read only where the
// operand is present; g is the forward's Y and the backward's dY.
struct DenseFacts {
  int prec, T, K, N;
  bool has_bias, has_u, has_r, has_r2, has_mask, has_drop, has_act, has_dx, has_dw, beta;
  bool x_ok, w_ok, g_ok, bias_ok, u_ok, r_ok, r2_ok, dx_ok;
  bool rows_on;             // adt_dense_rows_enable
  bool stage256_on;         // ADT_STAGE256
  int64_t ws_bytes;         // adt_dense_workspace; 0: none registered
};

enum DenseFwdArm { F256, FROWS, FTILED };
struct DenseFwdPlan {
  DenseFwdArm arm;
  int grid_x, grid_y, block;
  size_t lds_bytes;         // dynamic LDS
  int chunk, epi;           // F256: rows of T per workgroup; epilogue 1 residual / row mask | 2 dropout | 4 activation / saved U
  int pc, n_panels, row_groups, kb, ch;      // FROWS: panel width and count, workgroups per panel, k_dense_fwd_rows<KB, CH>
  int bn, nt_m, nt_n;       // FTILED: k_dense_fwd<PREC, BN> and its tile counts
};

// the row-streaming launch (k_dense_fwd_rows, k_dense_dx_rows): one workgroup per CU and panel group, twice that while two fit the LDS;
// never more row groups than 16-row tiles / waves
struct RowsGrid { int pc, n_panels, row_groups; size_t lds_bytes; };
static inline RowsGrid adt_rows_grid(int T, int cols, int contraction) {
  RowsGrid r;
  r.pc = cols >= ROWS_PC ? ROWS_PC : plan_round(cols, 16);
  r.n_panels = plan_ceil(cols, r.pc);
  r.lds_bytes = rows_lds_bytes(contraction, r.pc);
  int nrg = 256 / r.n_panels;
  if (r.lds_bytes <= 64 * 1024) nrg *= 2;
  r.row_groups = plan_max(plan_min(nrg, plan_ceil(plan_ceil(T, 16), ROWS_NW)), 1);
  return r;
}

// T split over at most `cap` workgroups in chunks of whole `tile`-row stages
static inline int adt_t_chunk(int T, int cap, int tile) { return plan_round(plan_ceil(T, plan_min(plan_ceil(T, tile), cap)), tile); }

static inline DenseFwdPlan adt_dense_fwd_plan(const DenseFacts& f) {
  DenseFwdPlan p{};
  const bool bf16 = f.prec != ADT_PREC_F32;
  const bool extras_ok = (!f.has_u || f.u_ok) && (!f.has_r || f.r_ok) && (!f.has_r2 || f.r2_ok);
  if (bf16 && f.rows_on && f.K == 256 && f.N % 256 == 0 && f.N <= 1024 && f.x_ok && f.w_ok && f.g_ok && extras_ok && f.stage256_on) {
    // K = 256, N = 256 .. 1024: weight rows in registers, activations through LDS, compile-time epilogue on rows (adt_gemm.cuh: k_dense_fwd256)
    p.arm = F256;
    p.chunk = adt_t_chunk(f.T, f.N > 256 ? 512 / (f.N / 256) : 256, DWP_TS);
    p.grid_x = plan_ceil(f.T, p.chunk); p.grid_y = f.N / 256; p.block = DWP_NTH;
    p.epi = ((f.has_r || f.has_r2 || f.has_mask) ? 1 : 0) | (f.has_drop ? 2 : 0) | ((f.has_act || f.has_u) ? 4 : 0);
    return p;
  }
  if (bf16 && f.rows_on && (f.K == 64 || f.K == 128 || f.K == 256) && f.N % 4 == 0 && f.g_ok && (!f.has_bias || f.bias_ok) && extras_ok) {
    p.arm = FROWS;
    const RowsGrid r = adt_rows_grid(f.T, f.N, f.K);
    p.pc = r.pc; p.n_panels = r.n_panels; p.row_groups = r.row_groups; p.lds_bytes = r.lds_bytes;
    p.grid_x = r.row_groups * r.n_panels; p.grid_y = 1; p.block = ROWS_NW * 64;
    // residual loads run one chunk of CH column tiles ahead (double buffered in registers): 8 tiles, or 4 when there are two residuals
    p.kb = f.K / 32; p.ch = f.has_r2 ? 4 : 8;
    return p;
  }
  p.arm = FTILED;
  p.bn = f.N > 64 ? 128 : 64;
  p.nt_n = f.N > 64 ? plan_ceil(f.N, 128) : 1;
  p.nt_m = plan_ceil(f.T, GBM);
  p.grid_x = xcd_grid(p.nt_m, p.nt_n); p.grid_y = 1; p.block = GTH;      // XCD-aware 1-D launch (xcd_tile)
  p.lds_bytes = gemm_tile_lds_bytes(bf16, p.bn);
  return p;
}

enum DenseDxArm { DXNONE, DX256, DXROWS, DXTILED };
enum DenseDwArm { DWNONE, DW256, DWROWS, DW64, DWTILED };
struct DxPiece { int n0, chunk, beta, kb, row_groups; size_t lds_bytes; };      // columns [n0, n0 + chunk) of G, k_dense_dx_rows<KB, has_u>
struct DenseBwdPlan {
  DenseDxArm dx;
  int dx_grid_x, dx_grid_y, dx_block;
  size_t dx_lds_bytes;
  int nb, dx_chunk;                          // DX256: k_dense_dx256<NB>, rows of T per workgroup
  int n_pieces, pc, n_panels; bool has_u;    // DXROWS: contraction pieces of <= 256 columns of G / rows of W over one panel layout of K
  DxPiece piece[16];
  int dx_bn, gx, gy, dx_splits, n_chunk; bool dx_zero_fill;      // DXTILED: k_dense_bwd_dx<PREC, BN>, K tiles, T tiles, N splits
  DenseDwArm dw;
  int dw_grid_x, dw_grid_y, dw_block;
  size_t dw_lds_bytes;
  int dw_chunk;                              // rows of T per workgroup / split, every arm
  int nwg, blocks, kblocks;                  // DW256, DW64: workgroups along T, 256 x 256 / 64 x 64 output blocks, blocks along K
  int per, reduce_groups;                    // DW256: k_dense_dw256_reduce folds `per` partials per workgroup
  int64_t ws_used;                           // DW256, DW64 with partials: bytes of the registered workspace written
  bool partials;                             // DW64: private partials + an ordered sum; else float atomics
  int dw_splits, n_blocks, k_blocks;         // DWROWS; DWTILED: splits
  int dw_bn, dw_gx, dw_gy;                   // DWTILED: k_dense_bwd_dw<PREC, BN>, K tiles, N tiles
};

static inline void adt_dense_dx_plan(const DenseFacts& f, DenseBwdPlan& p) {
  const bool bf16 = f.prec != ADT_PREC_F32, act_ok = !f.has_act || f.u_ok;
  const int T = f.T, K = f.K, N = f.N;
  p.dx = DXNONE;
  if (!f.has_dx) return;
  if (bf16 && f.rows_on && N % 256 == 0 && N <= 768 && K == 256 && f.w_ok && f.g_ok && act_ok && f.stage256_on) {
    // contraction 256 / 512 / 768 into 256 columns: weight in registers, gradient tiles through LDS, transposed output (adt_gemm.cuh:
    // k_dense_dx256; wider outputs -- K = 1024 as four column blocks -- measured neutral against the row-streaming kernel and stay there)
    p.dx = DX256;
    p.nb = N / 256;
    p.dx_chunk = adt_t_chunk(T, 256, DWP_TS);
    p.dx_grid_x = plan_ceil(T, p.dx_chunk); p.dx_grid_y = K / 256; p.dx_block = DWP_NTH;
    p.dx_lds_bytes = (size_t)DWP_IMG * p.nb;
    return;
  }
  if (bf16 && f.rows_on && N % 64 == 0 && N <= 1024 && K % 4 == 0 && f.dx_ok && f.g_ok && act_ok) {
    p.dx = DXROWS;
    p.has_u = f.has_act;
    p.dx_block = ROWS_NW * 64;
    for (int n0 = 0; n0 < N;) {
      // with an activation the saved pre-activation rides along in registers: contraction chunks of 128 instead of 256
      const int chunk = (N - n0 >= 256 && !f.has_act) ? 256 : (N - n0 >= 128 ? 128 : 64);
      const RowsGrid r = adt_rows_grid(T, K, chunk);
      p.pc = r.pc; p.n_panels = r.n_panels;
      p.piece[p.n_pieces++] = DxPiece{n0, chunk, (n0 > 0 || f.beta) ? 1 : 0, chunk / 32, r.row_groups, r.lds_bytes};      // every piece after the first accumulates
      n0 += chunk;
    }
    return;
  }
  p.dx = DXTILED;
  p.dx_bn = K > 64 ? 128 : 64;
  p.gx = K > 64 ? plan_ceil(K, 128) : 1; p.gy = plan_ceil(T, GBM);
  // long contractions over few output tiles (the all-item logits: N = V + 100) are split over blockIdx.z
  p.dx_splits = 1;
  if (N >= 4096 && p.gx * p.gy < 1024) {
    const int want = plan_min(plan_ceil(2048, p.gx * p.gy), 32);
    p.n_chunk = plan_round(plan_ceil(N, want), GBK);
    p.dx_splits = plan_ceil(N, p.n_chunk);
    p.dx_zero_fill = p.dx_splits > 1 && !f.beta;
  }
  p.dx_grid_x = xcd_grid(p.gy, p.gx * p.dx_splits); p.dx_grid_y = 1; p.dx_block = GTH;
  p.dx_lds_bytes = gemm_tile_lds_bytes(bf16, p.dx_bn);
}

static inline void adt_dense_dw_plan(const DenseFacts& f, DenseBwdPlan& p) {
  const bool bf16 = f.prec != ADT_PREC_F32, rows = bf16 && f.rows_on && f.x_ok && f.g_ok;
  const int T = f.T, K = f.K, N = f.N;
  p.dw = DWNONE;
  if (!f.has_dw) return;
  if (rows && N % 256 == 0 && K % 256 == 0 && (N / 256) * (K / 256) <= 4) {
    // the whole 256 x 256 product (of each 256 x 256 block) per workgroup, private partials in the registered workspace + a reduce
    // (adt_gemm.cuh: k_dense_dw256); 256 workgroups in all
    const int blocks = (N / 256) * (K / 256), nwg0 = plan_min(plan_ceil(T, DWP_TS), 256 / blocks);
    if ((int64_t)nwg0 * blocks * DWP_PART_BYTES <= f.ws_bytes) {
      p.dw = DW256;
      p.blocks = blocks; p.kblocks = K / 256;
      p.dw_chunk = plan_round(plan_ceil(T, nwg0), DWP_TS);
      p.nwg = plan_ceil(T, p.dw_chunk);
      p.per = p.nwg >= 128 ? 32 : 16; p.reduce_groups = plan_ceil(p.nwg, p.per);
      p.ws_used = (int64_t)nwg0 * blocks * DWP_PART_BYTES;
      p.dw_grid_x = p.nwg; p.dw_grid_y = blocks; p.dw_block = DWP_NTH;
      return;
    }
  }
  // the 256 x 128-block kernel pays off from four output blocks on (N = 768: 127 us vs 225 us tiled); at two blocks (256 x 256)
  // its 32 K atomics per workgroup cost what the deeper stages save (84 us vs 77 us)
  if (rows && plan_ceil(N, DW_BN) * plan_ceil(K, DW_BK) >= 4 && N % 4 == 0 && K % 4 == 0 && (!f.has_act || f.u_ok)) {
    p.dw = DWROWS;
    p.n_blocks = plan_ceil(N, DW_BN); p.k_blocks = plan_ceil(K, DW_BK);
    const int tiles = p.n_blocks * p.k_blocks;
    // one workgroup per CU (96 KB of LDS): 256 workgroups when the T chunks stay >= 4 stages, chunks are multiples of 64 rows
    p.dw_chunk = plan_max(plan_round(plan_ceil(T, tiles >= 256 ? 1 : 256 / tiles), DW_TS), DW_TS);
    p.dw_splits = plan_ceil(T, p.dw_chunk);
    p.dw_grid_x = xcd_grid(p.dw_splits, tiles); p.dw_grid_y = 1; p.dw_block = DW_NTH;
    p.dw_lds_bytes = DW_LDS_BYTES;
    return;
  }
  if (rows && N % 64 == 0 && K % 64 == 0 && (N / 64) * (K / 64) <= 4) {
    // 64 x 64 layers: 128-row stages, ~200 workgroups (adt_gemm.cuh: k_dense_dw64)
    p.dw = DW64;
    p.dw_chunk = plan_max(plan_round(plan_ceil(T, 256), DW64_ROWS), DW64_ROWS);
    p.nwg = plan_ceil(T, p.dw_chunk); p.blocks = (N / 64) * (K / 64); p.kblocks = K / 64;
    // private partials in the registered workspace + an ordered sum (no float atomics) when there is one
    const int64_t need = (int64_t)p.nwg * p.blocks * DW64_PART * 4;
    p.partials = need <= f.ws_bytes;
    p.ws_used = p.partials ? need : 0;
    p.dw_grid_x = p.nwg; p.dw_grid_y = p.blocks; p.dw_block = DW64_NTH;
    return;
  }
  p.dw = DWTILED;
  p.dw_bn = K > 64 ? 128 : 64;
  p.dw_gx = plan_ceil(K, p.dw_bn); p.dw_gy = plan_ceil(N, GBM);
  // split T so that enough workgroups are in flight while each still amortises the 16 K atomics of its flush over >= 10
  // k-steps; the targets are measured (tools/bench_dense.py at T = 51,200: 4 tiles 78 us @512 vs 98 @1024; 12 tiles 223 @2048
  // vs 247 @1024; 16 tiles 565 @1024 vs 602 @2048)
  const int tiles = p.dw_gx * p.dw_gy;
  const int target_wgs = tiles <= 4 ? 512 : (tiles <= 12 ? 2048 : 1024);
  p.dw_chunk = plan_max(plan_round(plan_ceil(T, plan_ceil(target_wgs, tiles)), GBK), GBK);
  p.dw_splits = plan_ceil(T, p.dw_chunk);
  p.dw_grid_x = xcd_grid(p.dw_splits, tiles); p.dw_grid_y = 1; p.dw_block = GTH;
  p.dw_lds_bytes = gemm_tile_lds_bytes(bf16, p.dw_bn);
}

// The two halves are independent: dX first (256-wide stage kernel, row-streaming pieces, tiled), then dW (256 x 256 partials, 256 x 128
// blocks, 64 x 64 blocks, tiled).
static inline DenseBwdPlan adt_dense_bwd_plan(const DenseFacts& f) {
  DenseBwdPlan p{};
  adt_dense_dx_plan(f, p);
  adt_dense_dw_plan(f, p);
  return p;
}

// Workspace bytes the weight gradient of a (T, K, N) layer would write (0: no workspace arm takes the shape): aligned operands, the
// row-streaming kernels enabled, any amount registered.  What adt_dense_bwd_ws_bytes of the C ABI returns.
static inline int64_t adt_dense_bwd_ws_need(int prec, int T, int K, int N) {
  if (T <= 0 || K <= 0 || N <= 0) return 0;
  DenseFacts f{};
  f.prec = prec; f.T = T; f.K = K; f.N = N; f.has_dw = true;
  f.x_ok = f.w_ok = f.g_ok = f.bias_ok = f.u_ok = f.r_ok = f.r2_ok = f.dx_ok = true;
  f.rows_on = f.stage256_on = true;
  f.ws_bytes = INT64_MAX;
  return adt_dense_bwd_plan(f).ws_used;
}

// ---- masked attention (adt_attn_gen.cuh, adt_attn_long.cuh) --------------------------------------------------------------------------
// LDS footprints; esz: 2 (bf16 images) or 4 (exact fp32).  The launchers assert them against AttnGenLds / AttnChunkLds / AttnLongLds.
constexpr size_t attn_esz(int prec) { return prec == ADT_PREC_F32 ? 4 : 2; }
constexpr size_t attn_resident_lds(int prec, int hd, int maxkt, bool bwd) {
  const size_t lp = (size_t)maxkt * 16, img = lp * (hd + 8) + hd * (lp + 8);
  return bwd ? 2 * img * attn_esz(prec) + 2 * lp * sizeof(float) + 2 * lp * sizeof(int) : img * attn_esz(prec) + 2 * lp * sizeof(int);
}
constexpr size_t attn_chunked_lds(int prec, int hd, int maxkt, int nch) {
  const size_t lp = (size_t)maxkt * 16, lpc = lp / nch;
  return 2 * (lpc * (hd + 8) + hd * (lpc + 8)) * attn_esz(prec) + 2 * lp * sizeof(float) + 2 * lp * sizeof(int);
}
// streamed (adt_attn_long.cuh), lmax rows of per-sequence state: beside the chunk images, LSE and delta of lmax rows (backward), key validity
// as lmax bytes and 32 bytes of per-wave scratch for the first attendable key
constexpr size_t attn_long_lds(int prec, int hd, int kc, bool bwd, int lmax) {
  const size_t img = (size_t)kc * (hd + 8) + (size_t)hd * (kc + 8), masks = (size_t)lmax + 32;
  return bwd ? 2 * img * attn_esz(prec) + 2 * lmax * sizeof(float) + masks : img * attn_esz(prec) + masks;
}

// bf16 operands: the forward (<= 106 VGPRs at every head size) and the backward at head size <= 64 (<= 124) fit the 128-register budget of
// 16 waves = 4 per SIMD: one query / key tile per wave at L = 200 instead of two, and twice the waves to cover each other's LDS and MFMA latency
constexpr int attn_resident_waves(int prec, int hd, bool bwd) { return prec != ADT_PREC_F32 && (!bwd || hd <= 64) ? 16 : 8; }
constexpr int ATTN_CHUNKED_NW = 8, ATTN_STREAMED_NW = 4;
constexpr int attn_streamed_kc(int prec, bool bwd) { return prec != ADT_PREC_F32 && !bwd ? 64 : 32; }      // key / query rows per streamed chunk
constexpr int ATTN_STREAMED_LMAX = 256, ATTN_LONG_LMAX = 1024;      // rows of per-sequence state: adt_attn_masked_* | adt_attn_long_*, adt_wattn_long_*

// RESIDENT: the whole (b, h) in LDS (k_attn_gen_fwd / k_attn_gen_bwd).  CHUNKED: backward staged in NCH chunks of the sequence
// (k_attn_gen_bwd_chunked).  STREAMED: key / query chunks of KC rows streamed through LDS, grid (B*H, groups of `waves` 16-row tiles).
enum AttnFamily { ATTN_RESIDENT, ATTN_CHUNKED, ATTN_STREAMED };
struct AttnPlan {
  AttnFamily family;
  int maxkt, nch, kc, waves;
  bool csk;                 // causal without key padding: the forward skips the key tiles above the diagonal
  int grid_y;
  size_t lds_bytes;
  char error[128];          // "" or the message for adt_last_error
};

// STREAMED at either lmax: waves, chunk, grid and footprint
static inline void attn_streamed_plan(AttnPlan& p, int P, int hd, int L, bool bwd, int lmax) {
  p.waves = ATTN_STREAMED_NW; p.kc = attn_streamed_kc(P, bwd);
  p.grid_y = plan_ceil(plan_ceil(L, 16), p.waves);
  p.lds_bytes = attn_long_lds(P, hd, p.kc, bwd, lmax);
}

static inline AttnPlan adt_attn_masked_plan(int prec, int hd, int L, bool bwd, bool causal, bool has_key_ids, float fill) {
  AttnPlan p{};
  const int P = prec == ADT_PREC_F32 ? ADT_PREC_F32 : ADT_PREC_BF16;
  const bool bf16 = P != ADT_PREC_F32;
  p.family = ATTN_RESIDENT; p.nch = 1; p.grid_y = 1;
  if (hd == 16 || hd == 32 || hd == 64) {
    if (L > 224) { snprintf(p.error, sizeof p.error, "masked attention: L=%d > 224 unsupported", L); return p; }
    p.maxkt = L <= 64 ? 4 : (L <= 128 ? 8 : 14);
    // exact fp32, hd = 64, L > 128: the whole-(b, h) backward images (248 KB at L = 200) do not fit the 160 KB of LDS
    if (L > 128 && !bf16 && hd == 64 && bwd) { p.family = ATTN_CHUNKED; p.maxkt = 16; p.nch = 2; }
  } else if (hd == 128) {
    // sasrec d = 256, H = 2: forward with the whole (b, h) resident, backward staged in NCH chunks
    if (L > 256) { snprintf(p.error, sizeof p.error, "masked attention: L=%d > 256 unsupported at head_dim 128", L); return p; }
    p.maxkt = L <= 64 ? 4 : 16; p.nch = L <= 64 ? 1 : 2;
    p.family = bwd ? ATTN_CHUNKED : ATTN_RESIDENT;
    // exact fp32 at L > 64: 270 KB resident forward, 272 KB two-chunk backward
    if (!bf16 && (bwd ? attn_chunked_lds(P, hd, p.maxkt, p.nch) : attn_resident_lds(P, hd, p.maxkt, false)) > ADT_LDS_MAX) p.family = ATTN_STREAMED;
  } else if (hd == 256) {
    // sasrec d = 256, H = 1
    if (L < 1 || L > 256) { snprintf(p.error, sizeof p.error, "masked attention: L=%d outside 1..256 at head_dim 256", L); return p; }
    p.family = ATTN_STREAMED;
  } else {
    snprintf(p.error, sizeof p.error, "masked attention: head_dim=%d unsupported (16/32/64/128/256)", hd);
    return p;
  }
  if (p.family == ATTN_RESIDENT) {
    p.waves = attn_resident_waves(P, hd, bwd);
    p.csk = hd == 128 && !bwd && causal && !has_key_ids && fill <= -1e9f;
    p.lds_bytes = attn_resident_lds(P, hd, p.maxkt, bwd);
    if (p.lds_bytes > ADT_LDS_MAX) snprintf(p.error, sizeof p.error, "masked attention: L=%d hd=%d prec=%d needs %zu B of LDS (> 160 KB)", L, hd, P, p.lds_bytes);
  } else if (p.family == ATTN_CHUNKED) {
    p.waves = ATTN_CHUNKED_NW;
    p.lds_bytes = attn_chunked_lds(P, hd, p.maxkt, p.nch);
    if (p.lds_bytes > ADT_LDS_MAX) snprintf(p.error, sizeof p.error, "masked attention bwd: L=%d hd=%d prec=%d needs %zu B of LDS (> 160 KB)", L, hd, P, p.lds_bytes);
  } else {
    attn_streamed_plan(p, P, hd, L, bwd, ATTN_STREAMED_LMAX);
    if (p.lds_bytes > ADT_LDS_MAX) snprintf(p.error, sizeof p.error, "masked attention: hd=%d prec=%d needs %zu B of LDS (> 160 KB)", hd, P, p.lds_bytes);
  }
  return p;
}

// The longest sequence adt_attn_masked_plan takes at a head size (0: a head size it does not take at all): the bound its branches apply,
// stated once for the callers that choose between it and adt_attn_long_plan.  The C ABI exports it under the same name (adt_attn_long.hip):
// where both are visible, qualify this one as adt::.
constexpr int adt_attn_masked_max_len(int hd) { return hd == 16 || hd == 32 || hd == 64 ? 224 : (hd == 128 || hd == 256 ? 256 : 0); }

// ---- masked attention at 1 <= L <= 1024 (adt_attn_long.cuh) --------------------------------------------------------------------------
// Always streamed, every head size, 1024 rows of per-sequence state.

static inline AttnPlan adt_attn_long_plan(int prec, int hd, int L, bool bwd, bool causal, bool has_key_ids, float fill) {
  AttnPlan p{};
  const int P = prec == ADT_PREC_F32 ? ADT_PREC_F32 : ADT_PREC_BF16;
  p.family = ATTN_STREAMED; p.nch = 1; p.grid_y = 1;
  if (hd != 16 && hd != 32 && hd != 64 && hd != 128 && hd != 256) {
    snprintf(p.error, sizeof p.error, "long attention: head_dim=%d unsupported (16/32/64/128/256)", hd);
    return p;
  }
  if (L < 1 || L > ATTN_LONG_LMAX) { snprintf(p.error, sizeof p.error, "long attention: L=%d outside 1..%d", L, ATTN_LONG_LMAX); return p; }
  attn_streamed_plan(p, P, hd, L, bwd, ATTN_LONG_LMAX);
  p.csk = causal && !has_key_ids && fill <= -1e9f;
  if (p.lds_bytes > ADT_LDS_MAX) snprintf(p.error, sizeof p.error, "long attention: hd=%d prec=%d needs %zu B of LDS (> 160 KB)", hd, P, p.lds_bytes);
  return p;
}

// ---- STOSA-ADT distance attention (adt_stosa.cuh, adt_klattn.cuh: vector ALU; adt_wattn_long.cuh: streamed, matrix cores) ---------------
// The vector-ALU kernels keep the whole (b, h) in LDS: four tensors of L rows of hd + 1 floats, 2 (forward) or 4 (backward) row vectors of
// L rounded up to 64 and four waves' scratch of 3 such vectors + 4 hd floats.  adt_stosa_args.cuh's wattn_lds_bytes, restated here for the host
// program and asserted equal in adt_wattn_long.hip.
constexpr int WATTN_VALU_LMAX = 256;            // W_KPL = 4 keys per lane
constexpr size_t wattn_valu_lds(int L, int hd, bool bwd) {
  const size_t lp = (size_t)plan_round(L, 64);
  return ((size_t)4 * L * (hd + 1) + (bwd ? 4 : 2) * lp + 4 * (3 * lp + 4 * (size_t)hd)) * sizeof(float);
}
// The longest L at which adt_wattn_* / adt_klattn_* run both directions at a head size: the smaller of 256 and what the LDS allows
// (0: a head size they do not take).  The footprint grows with L, so the first L that fits from above is the bound.  The C ABI exports it
// under the same name (adt_wattn_long.hip): where both are visible, qualify this one as adt::.
constexpr int adt_wattn_max_len(int hd) {
  if (hd != 16 && hd != 32 && hd != 64) return 0;
  int L = WATTN_VALU_LMAX;
  while (L > 0 && (wattn_valu_lds(L, hd, false) > ADT_LDS_MAX || wattn_valu_lds(L, hd, true) > ADT_LDS_MAX)) --L;
  return L;
}

// The streamed family at 1 <= L <= 1024, head size 16 / 32 / 64, both metrics: the scheme of adt_attn_long_plan (grid (B*H, groups of four
// 16-row tiles), one tile per wave) over fp32 images whatever the precision (bf16 operands are converted at the MFMA, as in
// adt_wattn_mfma.cuh), so the footprint does not depend on prec.  A chunk of kc rows holds the cross-term image (2 hd + 4 floats a row), its
// norms / biases and two transposed value images (forward), or the image, its norms, its transpose, two natural and two transposed images
// (backward) plus LSE and delta of 1024 rows; then 1024 key-validity bytes + 32.  adt_wattn_long.hip asserts it against WattnLongLds.
constexpr int wattn_long_kc(bool bwd) { return bwd ? 32 : 64; }
constexpr size_t wattn_long_lds(int hd, int kc, bool bwd) {
  const size_t cat = (size_t)kc * (2 * hd + 4) + kc, t = (size_t)hd * (kc + 4), nat = (size_t)kc * (hd + 4), masks = ATTN_LONG_LMAX + 32;
  return (bwd ? cat + 2 * t + 2 * nat + 2 * t + 2 * ATTN_LONG_LMAX : cat + 2 * t) * sizeof(float) + masks;
}

// csk: the attention is always causal, so the tiles above the diagonal are always skipped -- by the kernels' own rule, which exempts every
// tile that holds a query without an attendable key (such a row attends to all L keys; adt_wattn_long.cuh).
static inline AttnPlan adt_wattn_long_plan(int prec, int hd, int L, bool bwd) {
  AttnPlan p{};
  p.family = ATTN_STREAMED; p.nch = 1; p.grid_y = 1;
  if (prec != ADT_PREC_F32 && prec != ADT_PREC_BF16) { snprintf(p.error, sizeof p.error, "long distance attention: prec=%d unsupported", prec); return p; }
  if (hd != 16 && hd != 32 && hd != 64) { snprintf(p.error, sizeof p.error, "long distance attention: head_dim=%d unsupported (16/32/64)", hd); return p; }
  if (L < 1 || L > ATTN_LONG_LMAX) { snprintf(p.error, sizeof p.error, "long distance attention: L=%d outside 1..%d", L, ATTN_LONG_LMAX); return p; }
  p.waves = ATTN_STREAMED_NW; p.kc = wattn_long_kc(bwd);
  p.grid_y = plan_ceil(plan_ceil(L, 16), p.waves);
  p.csk = true;
  p.lds_bytes = wattn_long_lds(hd, p.kc, bwd);
  if (p.lds_bytes > ADT_LDS_MAX) snprintf(p.error, sizeof p.error, "long distance attention: hd=%d needs %zu B of LDS (> 160 KB)", hd, p.lds_bytes);
  return p;
}

// The same streamed family at head size 128 (adt_wattn_hd128.hip: entry points of their own, adt_wattn_long_plan keeps its refusals).
// The chunk is the largest of 64 / 32 rows whose footprint leaves room for two workgroups on a CU (half the LDS), else the largest that
// fits at all: 32 keys in the forward (71,328 B; 64 keys take 137,504 B and a CU to themselves), 32 rows in the backward (150,176 B, the
// only chunk of whole tile pairs that fits).  Head size 256 is refused: its backward fits the LDS only at a 16-row chunk, which the
// kernels' 32-row tile pairs do not allow, and its operand and accumulator fragments (2 x this head size's 256 registers in pass B)
// exceed the 512 registers of a lane.
constexpr int wattn_hd128_kc(bool bwd) {
  for (int kc = 64; kc >= 32; kc /= 2)
    if (wattn_long_lds(128, kc, bwd) <= ADT_LDS_MAX / 2) return kc;
  for (int kc = 64; kc >= 32; kc /= 2)
    if (wattn_long_lds(128, kc, bwd) <= ADT_LDS_MAX) return kc;
  return 0;
}

static inline AttnPlan adt_wattn_hd128_plan(int prec, int hd, int L, bool bwd) {
  AttnPlan p{};
  p.family = ATTN_STREAMED; p.nch = 1; p.grid_y = 1;
  if (prec != ADT_PREC_F32 && prec != ADT_PREC_BF16) { snprintf(p.error, sizeof p.error, "distance attention at head size 128: prec=%d unsupported", prec); return p; }
  if (hd != 128) {
    snprintf(p.error, sizeof p.error, "distance attention at head size 128: head_dim=%d unsupported (%s)", hd,
             hd == 256 ? "256 fits neither the LDS at a 32-row chunk nor 512 registers" : "16/32/64 run on the *_long entry points");
    return p;
  }
  if (L < 1 || L > ATTN_LONG_LMAX) { snprintf(p.error, sizeof p.error, "distance attention at head size 128: L=%d outside 1..%d", L, ATTN_LONG_LMAX); return p; }
  p.waves = ATTN_STREAMED_NW; p.kc = wattn_hd128_kc(bwd);
  p.grid_y = plan_ceil(plan_ceil(L, 16), p.waves);
  p.csk = true;
  p.lds_bytes = wattn_long_lds(hd, p.kc, bwd);
  return p;
}

}  // namespace adt
