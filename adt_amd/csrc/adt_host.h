// Host-side shared declarations for libadt_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/adt_hip.h"
#include "adt_common.cuh"
#include "adt_lossring_args.h"
#include "adt_wide_plan.h"      // ADT_LDS_MAX
#include "adt_step_plan.h"      // SeqSwitches, StepPlan

int adt_set_error(const char* fmt, ...);
DropCfg adt_make_drop(float p, const uint32_t* seed, uint32_t site);

// ---- launching; the out-of-line parts are defined next to adt_set_error in adt_capi.hip ----------------------------------------------
#define ADT_HIDDEN __attribute__((visibility("hidden")))      // shared by the translation units, not exported from libadt_hip.so
ADT_HIDDEN int adt_check_launch(const char* what);      // hipGetLastError() -> 0, or adt_set_error("<what>: <hip error>")

static inline int adt_grid_for(size_t work_items, int per_block, int cap) {
  size_t g = (work_items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > (size_t)cap) g = cap;
  return (int)g;
}

static inline bool adt_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

// Lanes (adt_common.cuh) of a padded layout from the ABI's (H, hd, hd_pad), checked: hd_pad a power of two in 16..256 that holds hd,
// H * hd_pad one of 64 / 128 / 192 / 256.  0, or -1 with the error set.
static inline int adt_make_lanes(Lanes& ln, int H, int hd, int hd_pad, const char* what) {
  int sh = 0;
  while ((1 << sh) < hd_pad) ++sh;
  const int dp = H * hd_pad;
  if (H < 1 || hd < 1 || hd > hd_pad || (1 << sh) != hd_pad || hd_pad < 16 || hd_pad > 256 || (dp % 64) || dp > 256)
    return adt_set_error("%s: lanes H=%d hd=%d hd_pad=%d: hd_pad a power of two in 16..256, H * hd_pad in {64,128,192,256}", what, H, hd, hd_pad);
  ln.H = H; ln.hd = hd; ln.hd_pad = hd_pad; ln.sh = sh;
  return 0;
}

// Dynamic LDS a kernel has been allowed so far (hipFuncAttributeMaxDynamicSharedMemorySize): one slot per kernel instantiation, kept as a
// function-local static (or an array of them) by its launcher.  A high-water mark, so a later launch that needs more opts in again.
struct AdtLdsOptIn { int bytes = 0; };

// Launch fn with smem bytes of dynamic LDS: error when smem > ADT_LDS_MAX, opt in when max(smem, optin) is above what slot recorded,
// hipLaunchKernel, adt_check_launch(what).  optin: a launcher whose smem varies per call passes the most it will ever ask for.
ADT_HIDDEN int adt_launch_lds(const void* fn, dim3 grid, dim3 block, size_t smem, void** kargs, hipStream_t stream, const char* what, AdtLdsOptIn& slot,
                              size_t optin = 0);
template <class Args>      // the usual case: one argument struct
static inline int adt_launch_lds1(const void* fn, dim3 grid, dim3 block, size_t smem, const Args& a, hipStream_t stream, const char* what,
                                  AdtLdsOptIn& slot, size_t optin = 0) {
  void* kargs[] = {const_cast<Args*>(&a)};
  return adt_launch_lds(fn, grid, block, smem, kargs, stream, what, slot, optin);
}

// ---- ADT_* switches --------------------------------------------------------------------------------------------------------------------
// The flagship step's (adt_sasrec.hip, adt_seq.hip) are read together, once per process, by adt_seq_switches() into the SeqSwitches of
// adt_step_plan.h; the staged and wide kernels' through `static const int on = adt_env_on("ADT_X");`, so once per process and site.
ADT_HIDDEN int adt_env_on(const char* name);                 // on unless the value parses to 0
ADT_HIDDEN int adt_env_int(const char* name, int dflt);      // atoi of the value; dflt when unset
ADT_HIDDEN const SeqSwitches& adt_seq_switches();            // defined in adt_seq.hip
ADT_HIDDEN size_t adt_seq_attn_bwd_lds(int L, int H);        // dynamic LDS of k_seq_attn_bwd (adt_seqattn.cuh: sab_lds_bytes), for StepFacts ; adt_seq.hip

// dropout sites (identical to oracle/sasrec_oracle.py)
enum { SITE_EMB_SEQ = 1, SITE_EMB_DEC = 2 };
static inline uint32_t enc_site(int layer, int which) { return 16u + 8u * (uint32_t)layer + (uint32_t)which; }   // 0 attn 1 ffn1 2 ffn2
static inline uint32_t dec_site(int layer, int which) { return 128u + 8u * (uint32_t)layer + (uint32_t)which; }  // 0 slf 1 enc 2 ffn1 3 ffn2

// fused backward chains (adt_bwdchain.cuh); defined in adt_capi.hip.  which: 0 enc_post, 1 dec_post, 2 enc_pre, 3 dec_pre, 4 dec_mid
namespace adt { struct BwdChainArgs; }
int adt_launch_bwdchain(int prec, int which, const adt::BwdChainArgs& a, void* stream);

// wave-local forward chains (adt_fwdchain.cuh); which: 0 enc_pre, 1 dec_pre, 2 enc_post, 3 dec_mid, 4 dec_post, 5 final
namespace adt { struct FwdChainArgs; }
int adt_launch_fwdchain(int prec, int which, const adt::FwdChainArgs& a, void* stream);

// per-sequence fused layer kernels (adt_seqfwd.cuh); defined in adt_seq.hip
namespace adt { struct SeqFwdArgs; }
int adt_launch_seq_enc_fwd(int hd, const adt::SeqFwdArgs& a, void* stream);
int adt_launch_seq_dec_fwd(int hd, const adt::SeqFwdArgs& a, void* stream);
// adt_pack_wimg (pre-packed bf16 weight images) is part of the C ABI now: include/adt_hip.h; defined in adt_seq.hip
#include "adt_attn_args.h"
int adt_launch_seq_attn_bwd(int hd, const adt::AttnArgs& a, void* stream);     // 0 launched, 1 shape not covered, < 0 error
// the argument block adt_attn_bwd_saved_bf16 launches with (for a caller that hands it to adt_launch_seq_xattn_mid_bwd instead)
adt::AttnArgs adt_attn_bwd_saved_bf16_args(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* O, int ldo, const float* LSE,
                                           const float* dO, int lddo, int B, int H, int L, int hd, float p, const uint32_t* seed, uint32_t site,
                                           uint32_t b_offset, float* dQ, int lddq, float* dK, int lddk, float* dV, int lddv, const uint32_t* mask,
                                           int out_bf16);
// adt_attn_bwd with Q, K, V, O saved as bf16 rows (ld* of those four count bf16 elements); per-sequence kernel only: anything it does not
// cover is an error.  Defined in adt_capi.hip.
int adt_attn_bwd_saved_bf16(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* O, int ldo, const float* LSE,
                            const float* dO, int lddo, int B, int H, int L, int hd, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset,
                            float* dQ, int lddq, float* dK, int lddk, float* dV, int lddv, const uint32_t* mask, int out_bf16, void* stream);
// The decoder's cross-attention backward and the mid chain behind it in one launch per sequence (adt_seqxattn_tt.cuh): `a` and `mid` are the
// argument blocks of adt_launch_seq_attn_bwd and adt_launch_seq_mid_bwd; dq2 / dk2 / dv2 stay in registers, a.dQ / dK / dV are not written.
// Bit-equal to the two launches.  0 launched, 1 not covered (run the two launches), < 0 error.  ADT_XATTN_FUSED=0: never covered.
int adt_seq_xattn_mid_covered(int hd, const adt::AttnArgs& a, const adt::BwdChainArgs& mid);      // 1 covered, 0 not
int adt_launch_seq_xattn_mid_bwd(int hd, const adt::AttnArgs& a, const adt::BwdChainArgs& mid, void* stream);
// per-sequence backward of the token-wise chains (adt_seqpost_tt.cuh); enc: 1 encoder post chain, 0 decoder post chain; 0 launched, 1 not covered
int adt_launch_seq_post_bwd(int hd, int enc, const adt::BwdChainArgs& a, void* stream);
int adt_launch_seq_mid_bwd(int hd, const adt::BwdChainArgs& a, void* stream);      // dec_mid + kv chains in one launch
// private per-workgroup partials of the 64 x 64 weight gradients instead of atomics (adt_seqbwd_tt.cuh: sb_dw_tiles) and their sum
int adt_dwpart_reduce(float* G, const float* part, size_t stride, int nwg, const int* slots, const int* offs, int nslots, void* stream);
// the same with a workgroup count per slot (nwg_slot[i] workgroups wrote slot i ; null: nwg everywhere)
int adt_dwpart_reduce_n(float* G, const float* part, size_t stride, int nwg, const int* nwg_slot, const int* slots, const int* offs, int nslots, void* stream);
namespace adt { struct SeqBwdArgs; }
int adt_launch_seq_attn_pre_bwd(int hd, int dec, const adt::SeqBwdArgs& a, void* stream);     // 0 launched, 1 not covered, < 0 error

// fused small kernels of the flagship backward (adt_misc.cuh; defined in adt_capi.hip): d log_feats + both item scatters in one pass,
// positional + item embedding gradient in one pass
extern "C" {
int adt_logits_bwd_scatter(const float* F, int ldf, const float* E, const int32_t* pos, const int32_t* neg, const float* dpos, const float* dneg,
                           int T, int d, float* dF, int lddf, float* rep, int nrep, int64_t rep_stride, void* stream);
// d = 64: logits, BCE seed + loss terms, d log_feats and the item rows of the positive / negative items in one pass (adt_misc.cuh)
int adt_logits_bce_scatter(const float* F, const float* E, const int32_t* pos, const int32_t* neg, const float* norms, int T, float* pos_logits,
                           float* neg_logits, float* dpos, float* dneg, float* loss_bce, float* dF, float* rep, int nrep, int64_t rep_stride, void* stream);
int adt_embed_bwd_rep(const int32_t* ids, const float* dX, int T, int L, int d, float p, const uint32_t* seed, uint32_t site, uint32_t row_offset,
                      float* dP, float* rep, int nrep, int64_t rep_stride, void* stream);
int adt_layernorm_bwd_rep(const float* dY, int lddy, const float* X, int ldx, const float* gamma, float eps, int T, int d, float* dX, int lddx,
                          int accumulate, float* dgamma, float* dbeta, int nrep, int64_t rep_stride, void* stream);
// Z / nz: a second range to zero (or null) ; pack_*: npack 64 x 64 blocks at pack_base + pack_offs[i] packed into pack_img (adt_pack_wimg's work) or null
int adt_step_begin_launch(uint32_t* seed, uint32_t inc, float* norms_dst, const float* norms_src, float* loss, int nloss, float* scal, float* G,
                          int64_t n, const float* E, int64_t nE, float* Z, int64_t nz, const float* pack_base, void* pack_img, const int* pack_offs,
                          int npack, void* stream);
int adt_step_begin_ring_launch(uint32_t* seed, uint32_t inc, float* norms_dst, float* loss, int nloss, float* scal, float* G, int64_t n, const float* E,
                               int64_t nE, const int32_t* ring, int64_t slot_ints, int nslots, int32_t* ids_dst, int64_t n_ints, uint32_t* state,
                               uint32_t* consumed, const int32_t* staging, const uint32_t* produced, float* Z, int64_t nz, const float* pack_base,
                               void* pack_img, const int* pack_offs, int npack, void* stream);
int adt_logits_bce_scatter_ex(const float* F, const float* E, const int32_t* pos, const int32_t* neg, const float* norms, int T, float* pos_logits,
                              float* neg_logits, float* dpos, float* dneg, float* loss_bce, float* dF, float* rep, int nrep, int64_t rep_stride,
                              int neg_only, void* stream);
int adt_loss_seeds(const float* pos_logits, const float* neg_logits, const int32_t* pos, int T, const float* norms, float* dpos, float* dneg,
                   float* loss_bce, int nmse, const float* const* A, const float* const* Bm, int64_t n, const float* lambdas, float* const* GA,
                   int accumulate_a, float* const* GB, float* const* loss_mse, int nnll, const float* const* rec, int n_rows, int H, float lambda2,
                   float* const* drec, float* const* loss_nll, void* stream);
int adt_fold_clip_adam(float* P, float* G, float* M, float* V, int64_t n, float* d0, const float* r0, int64_t n0, int nrep0, int64_t s0, float* d1,
                       const float* r1, int64_t n1, int nrep1, int64_t s1, float wd, float clip, float lr, float b1, float b2, float eps, float* scal,
                       void* stream);
int adt_replica_reduce2(float* d0, const float* r0, int64_t n0, int nrep0, int64_t s0, float* d1, const float* r1, int64_t n1, int nrep1, int64_t s1,
                        void* stream);
int adt_fold_parts_clip_adam(float* P, float* G, float* M, float* V, int64_t n, float* d0, const float* r0, int64_t n0, int nrep0, int64_t s0, float* d1,
                             const float* r1, int64_t n1, int nrep1, int64_t s1, const float* part, int64_t part_stride, const int* nwg_slot, const int* slots,
                             const int* offs, int nslots, const float* vpart, const int* vsrc, const int* vnwg, const int* vstride, const int* voff, int nvec,
                             float* gn_part, float wd, float clip, float lr, float b1, float b2, float eps, float* scal, void* stream);
// its fold half alone (no weight-decay term, no optimizer step)
int adt_fold_parts(float* P, float* G, int64_t n, float* d0, const float* r0, int64_t n0, int nrep0, int64_t s0, float* d1, const float* r1, int64_t n1,
                   int nrep1, int64_t s1, const float* part, int64_t part_stride, const int* nwg_slot, const int* slots, const int* offs, int nslots,
                   const float* vpart, const int* vsrc, const int* vnwg, const int* vstride, const int* voff, int nvec, float* gn_part, float* scal,
                   void* stream);
int adt_layernorm_bwd_parts(const float* dY, int lddy, const float* X, int ldx, const float* gamma, float eps, int T, int d, float* dX, int lddx,
                            int accumulate, float* part, int max_blocks, void* stream);
}

// One loss-assembly launch (adt_misc.cuh: k_loss_seeds) with everything that can ride on it.  nmse, nnll <= 4; pos_logits == nullptr: no BCE
// block (the seed is formed by the logits pass).  logits: that pass as the first workgroups of this launch.  ring (its part / nparts are set
// here): the next step's id batch is copied into ring->staging by extra workgroups -- with `split` only its first half, the second half and the
// staged mark being left to adt_embed_bwd3_prefetch of the same step, later in the stream.
struct AdtLossSeedsJob {
  const float* pos_logits; const float* neg_logits; const int32_t* pos; int T; const float* norms; float* dpos; float* dneg; float* loss_bce;
  int nmse; const float* const* A; const float* const* Bm; int64_t n; const float* lambdas; float* const* GA; int accumulate_a; float* const* GB;
  float* const* loss_mse;
  int nnll; const float* const* rec; int n_rows; int H; float lambda2; float* const* drec; float* const* loss_nll;
  const adt::LogitsBceArgs* logits; const adt::RingPrefetchArgs* ring; bool split;
};
extern "C" {
ADT_HIDDEN int adt_loss_seeds_prefetch(const AdtLossSeedsJob& job, void* stream);
// adt_embed_bwd3 (include/adt_hip.h) with the second half of a split ring prefetch as extra workgroups of its launch ; pf == nullptr: adt_embed_bwd3
ADT_HIDDEN int adt_embed_bwd3_prefetch(const int32_t* seq, const int32_t* dec, const int32_t* pos, const float* dXs, const float* dXd, const float* F,
                                       const float* dpos, int T, int L, float p, const uint32_t* seed, uint32_t site_seq, uint32_t site_dec,
                                       uint32_t row_offset, float* dP, float* rep, int nrep, int64_t rep_stride, const adt::RingPrefetchArgs* pf,
                                       void* stream);
}
