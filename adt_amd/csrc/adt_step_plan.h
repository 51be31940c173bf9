// Which kernels one flagship SASRec-ADT step launches (adt_sasrec.hip) and which shapes the per-sequence launchers cover (adt_seq.hip), decided
// once from the ADT_* switches and a handful of ints.  Plain C++: no HIP, no library state, no environment -- adt_seq_switches() (adt_seq.hip)
// fills SeqSwitches -- so the rules are tested by a host program (tests/test_step_plan_cpu.py).
#pragma once
#include <stddef.h>
#include <stdio.h>
#include "../../include/adt_hip.h"
#include "adt_bwd_plan.h"
#include "adt_wide_plan.h"      // ADT_LDS_MAX

constexpr int ADT_SEQ_MAXLEN = 224;      // rows of the per-sequence kernels' LDS images (adt_seq.hip asserts it against SQ_LP and SB_R)

// ---- the switches, as the environment gives them (an on / off switch is on unless its value parses to 0) ------------------------------------
struct SeqSwitches {
  bool seq = true;             // ADT_SEQ            the per-sequence fused layer kernels (off: the staged stage kernels)
  bool seq_lean = true;        // ADT_SEQ_LEAN       bf16 saved tensors, no LN(x) / qkv saved
  bool seq_tt = true;          // ADT_SEQ_TT         register-resident transposed chains in the forward (off: the row-major fused form)
  bool seq_bwd = true;         // ADT_SEQ_BWD        fused attention-block backward (k_seqtt_attn_pre_bwd)
  bool seq_attn_bwd = true;    // ADT_SEQ_ATTN_BWD   per-sequence attention backward (k_seq_attn_bwd)
  bool seq_post_bwd = true;    // ADT_SEQ_POST_BWD   per-sequence post / mid chain backward (k_seqtt_post_bwd, k_seqtt_mid_bwd)
  bool seq_partials = true;    // ADT_SEQ_PARTIALS   64 x 64 weight gradients as private per-workgroup partials + one ordered sum
  bool xattn_fused = true;     // ADT_XATTN_FUSED    cross-attention backward + mid chain in one launch (k_seqtt_xattn_mid_bwd)
  int seq_ablate = 0;          // ADT_SEQ_ABLATE     timing experiments: bit 0 drops the forward's saved tensors
  bool seq_ablate_set = false; //                    ... set at all, to 0 included: the lean path is off
  int seq_split = 0;           // ADT_SEQ_SPLIT      workgroups per sequence, forced (0: by batch size)
  bool attn_split = true;      // ADT_ATTN_SPLIT     two workgroups per sequence in k_seqtt_attn_pre_bwd at small batches
  int side_stream = 7;         // ADT_SIDE_STREAM    bit 0 the logits' item rows, 1 the decoder's embedding gradient + partial sums, 2 the encoder's partial sums
  bool side_stream_dp = false; // ADT_SIDE_STREAM_DP the side stream in the two-phase (data-parallel) backward too
  bool item_sort = false;      // ADT_ITEM_SORT      table gradients as sorted segmented sums (bit-reproducible) instead of float-atomic scatters
  bool lnl_fused = true;       // ADT_LNL_FUSED      last LayerNorm reversed inside the last encoder block's first backward kernel
  bool fold_parts = true;      // ADT_FOLD_PARTS     the optimizer's first kernel sums the partials (single-GPU step, <= 2 layers)
  bool fwd_fused = true;       // ADT_FWD_FUSED      log_feats from the last encoder kernel, logits + BCE deferred to the backward's first side kernel
  bool embed3 = true;          // ADT_EMBED3         both embedding gradients and the positive-logit rows in one scatter (deferred path)
  bool bce_merged = true;      // ADT_BCE_MERGED     the forward's logits / BCE kernel rides on the loss launch (off: on the side stream)
  // hand-overs between the backward's kernels (on by default)
  bool do_bf16{true};          // ADT_DO_BF16        dO from an out-projection reverse to the attention backward behind it as bf16 operand rows + delta
  bool pad_elide{true};        // ADT_PAD_ELIDE      the chain kernels request no row of a 16-token tile inside a sequence's pad prefix whose value is known or dead
};

constexpr bool adt_seq_head_ok(int hd) { return hd == 16 || hd == 32 || hd == 64; }

// ---- what a launcher of adt_seq.hip covers: pure functions of its argument block's shape --------------------------------------------------
struct SeqAttnFacts {      // of an AttnArgs
  int L, H, B;
  bool causal, in_bf16, out_bf16;
  int ldq, ldk, ldv, ldo, lddo;
  bool dropout, keep_bits;      // drop.thr != 0 ; the forward's saved keep bits are there (mask != nullptr)
  size_t sab_lds, xm_lds;       // dynamic LDS of k_seq_attn_bwd / k_seqtt_xattn_mid_bwd at (L, H): sab_lds_bytes, xm_lds_bytes of the device headers
};
struct SeqChainFacts {     // of a BwdChainArgs or SeqBwdArgs
  int L, H, B, T;
  bool wimg;                    // pre-packed weight images (wp_img != nullptr)
  bool saved_bf16, grad_bf16, parts4;      // parts4: all four weight-gradient partial areas of the mid chain
  int nsplit, ablate;
  bool drec;                    // the encoder post chain reverses the head classifier too
};

// k_seq_attn_bwd (adt_launch_seq_attn_bwd)
static inline bool adt_covers_attn_bwd(const SeqSwitches& sw, int hd, const SeqAttnFacts& a) {
  if (!sw.seq_attn_bwd || !a.causal || a.H * hd != 64 || a.L > ADT_SEQ_MAXLEN) return false;
  if ((a.ldq % 4) || (a.ldk % 4) || (a.ldv % 4) || (a.ldo % 4)) return false;
  if (a.in_bf16 && ((a.ldq % 8) || (a.ldk % 8) || (a.ldv % 8) || (a.ldo % 8))) return false;
  return a.sab_lds <= ADT_LDS_MAX && adt_seq_head_ok(hd);
}
// k_seqtt_attn_pre_bwd (adt_launch_seq_attn_pre_bwd)
static inline bool adt_covers_attn_pre_bwd(const SeqSwitches& sw, int hd, const SeqChainFacts& a) {
  return sw.seq_bwd && a.wimg && a.L <= ADT_SEQ_MAXLEN && (a.L & 3) == 0 && a.H * hd == 64 && adt_seq_head_ok(hd);
}
// k_seqtt_mid_bwd (adt_launch_seq_mid_bwd), and k_seqtt_post_bwd (adt_launch_seq_post_bwd) but for the classifier
static inline bool adt_covers_mid_bwd(const SeqSwitches& sw, int hd, const SeqChainFacts& a) {
  return sw.seq_post_bwd && a.wimg && a.L <= ADT_SEQ_MAXLEN && a.T == a.B * a.L && adt_seq_head_ok(hd);
}
static inline bool adt_covers_post_bwd(const SeqSwitches& sw, int hd, bool enc, const SeqChainFacts& a) {
  return adt_covers_mid_bwd(sw, hd, a) && !(enc && a.drec && a.H * hd != 64);
}
// k_seqtt_xattn_mid_bwd (adt_launch_seq_xattn_mid_bwd): the lean bf16 path with private partials, one workgroup per sequence, saved keep bits (or
// no dropout).  handover: what the attention would write is what the mid chain would read (bf16 rows: dq2 of 64, dk2 | dv2 of 128 elements).
static inline bool adt_covers_xattn_mid(const SeqSwitches& sw, int hd, const SeqAttnFacts& at, const SeqChainFacts& ch, bool handover) {
  if (!sw.xattn_fused || !adt_covers_mid_bwd(sw, hd, ch)) return false;
  if (!at.in_bf16 || !at.out_bf16 || !ch.saved_bf16 || !ch.grad_bf16 || !ch.parts4) return false;
  if (ch.nsplit > 1 || ch.ablate) return false;
  if (!at.causal || at.H * hd != 64 || (at.L & 3) || at.L > ADT_SEQ_MAXLEN || at.L != ch.L || at.B != ch.B) return false;
  if (at.dropout && !at.keep_bits) return false;
  if ((at.ldq % 8) || (at.ldk % 8) || (at.ldv % 8) || (at.ldo % 8) || (at.lddo % 4)) return false;
  return handover && at.xm_lds <= ADT_LDS_MAX;
}
// the forward's transposed chains (k_seqtt_enc_fwd / k_seqtt_dec_fwd) against the row-major fused form; L % 4 == 0: a quad of attention keys
// shares one dropout hash word
static inline bool adt_seq_fwd_tt(const SeqSwitches& sw, bool wimg, int L) { return sw.seq_tt && wimg && (L & 3) == 0; }

// ---- one step ------------------------------------------------------------------------------------------------------------------------------
struct StepFacts {
  int prec, L, d, H, num_layers, B;      // adt_sasrec_cfg: prec, maxlen, hidden, num_heads, num_layers ; sequences in the batch
  int rows;                              // item_num + 1
  bool item_sort_ok;                     // adt_item_sort_supported(rows)
  size_t sab_lds;                        // dynamic LDS of k_seq_attn_bwd at (L, H): adt_seq_attn_bwd_lds (adt_seq.hip), the device header's sab_lds_bytes
};

struct StepPlan {
  char cfg_error[96];      // why the executor refuses the configuration ("" : it does not) ; the fields below are filled either way
  bool use_seq;            // the per-sequence kernels cover the shape
  bool lean;               // a training forward saves bf16 tensors and no LN(x) / qkv: the backward's kernels must all be the per-sequence ones
  bool parts;              // weight gradients through private per-workgroup partials + one ordered sum instead of float atomics
  bool fold_parts;         // adt_sasrec_fold_* sums those partials, if the backward defers its fold to it
  bool parts_area, sort_area;      // the workspace holds the partials ; the scratch of the sorted table gradients
  bool det;                // item / positional table gradients by sorted segmented sums (no replicas, no float atomics)
  bool embed3_on;          // one scatter for both embedding gradients and the positive-logit rows, behind a forward with virtual seeds
  bool lnl_fused;          // the last LayerNorm is reversed inside the last encoder block's first kernel
  bool bce_deferred;       // adt_sasrec_forward_loss* leaves logits + BCE seed to the backward (adt_sasrec_bce_deferred)
  bool bce_merged;         // its logits kernel rides on the loss launch
  int seq_split;           // workgroups per sequence of the per-sequence kernels
  int attn_split;          // ... of k_seqtt_attn_pre_bwd (1 or 2)
  int side_sites;          // ADT_SIDE_STREAM bits
  bool side_dp;            // side stream in the two-phase backward
  bool loss_one_launch;    // every loss term in one k_loss_seeds launch
  bool pad_elide;          // the per-sequence chain kernels get the pad prefix of every sequence (adt_seq_args.h: pad_pre) and leave the rows it covers in HBM
  bool do_handover;        // the out-projection reverses hand dO to the attention backward behind them as bf16 rows + delta (adt_tt.cuh: tt_head_delta)
};

static inline StepPlan adt_step_plan(const StepFacts& f, const SeqSwitches& sw) {
  StepPlan p{};
  const int nl = f.num_layers;
  const int hd = (f.H >= 1 && f.d % f.H == 0) ? f.d / f.H : 0;
  if (f.d != 64) snprintf(p.cfg_error, sizeof p.cfg_error, "sasrec: hidden=%d unsupported in this build (64)", f.d);
  else if (hd == 0) snprintf(p.cfg_error, sizeof p.cfg_error, "sasrec: bad num_heads");
  else if (!adt_seq_head_ok(hd)) snprintf(p.cfg_error, sizeof p.cfg_error, "sasrec: head_dim=%d unsupported (16/32/64)", hd);
  else if (f.L > ADT_SEQ_MAXLEN) snprintf(p.cfg_error, sizeof p.cfg_error, "sasrec: maxlen=%d > %d unsupported", f.L, ADT_SEQ_MAXLEN);
  else if (nl < 1 || nl > 16) snprintf(p.cfg_error, sizeof p.cfg_error, "sasrec: num_layers");

  const bool bf16 = f.prec == ADT_PREC_BF16;
  p.use_seq = sw.seq && bf16 && f.d == 64 && f.L <= ADT_SEQ_MAXLEN && adt_seq_head_ok(hd);
  // every kernel of the backward that reads the lean tensors is a per-sequence one: k_seq_attn_bwd and k_seqtt_attn_pre_bwd cover the shape
  p.lean = sw.seq_lean && sw.seq_tt && sw.seq_bwd && sw.seq_attn_bwd && !sw.seq_ablate_set && p.use_seq && (f.L & 3) == 0 &&
           f.sab_lds <= ADT_LDS_MAX;
  // ... and the post / mid chains too: all five per-sequence backward kernels
  p.parts = sw.seq_partials && sw.seq_post_bwd && p.lean;
  p.fold_parts = sw.fold_parts && nl <= 2 && p.parts;
  p.parts_area = bf16 && f.d == 64;
  p.sort_area = f.d == 64 && f.item_sort_ok;
  p.det = sw.item_sort && p.sort_area;
  p.embed3_on = sw.embed3 && !p.det && f.d == 64;
  p.lnl_fused = p.parts && sw.lnl_fused;
  p.bce_deferred = sw.fwd_fused && f.d == 64 && nl <= 4 && p.lean;
  p.bce_merged = sw.bce_merged;
  // the largest power of two that keeps B * S within the CUs (1 at B >= 129): small batches -- a data-parallel rank's share of a global
  // batch -- otherwise leave most CUs without a workgroup
  p.seq_split = 1;
  if (sw.seq_split > 0) p.seq_split = sw.seq_split;
  else while (p.seq_split < 8 && f.B * p.seq_split * 2 <= 256) p.seq_split *= 2;
  p.attn_split = sw.attn_split && p.seq_split >= 2 ? 2 : 1;
  p.side_sites = sw.side_stream & 7;
  p.side_dp = sw.side_stream_dp;
  p.loss_one_launch = nl <= 4;
  // every producer (k_seqtt_post_bwd, k_seqtt_mid_bwd / k_seqtt_xattn_mid_bwd) and every consumer (k_seqtt_attn_pre_bwd, k_seq_attn_bwd /
  // k_seqtt_xattn_mid_bwd) is a per-sequence kernel exactly where `parts` holds: the lean path, whose "not covered" is an error and never a staged fallback
  p.do_handover = sw.do_bf16 && p.parts;
  // the prefixes are written by the encoder's embedding layer (k_seqtt_enc_fwd) and read by per-sequence kernels only: the lean path with partials again.
  // Not with 16-wide heads: those instantiations sit at their register budgets and spill already, and every form of the prefix code tried
  // added scratch to one of them ("Pad prefix")
  p.pad_elide = sw.pad_elide && p.parts && hd != 16;
  return p;
}

// ---- one adt_sasrec_backward* call of that step ----------------------------------------------------------------------------------------------
struct BwdCallPlan {
  bool late_parts;      // adt_sasrec_fold_* sums the partials, and the bias / LayerNorm / classifier sums the chain kernels then STORE per workgroup
  bool embed3;          // encoder / decoder embedding gradients and the positive-logit rows share ONE scatter at the end (adt_embed_bwd3)
  bool side;            // scatter / fold kernels on the side stream.  (One-phase backward by default: the two-phase form belongs to the
                        // data-parallel step, whose capture already carries the collectives' stream; there the side stream measured 0.692
                        // against 0.699 ms on a 1-rank RCCL group and is opt-in: ADT_SIDE_STREAM_DP=1)
};
static inline BwdCallPlan adt_bwd_call_plan(const StepPlan& s, const BwdPlan& b) {
  BwdCallPlan p;
  p.late_parts = b.defer_fold && s.fold_parts;
  p.embed3 = b.seeds_virtual && s.embed3_on;
  p.side = s.side_sites != 0 && (b.phase == 0 || s.side_dp);
  return p;
}
