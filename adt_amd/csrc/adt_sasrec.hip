// Model-level executor for SASRec-ADT: the sequence of stage launches that replaces SASRecADT.forward /
// predict (sasrec/model.py:32-97), Encoder/EncoderLayer/Decoder/DecoderLayer (sasrec/modules.py:635-757) and
// their autograd reverse pass, plus the loss seeds of sasrec/main.py:151-169.  Pure host code: it only
// enqueues kernels (via the per-stage C ABI) on the caller's stream -- and, in the one-phase backward, a few scatter / fold
// kernels on a side stream of its own that forks from and joins the caller's stream inside the call (side_stream below).
#include "adt_host.h"
#include <string.h>
#include <mutex>
#include "adt_bwdchain_args.h"
#include "adt_fwdchain_args.h"
#include "adt_seq_args.h"
#include "adt_seqbwd_args.h"

namespace {

constexpr float LN_EPS = 1e-8f;
constexpr int NREPP = 16;          // replicas of the layer-parameter gradients the backward chains flush into (one per XCD)
constexpr int LN_PART_BLOCKS = 1024;     // blocks of the last LayerNorm's backward when it stores per-block sums (adt_layernorm_bwd_parts); 256 blocks ran 22.8 us against 14.5
constexpr int NREP = 16;          // replicas of the item-table gradient (contention relief for popular items)   // sasrec/modules.py:638,640,660 ; sasrec/model.py:28

struct Layout {
  int64_t off[4 + 30 * 16];
  int64_t total;
  int nl;
  int64_t item() const { return off[0]; }
  int64_t posw() const { return off[1]; }
  int64_t lnl_w() const { return off[2]; }
  int64_t lnl_b() const { return off[3]; }
  int64_t enc(int i, int k) const { return off[4 + 14 * i + k]; }
  int64_t dec(int i, int k) const { return off[4 + 14 * nl + 16 * i + k]; }
};
enum { E_LN1W, E_LN1B, E_INW, E_INB, E_OW, E_OB, E_LN2W, E_LN2B, E_C1W, E_C1B, E_C2W, E_C2B, E_SW, E_SB };
enum { D_LNW, D_LNB, D_SINW, D_SINB, D_SOW, D_SOB, D_EINW, D_EINB, D_EOW, D_EOB, D_C1W, D_C1B, D_C2W, D_C2B, D_UW, D_UB };

int64_t up64(int64_t x) { return (x + 63) / 64 * 64; }

// what a step with this configuration and B sequences launches (adt_step_plan.h)
StepPlan step_plan(const adt_sasrec_cfg* c, int B) {
  const StepFacts f{c->prec, c->maxlen, c->hidden, c->num_heads, c->num_layers, B, c->item_num + 1, adt_item_sort_supported(c->item_num + 1) != 0,
                    c->num_heads > 0 ? adt_seq_attn_bwd_lds(c->maxlen, c->num_heads) : 0};
  return adt_step_plan(f, adt_seq_switches());
}

bool make_layout(const adt_sasrec_cfg* c, Layout* lo) {
  if (c->num_layers < 1 || c->num_layers > 16) return false;
  const int64_t d = c->hidden, H = c->num_heads, hd = d / H, L = c->maxlen, V = c->item_num;
  lo->nl = c->num_layers;
  int64_t o = 0;
  int n = 0;
  auto put = [&](int64_t sz) { lo->off[n++] = o; o += up64(sz); };
  put((V + 1) * d); put(L * d); put(d); put(d);
  for (int i = 0; i < c->num_layers; ++i) {
    put(d); put(d); put(3 * d * d); put(3 * d); put(d * d); put(d); put(d); put(d);
    put(d * d); put(d); put(d * d); put(d); put(H * hd); put(H);
  }
  for (int i = 0; i < c->num_layers; ++i) {
    put(d); put(d);
    put(3 * d * d); put(3 * d); put(d * d); put(d);
    put(3 * d * d); put(3 * d); put(d * d); put(d);
    put(d * d); put(d); put(d * d); put(d); put(d); put(d);
  }
  lo->total = o;
  return true;
}

// workspace carve-up (offsets in floats)
struct WS {
  int64_t T, d, H, L, nl, B;
  int64_t enc_x, dec_x, f, posl, negl;                                  // (nl+1)*Td each for enc_x/dec_x
  int64_t e_qn, e_qkv, e_o, e_lse, e_h, e_h2, e_u, e_rec, e_mask, e_stride;     // per encoder layer
  int64_t d_dn, d_qkv, d_o1, d_lse1, d_a1, d_q2, d_kv2, d_o2, d_lse2, d_a2, d_u, d_mask1, d_mask2, d_stride;
  int64_t g_enc_x, g_dec_x, g_f, g_pos, g_neg, g_rec;                   // gradients
  int64_t s1, s2, s3, s4, s5;                                           // backward scratch: Td, Td, 3Td, 2Td, Td
  int64_t loss, norms, scal;
  int64_t rep, rep_stride;                                              // item-table gradient replicas
  int64_t prep, prep_stride;                                            // replicas of every other parameter gradient
  int64_t wpack;                                                        // pre-packed bf16 weight images (3 floats per parameter float)
  int64_t part, part_stride;                                            // per-sequence partials of the 64 x 64 weight gradients (bf16 mode, d = 64)
  int64_t isort, isort_n;                                               // scratch of the sorted item-table gradient (adt_item_sort), isort_n int32 (0: not used)
  int64_t dodelta;                                                      // delta[T][4] of the dO hand-over (StepPlan::do_handover; adt_tt.cuh: tt_head_delta)
  int64_t padpre;                                                       // int32 pad prefix of every sequence: B of the encoder ids, B of the decoder ids (StepPlan::pad_elide)
  int64_t vpart, vcall, lnpart, gnpart;                                 // per-workgroup bias / LayerNorm / classifier gradient sums: 5 * nl calls x vcall floats ;
                                                                        // the last LayerNorm's per-block sums ; per-block partials of ||g||^2
  int64_t total;
};

void make_ws(const adt_sasrec_cfg* c, int B, const StepPlan& pl, WS* w) {
  w->B = B; w->d = c->hidden; w->H = c->num_heads; w->L = c->maxlen; w->nl = c->num_layers;
  w->T = (int64_t)B * w->L;
  const int64_t Td = up64(w->T * w->d), T1 = up64(w->T), lse = up64((int64_t)B * w->H * w->L);
  const int64_t rec = up64(w->T * w->H * w->H);
  int64_t o = 0;
  auto take = [&](int64_t n) { int64_t r = o; o += n; return r; };
  w->enc_x = take((w->nl + 1) * Td); w->dec_x = take((w->nl + 1) * Td); w->f = take(Td);
  w->posl = take(T1); w->negl = take(T1);
  {
    const int64_t s = o;
    w->e_qn = take(Td); w->e_qkv = take(3 * Td); w->e_o = take(Td); w->e_lse = take(lse); w->e_h = take(Td);
    w->e_h2 = take(Td); w->e_u = take(Td); w->e_rec = take(rec); w->e_mask = take(8 * lse);
    w->e_stride = o - s;
    o = s + w->e_stride * w->nl;
  }
  {
    const int64_t s = o;
    w->d_dn = take(Td); w->d_qkv = take(3 * Td); w->d_o1 = take(Td); w->d_lse1 = take(lse); w->d_a1 = take(Td);
    w->d_q2 = take(Td); w->d_kv2 = take(2 * Td); w->d_o2 = take(Td); w->d_lse2 = take(lse); w->d_a2 = take(Td);
    w->d_u = take(Td); w->d_mask1 = take(8 * lse); w->d_mask2 = take(8 * lse);
    w->d_stride = o - s;
    o = s + w->d_stride * w->nl;
  }
  w->g_enc_x = take((w->nl + 1) * Td); w->g_dec_x = take((w->nl + 1) * Td); w->g_f = take(Td);
  w->g_pos = take(T1); w->g_neg = take(T1); w->g_rec = take(rec * w->nl);
  w->s1 = take(Td); w->s2 = take(Td); w->s3 = take(3 * Td); w->s4 = take(2 * Td); w->s5 = take(Td);
  w->loss = take(64 * (2 + 2 * 16)); w->norms = take(64); w->scal = take(192);
  w->rep_stride = up64((int64_t)(c->item_num + 1) * w->d);
  w->rep = take(NREP * w->rep_stride);
  {
    Layout lo;
    make_layout(c, &lo);
    w->prep_stride = up64(lo.total - lo.posw());
    w->prep = take(NREPP * w->prep_stride);
    w->wpack = take(3 * w->prep_stride);
  }
  w->part_stride = pl.parts_area ? (int64_t)w->nl * 16 * 4096 : 0;
  w->part = take((int64_t)B * pl.seq_split * w->part_stride);      // one partial area per WORKGROUP (several per sequence at small batches)
  w->isort_n = pl.sort_area ? adt_item_sort_work_ints(4, (int)w->T, c->item_num + 1) : 0;
  w->isort = take(up64(w->isort_n));
  w->vcall = (int64_t)B * pl.seq_split * 512;
  w->vpart = take(w->part_stride > 0 ? (5 * w->nl + 1) * w->vcall : 0);      // (+ 1: the last LayerNorm's sums from the first encoder kernel of the backward)
  w->lnpart = take(LN_PART_BLOCKS * 128);
  w->gnpart = take(4096);
  w->dodelta = take(pl.do_handover ? up64(w->T * 4) : 0);
  w->padpre = take(pl.pad_elide ? up64(2 * (int64_t)B) : 0);
  w->total = o;
}

#define CK(call) do { int _r = (call); if (_r) return _r; } while (0)

// Side stream of the backward pass.  The chain kernels are one workgroup per CU and serial by data dependence; the scatter / fold kernels
// beside them (item-table gradient of the logits, decoder input embedding gradient, the ordered sums of the weight-gradient partials) depend
// on little and are bound by memory-side atomics or HBM, so they run on a second stream under the chain kernels: fork = an event recorded on
// the caller's stream that the side stream waits for, join = the reverse.  Inside a stream capture both become edges of the graph.  The
// stream and its events are created on the first call that is not being captured (creating them is not a capturable operation); until then,
// and with ADT_SIDE_STREAM=0, everything stays on the caller's stream.
struct SideStream {
  hipStream_t s = nullptr;
  hipEvent_t fork_ev[4] = {nullptr, nullptr, nullptr, nullptr}, join_ev[4] = {nullptr, nullptr, nullptr, nullptr};      // [3]: the id sort
};
// StepPlan::side_sites (ADT_SIDE_STREAM): bit 0 the logits' item rows, bit 1 the decoder's embedding gradient + partial sums, bit 2 the
// encoder's partial sums (default 7, 0 = everything on the caller's stream)
SideStream* side_stream(const StepPlan& pl, hipStream_t main) {
  static SideStream g[16];
  static std::mutex mu;                          // first use from two host threads at once (one trainer per thread)
  if (!pl.side_sites) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  SideStream* sd = &g[dev];
  std::lock_guard<std::mutex> lock(mu);
  if (sd->s) return sd;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(main, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return nullptr; }
  hipStream_t s = nullptr;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  for (int i = 0; i < 4; ++i)
    if (hipEventCreateWithFlags(&sd->fork_ev[i], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&sd->join_ev[i], hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipStreamDestroy(s);
      return nullptr;
    }
  sd->s = s;
  return sd;
}
// fork in two halves: side_mark records the point of the caller's stream the side work depends on, side_enter makes the side stream wait
// for it and returns the stream to enqueue the side work on (the caller's stream when there is no side stream).  The caller enqueues its
// OWN next kernel between the two: in a captured graph the branch whose node is created first stays on the queue of the parent node, and
// a chain kernel that hops queues pays the cross-queue signal (5-11 us, profiles/r03_side_stream_timeline.txt).
int side_mark(SideStream* sd, int k, void* main) {
  if (!sd) return 0;
  if (hipEventRecord(sd->fork_ev[k], (hipStream_t)main) != hipSuccess) return adt_set_error("backward: side-stream fork %d failed", k);
  return 0;
}
int side_enter(SideStream* sd, int k, void* main, void** out) {
  *out = main;
  if (!sd) return 0;
  if (hipStreamWaitEvent(sd->s, sd->fork_ev[k], 0) != hipSuccess) return adt_set_error("backward: side-stream fork %d failed", k);
  *out = sd->s;
  return 0;
}
int side_join(SideStream* sd, int k, void* main) {
  if (!sd) return 0;
  if (hipEventRecord(sd->join_ev[k], sd->s) != hipSuccess || hipStreamWaitEvent((hipStream_t)main, sd->join_ev[k], 0) != hipSuccess)
    return adt_set_error("backward: side-stream join %d failed", k);
  return 0;
}

// what every entry point starts with: the configuration checked, the step's plan, the parameter layout and the workspace carve-up for B sequences
int layout_ws(const adt_sasrec_cfg* c, int B, Layout* lo, WS* w, StepPlan* pl) {
  *pl = step_plan(c, B);
  if (pl->cfg_error[0]) return adt_set_error("%s", pl->cfg_error);
  make_layout(c, lo);
  make_ws(c, B, *pl, w);
  return 0;
}

adt::FwdChainArgs fwd_args(int T, int L, int B, int H, const int32_t* ids, float p, const uint32_t* seed, uint32_t row_offset) {
  adt::FwdChainArgs a;
  memset(&a, 0, sizeof(a));
  a.T = T; a.L = L; a.B = B; a.H = H; a.ids = ids; a.drop = adt_make_drop(p, seed, 0); a.row_offset = row_offset; a.ln_eps = LN_EPS;
  return a;
}

adt::BwdChainArgs bwd_args(int T, int L, int B, const int32_t* ids, float p, const uint32_t* seed, uint32_t row_offset) {
  adt::BwdChainArgs a;
  memset(&a, 0, sizeof(a));
  a.T = T; a.L = L; a.B = B; a.ids = ids; a.drop = adt_make_drop(p, seed, 0); a.row_offset = row_offset; a.ln_eps = LN_EPS;
  return a;
}

// bf16 mode: both LDS images of every 64 x 64 layer weight, written once per forward (the weights do not change until the
// optimizer step that follows the backward), so that every kernel's weight staging is a plain copy
int pack_offsets(const adt_sasrec_cfg* c, const Layout& lo, int* offs) {      // float offsets from lo.posw() of the 64 x 64 blocks ; 0 blocks outside bf16 mode
  if (c->prec != ADT_PREC_BF16) return 0;
  int n = 0;
  const int64_t base = lo.posw();
  const int dd = c->hidden * c->hidden;
  for (int i = 0; i < c->num_layers; ++i) {
    for (int j = 0; j < 3; ++j) offs[n++] = (int)(lo.enc(i, E_INW) + j * dd - base);
    offs[n++] = (int)(lo.enc(i, E_OW) - base); offs[n++] = (int)(lo.enc(i, E_C1W) - base); offs[n++] = (int)(lo.enc(i, E_C2W) - base);
    for (int j = 0; j < 3; ++j) offs[n++] = (int)(lo.dec(i, D_SINW) + j * dd - base);
    for (int j = 0; j < 3; ++j) offs[n++] = (int)(lo.dec(i, D_EINW) + j * dd - base);
    offs[n++] = (int)(lo.dec(i, D_SOW) - base); offs[n++] = (int)(lo.dec(i, D_EOW) - base);
    offs[n++] = (int)(lo.dec(i, D_C1W) - base); offs[n++] = (int)(lo.dec(i, D_C2W) - base);
  }
  return n;
}
int pack_weights(const adt_sasrec_cfg* c, const Layout& lo, const WS& w, const float* P, float* ws, void* st) {
  int offs[256];
  const int n = pack_offsets(c, lo, offs);
  if (n == 0) return 0;
  return adt_pack_wimg(P + lo.posw(), ws + w.wpack, offs, n, st);
}

// slot of a 64 x 64 block in a workgroup's partial area: the order of pack_weights
enum { PS_E_IN = 0, PS_E_O = 3, PS_E_C1 = 4, PS_E_C2 = 5, PS_D_SIN = 6, PS_D_EIN = 9, PS_D_SO = 12, PS_D_EO = 13, PS_D_C1 = 14, PS_D_C2 = 15 };

// the partial slots of the encoder (enc = true) and / or decoder (dec = true) blocks of every layer and their offsets in G
int partial_slots(const adt_sasrec_cfg* c, const Layout& lo, bool enc, bool dec, int* slots, int* offs);
// workgroups that wrote partial `slot` of a step with B sequences: the token-chain kernels run StepPlan::seq_split workgroups per sequence,
// k_seqtt_attn_pre_bwd one, two at small batches (StepPlan::attn_split)
int partial_nwg(const StepPlan& pl, int slot, int B) {
  const int k = slot % 16;
  const bool attn_block = (k >= PS_E_IN && k < PS_E_IN + 3) || (k >= PS_D_SIN && k < PS_D_SIN + 3);
  return attn_block ? B * pl.attn_split : B * pl.seq_split;
}
// sums the partials of the encoder (enc = true) and / or decoder (dec = true) blocks of every layer into G
int reduce_partials(const adt_sasrec_cfg* c, const Layout& lo, const WS& w, const StepPlan& pl, float* G, float* ws, bool enc, bool dec, void* st) {
  int slots[256], offs[256];
  const int n = partial_slots(c, lo, enc, dec, slots, offs);
  int nwg[256];
  for (int i = 0; i < n; ++i) nwg[i] = partial_nwg(pl, slots[i], (int)w.B);
  return adt_dwpart_reduce_n(G, ws + w.part, (size_t)w.part_stride, (int)w.B, nwg, slots, offs, n, st);
}
int partial_slots(const adt_sasrec_cfg* c, const Layout& lo, bool enc, bool dec, int* slots, int* offs) {
  int n = 0;
  const int dd = c->hidden * c->hidden;
  for (int i = 0; i < c->num_layers; ++i) {
    if (enc) {
      for (int j = 0; j < 3; ++j) { slots[n] = 16 * i + PS_E_IN + j; offs[n++] = (int)(lo.enc(i, E_INW) + j * dd); }
      slots[n] = 16 * i + PS_E_O; offs[n++] = (int)lo.enc(i, E_OW);
      slots[n] = 16 * i + PS_E_C1; offs[n++] = (int)lo.enc(i, E_C1W);
      slots[n] = 16 * i + PS_E_C2; offs[n++] = (int)lo.enc(i, E_C2W);
    }
    if (dec) {
      for (int j = 0; j < 3; ++j) { slots[n] = 16 * i + PS_D_SIN + j; offs[n++] = (int)(lo.dec(i, D_SINW) + j * dd); }
      for (int j = 0; j < 3; ++j) { slots[n] = 16 * i + PS_D_EIN + j; offs[n++] = (int)(lo.dec(i, D_EINW) + j * dd); }
      slots[n] = 16 * i + PS_D_SO; offs[n++] = (int)lo.dec(i, D_SOW);
      slots[n] = 16 * i + PS_D_EO; offs[n++] = (int)lo.dec(i, D_EOW);
      slots[n] = 16 * i + PS_D_C1; offs[n++] = (int)lo.dec(i, D_C1W);
      slots[n] = 16 * i + PS_D_C2; offs[n++] = (int)lo.dec(i, D_C2W);
    }
  }
  return n;
}

adt::SeqBwdArgs seq_bwd_args(int L, int B, int H, const int32_t* ids, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, int hd) {
  adt::SeqBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.L = L; a.B = B; a.H = H; a.ids = ids; a.drop = adt_make_drop(p, seed, site); a.b_offset = b_offset; a.ln_eps = LN_EPS;
  a.scale = 1.0f / sqrtf((float)hd);
  return a;
}

adt::SeqFwdArgs seq_args(int nsplit, int L, int B, int H, const int32_t* ids, float p, const uint32_t* seed, uint32_t b_offset, int hd) {
  adt::SeqFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.nsplit = nsplit;
  a.L = L; a.B = B; a.H = H; a.ids = ids; a.drop = adt_make_drop(p, seed, 0); a.b_offset = b_offset; a.ln_eps = LN_EPS;
  a.scale = 1.0f / sqrtf((float)hd);
  return a;
}

// argument block of one encoder layer's fused forward (adt_seqfwd_tt.cuh / adt_seqfwd.cuh)
adt::SeqFwdArgs enc_layer_seq_args(const adt_sasrec_cfg* c, const Layout& lo, const WS& w, const StepPlan& pl, const float* P, float* ws, const int32_t* seq,
                                   float p, const uint32_t* seed, uint32_t b_offset, int i, bool training_outputs, bool lean, const int32_t* dec = nullptr) {
  const int d = (int)w.d, H = (int)w.H, hd = d / H, L = (int)w.L, B = (int)w.B, prec = c->prec;
  const int64_t Td = up64(w.T * w.d);
  float* x = ws + w.enc_x + i * Td;
  float* y = ws + w.enc_x + (i + 1) * Td;
  float* base = ws + i * w.e_stride;
  adt::SeqFwdArgs a = seq_args(pl.seq_split, L, B, H, seq, p, seed, b_offset, hd);
  a.x = i == 0 ? nullptr : x; a.E = P + lo.item(); a.P = P + lo.posw(); a.emb_scale = sqrtf((float)d); a.site_emb = SITE_EMB_SEQ;
  a.site_attn = enc_site(i, 0); a.site1 = enc_site(i, 1); a.site2 = enc_site(i, 2);
  a.gamma = P + lo.enc(i, E_LN1W); a.beta = P + lo.enc(i, E_LN1B); a.Win = P + lo.enc(i, E_INW); a.bin = P + lo.enc(i, E_INB);
  a.Wo = P + lo.enc(i, E_OW); a.bo = P + lo.enc(i, E_OB); a.gamma2 = P + lo.enc(i, E_LN2W); a.beta2 = P + lo.enc(i, E_LN2B);
  a.W1 = P + lo.enc(i, E_C1W); a.b1 = P + lo.enc(i, E_C1B); a.W2 = P + lo.enc(i, E_C2W); a.b2 = P + lo.enc(i, E_C2B);
  a.x_out = x; a.xn = base + w.e_qn; a.qkv = base + w.e_qkv; a.o = base + w.e_o; a.lse = base + w.e_lse;
  a.mask = reinterpret_cast<uint32_t*>(base + w.e_mask); a.h = base + w.e_h; a.u = base + w.e_u; a.y = y;
  if (training_outputs && H > 1) { a.rec = base + w.e_rec; a.Ws = P + lo.enc(i, E_SW); a.bs = P + lo.enc(i, E_SB); }
  a.wp_base = P + lo.posw(); a.wp_img = prec == ADT_PREC_BF16 ? (const void*)(ws + w.wpack) : nullptr;
  if (lean) { a.xn = nullptr; a.qkv = nullptr; a.saved_bf16 = 1; }
  // the encoder's layer 0, the step's first kernel, writes the prefixes of both stacks (it is given the decoder's ids for that) ; every per-sequence kernel
  // of the step behind it reads its stack's
  if (lean && pl.pad_elide && dec) { a.pad_pre = reinterpret_cast<int*>(ws + w.padpre); a.pad_ids2 = dec; }
  return a;
}

// encoder stack forward (gathers the input embedding inside the first chain) + last LayerNorm (+ logits and the
// cross-attention k/v projections of every decoder layer when training_outputs)
int encoder_forward(const adt_sasrec_cfg* c, const Layout& lo, const WS& w, const StepPlan& pl, const float* P, float* ws,
                    const int32_t* seq, const int32_t* pos, const int32_t* neg, float p, const uint32_t* seed,
                    uint32_t b_offset, bool training_outputs, void* st, bool packed = false, const int32_t* dec = nullptr) {
  const int T = (int)w.T, d = (int)w.d, H = (int)w.H, hd = d / H, L = (int)w.L, B = (int)w.B, prec = c->prec, nl = c->num_layers;
  const int64_t Td = up64(w.T * w.d);
  const uint32_t ro = b_offset * (uint32_t)L;
  const int dd = d * d;
  const bool use_seq = pl.use_seq;
  const bool lean = training_outputs && pl.lean;   // bf16 saved tensors, no LN(x) / qkv (the fused backward recomputes them)
  if (!packed) CK(pack_weights(c, lo, w, P, ws, st));      // packed: adt_sasrec_step_begin* of this step wrote the images
  const float* wp_base = P + lo.posw();
  const void* wp_img = prec == ADT_PREC_BF16 ? (const void*)(ws + w.wpack) : nullptr;
  for (int i = 0; i < nl; ++i) {
    float* x = ws + w.enc_x + i * Td;
    float* y = ws + w.enc_x + (i + 1) * Td;
    float* base = ws + i * w.e_stride;
    float *qn = base + w.e_qn, *qkv = base + w.e_qkv, *o = base + w.e_o, *lse = base + w.e_lse, *h = base + w.e_h,
          *u = base + w.e_u, *rec = base + w.e_rec;
    const float* inw = P + lo.enc(i, E_INW);
    const float* inb = P + lo.enc(i, E_INB);
    if (use_seq) {   // the whole layer in one launch, one workgroup per sequence (adt_seqfwd.cuh)
      const adt::SeqFwdArgs a = enc_layer_seq_args(c, lo, w, pl, P, ws, seq, p, seed, b_offset, i, training_outputs, lean, dec);
      CK(adt_launch_seq_enc_fwd(hd, a, st));
      continue;
    }
    {  // [gather] ; Q = LN1(x) ; q = Q Wq^T + bq ; k, v = x Wk^T, x Wv^T     (sasrec/model.py:34-41, modules.py:646-647)
      adt::FwdChainArgs a = fwd_args(T, L, B, H, seq, p, seed, ro);
      a.x = i == 0 ? nullptr : x; a.E = P + lo.item(); a.P = P + lo.posw(); a.emb_scale = sqrtf((float)d); a.site0 = SITE_EMB_SEQ;
      a.gamma = P + lo.enc(i, E_LN1W); a.beta = P + lo.enc(i, E_LN1B);
      for (int j = 0; j < 3; ++j) { a.W[j] = inw + j * dd; a.b[j] = inb + j * d; }
      a.o0 = x; a.ld0 = d; a.o1 = qn; a.ld1 = d; a.o2 = qkv; a.ld2 = 3 * d;
      CK(adt_launch_fwdchain(prec, 0, a, st));
    }
    CK(adt_attn_fwd(prec, qkv, 3 * d, qkv + d, 3 * d, qkv + 2 * d, 3 * d, B, H, L, hd, 1, p, seed, enc_site(i, 0), b_offset, o, d,
                    lse, reinterpret_cast<uint32_t*>(base + w.e_mask), st));
    {  // h = Q + out_proj(o); h2 = LN2(h); u = relu(drop1(conv1 h2)); y = (h2 + drop2(conv2 u)) * mask   (:648-654)
      adt::FwdChainArgs a = fwd_args(T, L, B, H, seq, p, seed, ro);
      a.x = o; a.r0 = qn; a.site1 = enc_site(i, 1); a.site2 = enc_site(i, 2);
      a.W[0] = P + lo.enc(i, E_OW); a.b[0] = P + lo.enc(i, E_OB);
      a.W[1] = P + lo.enc(i, E_C1W); a.b[1] = P + lo.enc(i, E_C1B);
      a.W[2] = P + lo.enc(i, E_C2W); a.b[2] = P + lo.enc(i, E_C2B);
      a.gamma = P + lo.enc(i, E_LN2W); a.beta = P + lo.enc(i, E_LN2B);
      a.o0 = h; a.ld0 = d; a.o1 = u; a.ld1 = d; a.o2 = y; a.ld2 = d;
      int which = 2;
      if (training_outputs) {
        a.rec = rec; a.Ws = P + lo.enc(i, E_SW); a.bs = P + lo.enc(i, E_SB);
        which = H <= 2 ? 6 : (H <= 4 ? 7 : 8);     // classifier width specialisations
      }
      CK(adt_launch_fwdchain(prec, which, a, st));
    }
  }
  // log_feats = last_layernorm(encoder out); pos/neg logits; [k2, v2] of every decoder layer   (model.py:48, :72-76)
  for (int j0 = 0; j0 == 0 || (training_outputs && !use_seq && j0 < nl); j0 += 2) {
    adt::FwdChainArgs a = fwd_args(T, L, B, H, seq, 0.f, nullptr, ro);
    a.x = ws + w.enc_x + nl * Td; a.gamma = P + lo.lnl_w(); a.beta = P + lo.lnl_b();
    if (j0 == 0) { a.o0 = ws + w.f; a.ld0 = d; }
    if (training_outputs) {
      if (j0 == 0) { a.E = P + lo.item(); a.pos = pos; a.neg = neg; a.pos_logits = ws + w.posl; a.neg_logits = ws + w.negl; }
      a.nkv = use_seq ? 0 : (nl - j0 >= 2 ? 2 : 1);       // the fused decoder layer projects its own cross keys / values
      for (int k = 0; k < a.nkv; ++k) {
        const float* einw = P + lo.dec(j0 + k, D_EINW);
        const float* einb = P + lo.dec(j0 + k, D_EINB);
        a.W[2 * k] = einw + dd; a.W[2 * k + 1] = einw + 2 * dd; a.b[2 * k] = einb + d; a.b[2 * k + 1] = einb + 2 * d;
        float* kv2 = ws + (j0 + k) * w.d_stride + w.d_kv2;
        if (k == 0) { a.o2 = kv2; a.ld2 = 2 * d; } else { a.o3 = kv2; a.ld3 = 2 * d; }
      }
    }
    CK(adt_launch_fwdchain(prec, 5, a, st));
  }
  return 0;
}

// one decoder layer, fused forward: one launch, one workgroup per sequence (adt_seqfwd_tt.cuh / adt_seqfwd.cuh)
adt::SeqFwdArgs dec_layer_seq_args(const Layout& lo, const WS& w, const StepPlan& pl, const float* P, float* ws, const int32_t* dec, float p,
                                   const uint32_t* seed, uint32_t b_offset, int i) {
  const int d = (int)w.d, H = (int)w.H, hd = d / H, L = (int)w.L, B_ = (int)w.B;
  const int64_t Td = up64(w.T * w.d);
  float* x = ws + w.dec_x + i * Td;
  float* y = ws + w.dec_x + (i + 1) * Td;
  float* base = ws + i * w.d_stride;   // d_* offsets are absolute for layer 0
  float *dn = base + w.d_dn, *qkv = base + w.d_qkv, *o1 = base + w.d_o1, *lse1 = base + w.d_lse1, *a1 = base + w.d_a1,
        *q2 = base + w.d_q2, *kv2 = base + w.d_kv2, *o2 = base + w.d_o2, *lse2 = base + w.d_lse2, *a2 = base + w.d_a2, *u = base + w.d_u;
  adt::SeqFwdArgs a = seq_args(pl.seq_split, L, B_, H, dec, p, seed, b_offset, hd);
  a.x = i == 0 ? nullptr : x; a.E = P + lo.item(); a.P = P + lo.posw(); a.emb_scale = sqrtf((float)d); a.site_emb = SITE_EMB_DEC;
  a.site_attn = dec_site(i, 0); a.site_attn2 = dec_site(i, 1); a.site1 = dec_site(i, 2); a.site2 = dec_site(i, 3);
  a.gamma = P + lo.dec(i, D_LNW); a.beta = P + lo.dec(i, D_LNB); a.Win = P + lo.dec(i, D_SINW); a.bin = P + lo.dec(i, D_SINB);
  a.Wo = P + lo.dec(i, D_SOW); a.bo = P + lo.dec(i, D_SOB); a.f = ws + w.f; a.Win2 = P + lo.dec(i, D_EINW); a.bin2 = P + lo.dec(i, D_EINB);
  a.Wo2 = P + lo.dec(i, D_EOW); a.bo2 = P + lo.dec(i, D_EOB);
  a.W1 = P + lo.dec(i, D_C1W); a.b1 = P + lo.dec(i, D_C1B); a.W2 = P + lo.dec(i, D_C2W); a.b2 = P + lo.dec(i, D_C2B);
  a.x_out = x; a.xn = dn; a.qkv = qkv; a.o = o1; a.lse = lse1; a.mask = reinterpret_cast<uint32_t*>(base + w.d_mask1);
  a.a1 = a1; a.q2 = q2; a.kv2 = kv2; a.o2 = o2; a.lse2 = lse2; a.mask2 = reinterpret_cast<uint32_t*>(base + w.d_mask2);
  a.h = a2; a.u = u; a.y = y;
  a.wp_base = P + lo.posw(); a.wp_img = ws + w.wpack;
  if (pl.lean) { a.xn = nullptr; a.qkv = nullptr; a.saved_bf16 = 1; }
  if (pl.pad_elide) a.pad_pre = reinterpret_cast<int*>(ws + w.padpre) + B_;      // the decoder ids' prefixes behind the encoder ids' (pad_elide implies lean)
  return a;
}
int dec_layer_seq_fwd(const Layout& lo, const WS& w, const StepPlan& pl, const float* P, float* ws, const int32_t* dec, float p,
                      const uint32_t* seed, uint32_t b_offset, int i, void* st) {
  const adt::SeqFwdArgs a = dec_layer_seq_args(lo, w, pl, P, ws, dec, p, seed, b_offset, i);
  return adt_launch_seq_dec_fwd((int)(w.d / w.H), a, st);
}

// Training forward + loss assembly of the lean per-sequence path (StepPlan::bce_deferred): log_feats is the tail of the last encoder layer's
// kernel (no k_final_fwd launch) and the pos / neg logits + BCE seed are formed by the backward's first side kernel, which gathers E[pos], E[neg]
// and log_feats anyway (adt_logits_bce_scatter; adt_sasrec_backward with phase bit 4): forward_loss_lean below.
// the stream the forward's logits kernel runs on when it is not merged into the loss launch (nullptr: the caller's), and whose join_ev[0] the backward waits for
SideStream* fwd_logits_stream(const StepPlan& pl, void* st) { return ((pl.side_sites & 1) && !pl.bce_merged) ? side_stream(pl, (hipStream_t)st) : nullptr; }
// same step, same ring arguments: the forward's loss launch copies the first half of the next batch's ring slot exactly when the backward's
// embedding scatter copies the second (and then marks the batch staged) -- 819 KB over PCIe do not fit behind either launch alone
bool ring_prefetch_split(const adt::RingPrefetchArgs& rr, bool bce_by_forward, const StepPlan& pl) {
  return rr.ring && rr.staging && rr.state && bce_by_forward && pl.embed3_on;
}

// Pointer arrays of the loss launch (AdtLossSeedsJob) and its reconstruction / independence terms: pair i = (enc_in[i], dec_out_rev[i] = DEC_X[nl - i])
// (sasrec/main.py:155-158), independence term i = encoder layer i with the stale loop index lambdas2[nl - 1] (sasrec/main.py:169).
// all_seeds = false: only the reconstruction seed the backward's FIRST kernels read as a plain input (d / d decoder output) is written.  The others
// were written to be added to the input gradient of a block that re-reads that very input: k_seqtt_attn_pre_bwd forms them from its own x
// rows and the other stack's rows (SeqBwdArgs::seed_other) -- 39 MB of stores here and as many loads there less per step.
struct LossPtrs { const float *A[4], *Bm[4], *rc[4]; float *GA[4], *GB[4], *lm[4], *dr[4], *ln[4]; };
AdtLossSeedsJob loss_terms(const WS& w, float* ws, const float* lambdas1, const float* lambdas2, bool all_seeds, LossPtrs* q) {
  const int nl = (int)w.nl, H = (int)w.H;
  const int64_t Td = up64(w.T * w.d), rec = up64(w.T * w.H * w.H);
  float* loss = ws + w.loss;
  for (int i = 0; i < nl; ++i) {
    q->A[i] = ws + w.enc_x + i * Td; q->Bm[i] = ws + w.dec_x + (nl - i) * Td;
    q->GA[i] = all_seeds ? ws + w.g_enc_x + i * Td : nullptr;
    q->GB[i] = (all_seeds || i == 0) ? ws + w.g_dec_x + (nl - i) * Td : nullptr;      // (i >= 1: not even read -- the encoder block's backward adds the loss term)
    q->lm[i] = loss + 64 * (2 + i);
    q->rc[i] = ws + i * w.e_stride + w.e_rec; q->dr[i] = ws + w.g_rec + i * rec; q->ln[i] = loss + 64 * (2 + nl + i);
  }
  AdtLossSeedsJob j{};
  j.T = (int)w.T; j.norms = ws + w.norms; j.loss_bce = loss;
  j.nmse = nl; j.A = q->A; j.Bm = q->Bm; j.n = w.T * w.d; j.lambdas = lambdas1; j.GA = q->GA; j.GB = q->GB; j.loss_mse = q->lm;
  j.nnll = H > 1 ? nl : 0; j.rec = q->rc; j.n_rows = (int)w.T; j.H = H; j.lambda2 = lambdas2[nl - 1]; j.drec = q->dr; j.loss_nll = q->ln;
  return j;
}

// Returns 1 when the shape is not covered (nothing launched).
// bce_side (ADT_TRAIN_BCE_SIDE of adt_sasrec_forward_loss*): the logits + BCE + item-row scatter kernel of the deferred path is launched HERE, as the
// first workgroups of the loss launch or (ADT_BCE_MERGED=0) on the library's side stream beside it (both are memory passes; under the backward's
// first chain kernels it stretched the latency-bound cross-attention backward by about its own duration), and joined by
// adt_sasrec_backward(ADT_PHASE_BCE_FWD) in front of the first kernel that reads d log_feats.  The item-table replicas are zero:
// adt_sasrec_step_begin* of this step.
int forward_loss_lean(const adt_sasrec_cfg* c, const Layout& lo, const WS& w, const StepPlan& pl, const float* P, float* ws, const int32_t* seq, const int32_t* dec,
                      const int32_t* pos, const int32_t* neg, bool bce_side, float p, const uint32_t* seed, uint32_t b_offset, const float* lambdas1,
                      const float* lambdas2, const adt::RingPrefetchArgs& rr, void* st) {
  const int hd = (int)(w.d / w.H), nl = c->num_layers;
  if (!pl.bce_deferred) return 1;
  if (pl.pad_elide && !dec) return adt_set_error("forward: the pad prefixes need the decoder's ids");
  for (int i = 0; i < nl; ++i) {
    adt::SeqFwdArgs a = enc_layer_seq_args(c, lo, w, pl, P, ws, seq, p, seed, b_offset, i, true, true, dec);
    if (i == nl - 1) { a.lnl_gamma = P + lo.lnl_w(); a.lnl_beta = P + lo.lnl_b(); a.f_out = ws + w.f; }
    CK(adt_launch_seq_enc_fwd(hd, a, st));
  }
  for (int j = 0; j < nl; ++j) CK(dec_layer_seq_fwd(lo, w, pl, P, ws, dec, p, seed, b_offset, j, st));
  // reconstruction + independence seeds in one launch (no BCE block: no logits yet)
  LossPtrs q;
  AdtLossSeedsJob job = loss_terms(w, ws, lambdas1, lambdas2, false, &q);
  // (+ the next step's id batch, if its producer has published it: the PCIe read runs under this streaming pass)
  job.ring = &rr; job.split = ring_prefetch_split(rr, bce_side, pl);
  const adt::LogitsBceArgs lb{ws + w.f, P + lo.item(), pos, neg, ws + w.norms, (int)w.T, ws + w.posl, ws + w.negl, ws + w.g_pos, ws + w.g_neg, ws + w.loss,
                              ws + w.g_f, pl.det ? nullptr : ws + w.rep, NREP, (size_t)w.rep_stride, pl.embed3_on ? 1 : 0};
  const bool merged = bce_side && pl.bce_merged;
  if (merged) job.logits = &lb;      // ... as the first workgroups of the loss launch itself: no second stream, no fork / join
  SideStream* const sd = (bce_side && !merged) ? fwd_logits_stream(pl, st) : nullptr;
  if (bce_side && !merged) CK(side_mark(sd, 0, st));
  CK(adt_loss_seeds_prefetch(job, st));
  if (bce_side && !merged) {
    void* s2 = nullptr;
    CK(side_enter(sd, 0, st, &s2));
    CK(adt_logits_bce_scatter_ex(lb.F, lb.E, pos, neg, lb.norms, lb.T, lb.pos_logits, lb.neg_logits, lb.dpos, lb.dneg, lb.loss, lb.dF, lb.rep, lb.nrep,
                                 w.rep_stride, lb.neg_only, s2));
    if (sd && hipEventRecord(sd->join_ev[0], sd->s) != hipSuccess) return adt_set_error("forward_loss: logits event");
  }
  return 0;
}

// ---- the reverse pass ----------------------------------------------------------------------------------------------------------------
// Measurement hook (bench.py's roofline probe; not part of include/adt_hip.h): HIP events recorded on the launch stream right before and right
// after ONE launch inside adt_sasrec_backward -- which = 1: the fused attention-block backward (k_seqtt_attn_pre_bwd) of encoder layer `layer`;
// which = 2: the same kernel's decoder instantiation for decoder layer `layer`; 3: see time_mark; 0 switches the hook off.
int g_time_which = 0, g_time_layer = 0;
hipEvent_t g_time_ev0 = nullptr, g_time_ev1 = nullptr;
// which = 3: calibration -- BOTH events in front of the launch of which = 1 (nothing between them): what an event pair itself adds to an interval
inline void time_mark(int which, int layer, bool start, void* st) {
  if (!g_time_ev0 || !g_time_ev1 || g_time_layer != layer) return;
  if (g_time_which == 3 && which == 1 && start) {
    (void)hipEventRecord(g_time_ev0, (hipStream_t)st);
    (void)hipEventRecord(g_time_ev1, (hipStream_t)st);
  } else if (g_time_which == which) {
    (void)hipEventRecord(start ? g_time_ev0 : g_time_ev1, (hipStream_t)st);
  }
}

// Defensive: StepPlan::parts implies adt_covers_post_bwd / adt_covers_mid_bwd for the argument blocks built here (ADT_SEQ_POST_BWD, bf16 weight
// images, L <= ADT_SEQ_MAXLEN, T = B L, a head size of 16 / 32 / 64, H hd = 64): tests/test_step_plan_cpu.py asserts it over the whole table.
const char* const NO_FALLBACK = "backward: shape L=%d hd=%d left the per-sequence kernels although the partial-gradient path was chosen";

// What one adt_sasrec_backward* call works on: built once (bwd_init), read by the functions of the blocks below.
struct Bwd {
  const adt_sasrec_cfg* c; Layout lo; WS w;
  const float* P; float* G; float* ws;
  const int32_t *seq, *dec, *pos, *neg;
  float p; const uint32_t* seed; uint32_t b_offset, ro;      // ro: b_offset in token rows
  void* st;                      // the caller's stream
  BwdPlan plan;                  // the phase word of this call
  StepPlan sp;                   // what the step launches: the forward of this step read the same plan
  BwdCallPlan call;              // ... and this call of it
  adt::RingPrefetchArgs ring;      // the step's id ring as adt_sasrec_forward_loss_prefetch got it (ring == nullptr: none)
  int T, d, H, hd, L, prec, nl;
  int64_t Td, recsz;
  // the backward chains flush their weight / bias / LayerNorm gradients into NREPP zeroed replicas of the non-item parameters
  // (Gq + lo.xxx() addresses replica 0); each phase folds its range into G at its end
  float* Gq;
  float *s1, *s3, *s4, *s5, *gf;      // scratch ; d log_feats
  // StepPlan::do_handover: every out-projection reverse hands dO to the attention backward behind it as bf16 rows of dO * drop.scale + delta
  // (adt_bwdchain_args.h: do_bf16).  The cross-attention's dO2 rows live in the first half of s1; the self-attention blocks' rows in s3, which
  // only the staged kernels use (never on this path): the launch that reads dO2 writes dO1, and the two do not share a buffer.  One delta area
  // serves both: a sequence's dO2 delta is consumed by the prologue of the launch whose mid chain later writes its dO1 delta.
  void* do_rows() const { return sp.do_handover ? (void*)s3 : nullptr; }
  void* do_rows_cross() const { return sp.do_handover ? (void*)s1 : nullptr; }
  float* do_delta() const { return sp.do_handover ? ws + w.dodelta : nullptr; }
  float do_scale(uint32_t site) const { return adt_make_drop(p, seed, site).scale; }      // the consumer's drop.scale
  // StepPlan::pad_elide: the pad prefixes the encoder's embedding layer of this step's forward left in the workspace (adt_seq_args.h: pad_pre)
  const int* pad_pre(bool dec_stack) const { return sp.pad_elide ? reinterpret_cast<const int*>(ws + w.padpre) + (dec_stack ? w.B : 0) : nullptr; }
  const float* f;                     // log_feats
  SideStream *sd, *sd_sort;           // side stream of the scatter / fold kernels ; of the id sort (nullptr: the caller's stream)

  adt::BwdChainArgs BA(const int32_t* ids, float pp, const uint32_t* sdp) const {
    adt::BwdChainArgs a = bwd_args(T, L, (int)w.B, ids, pp, sdp, ro);
    a.nrep = NREPP; a.rep_stride = (size_t)w.prep_stride;
    a.wp_base = P + lo.posw(); a.wp_img = prec == ADT_PREC_BF16 ? (const void*)(ws + w.wpack) : nullptr;   // packed by the forward of this step
    a.nsplit = sp.seq_split;
    return a;
  }
  float* PART(int layer, int slot) const { return sp.parts ? ws + w.part + (int64_t)(16 * layer + slot) * 4096 : nullptr; }
  float* VPART(int layer, int k) const { return call.late_parts ? ws + w.vpart + (int64_t)(5 * layer + k) * w.vcall : nullptr; }
  // d log_feats + item rows of pos / neg (+ logits and BCE seed on the deferred path)   (sasrec/model.py:72-76)
  int logits_scatter(void* s) const {
    if (plan.bce_here)
      return adt_logits_bce_scatter_ex(f, P + lo.item(), pos, neg, ws + w.norms, T, ws + w.posl, ws + w.negl, ws + w.g_pos, ws + w.g_neg, ws + w.loss,
                                       gf, sp.det ? nullptr : ws + w.rep, NREP, w.rep_stride, call.embed3 ? 1 : 0, s);
    if (sp.det) return adt_logits_bwd_df(P + lo.item(), pos, neg, ws + w.g_pos, ws + w.g_neg, T, d, gf, d, s);
    return adt_logits_bwd_scatter(f, d, P + lo.item(), pos, neg, ws + w.g_pos, ws + w.g_neg, T, d, gf, d, ws + w.rep, NREP, w.rep_stride, s);
  }
  // a replica area that adt_sasrec_step_begin* did not zero for this step
  int zero_unless_prezeroed(int64_t at, size_t n, void* s) const {
    return (!plan.prep_zeroed && adt::zero_f32_async(ws + at, n, (hipStream_t)s)) ? adt_set_error("replica zero") : 0;
  }
};

int bwd_init(Bwd& x, const adt_sasrec_cfg* c, const float* P, float* G, float* ws, const int32_t* seq, const int32_t* dec, const int32_t* pos,
             const int32_t* neg, int B, int training, const uint32_t* seed, uint32_t b_offset, int phase, const adt::RingPrefetchArgs& ring, void* st) {
  CK(layout_ws(c, B, &x.lo, &x.w, &x.sp));
  if (const char* err = adt_bwd_plan(phase, x.sp.bce_deferred, &x.plan)) return adt_set_error("%s", err);
  x.call = adt_bwd_call_plan(x.sp, x.plan);
  const WS& w = x.w;
  x.c = c; x.P = P; x.G = G; x.ws = ws; x.seq = seq; x.dec = dec; x.pos = pos; x.neg = neg; x.seed = seed; x.b_offset = b_offset; x.st = st; x.ring = ring;
  x.T = (int)w.T; x.d = (int)w.d; x.H = (int)w.H; x.hd = x.d / x.H; x.L = (int)w.L; x.prec = c->prec; x.nl = c->num_layers;
  x.Td = up64(w.T * w.d); x.recsz = up64(w.T * w.H * w.H);
  x.p = training ? c->dropout : 0.f;
  x.ro = b_offset * (uint32_t)x.L;
  x.s1 = ws + w.s1; x.s3 = ws + w.s3; x.s4 = ws + w.s4; x.s5 = ws + w.s5; x.gf = ws + w.g_f; x.f = ws + w.f;
  x.Gq = ws + w.prep - x.lo.posw();
  x.sd_sort = x.sp.det ? side_stream(x.sp, (hipStream_t)st) : nullptr;      // the id sort runs beside the decoder's chain kernels, also in the two-phase form
  x.sd = x.call.side ? side_stream(x.sp, (hipStream_t)st) : nullptr;
  return 0;
}

// Where the logits kernel (Bwd::logits_scatter) goes.  Its item-table rows and d log_feats (first read by the reverse of the cross-attention
// projections) run on the side stream under the first two decoder kernels, which only need the parameter replicas zeroed.
struct LogitsSide {
  enum { DONE, MARKED, ENQUEUED, BY_FORWARD } at = DONE;      // MARKED: forked, to be enqueued behind the first chain kernel

  // in front of the decoder stack (item-table replicas and parameter replicas are adjacent in the workspace: one fill)
  int begin(const Bwd& x) {
    const WS& w = x.w;
    if (x.plan.bce_fwd) {      // nothing to launch: the forward put the kernel on the side stream (or, without one, on this stream); joined below
      at = BY_FORWARD;
    } else if (x.sp.det) {
      CK(x.zero_unless_prezeroed(w.prep, (size_t)NREPP * w.prep_stride, x.st));
      CK(x.logits_scatter(x.st));      // no atomics left in it: a short streaming pass on the caller's stream
    } else if (x.sd && (x.sp.side_sites & 1)) {
      CK(side_mark(x.sd, 0, x.st));
      CK(x.zero_unless_prezeroed(w.prep, (size_t)NREPP * w.prep_stride, x.st));
      at = MARKED;
    } else {
      CK(x.zero_unless_prezeroed(w.rep, (size_t)NREP * w.rep_stride + (size_t)NREPP * w.prep_stride, x.st));
      CK(x.logits_scatter(x.st));
    }
    return 0;
  }
  int after_first_chain_kernel(const Bwd& x) {
    if (at != MARKED) return 0;
    void* s2 = nullptr;
    CK(side_enter(x.sd, 0, x.st, &s2));
    CK(x.zero_unless_prezeroed(x.w.rep, (size_t)NREP * x.w.rep_stride, s2));
    CK(x.logits_scatter(s2));
    at = ENQUEUED;
    return 0;
  }
  // in front of the first kernel that reads d log_feats: complete from here on
  int join(const Bwd& x) {
    if (at == ENQUEUED) CK(side_join(x.sd, 0, x.st));
    if (at == BY_FORWARD) {
      SideStream* const sl = fwd_logits_stream(x.sp, x.st);
      if (sl && hipStreamWaitEvent((hipStream_t)x.st, sl->join_ev[0], 0) != hipSuccess) return adt_set_error("backward: logits join");
    }
    at = DONE;
    return 0;
  }
};

// ---- one decoder block, last kernel first ------------------------------------------------------------------------------------------
// FFN + mask + enc_attn.out_proj reverse -> dO2 (s1)
int dec_post_bwd(const Bwd& x, int i) {
  const WS& w = x.w; const Layout& lo = x.lo; const float* P = x.P; float* const Gq = x.Gq;
  float* base = x.ws + i * w.d_stride;
  adt::BwdChainArgs a = x.BA(x.dec, x.p, x.seed);
  a.site1 = dec_site(i, 2); a.site2 = dec_site(i, 3);
  a.gy = x.ws + w.g_dec_x + (i + 1) * x.Td; a.u = base + w.d_u; a.xin = base + w.d_a2; a.o = base + w.d_o2; a.saved_bf16 = x.sp.lean;
  a.W0 = P + lo.dec(i, D_C2W); a.W1 = P + lo.dec(i, D_C1W); a.W2 = P + lo.dec(i, D_EOW);
  a.dW0 = Gq + lo.dec(i, D_C2W); a.dW1 = Gq + lo.dec(i, D_C1W); a.dW2 = Gq + lo.dec(i, D_EOW);
  a.db0 = Gq + lo.dec(i, D_C2B); a.db1 = Gq + lo.dec(i, D_C1B); a.db2 = Gq + lo.dec(i, D_EOB);
  a.out0 = x.s1;
  a.do_bf16 = x.do_rows_cross(); a.do_delta = x.do_delta(); a.do_scale = x.do_scale(dec_site(i, 1)); a.do_hd = x.hd;      // -> the cross-attention backward
  a.pad_pre = x.pad_pre(true);
  a.part[0] = x.PART(i, PS_D_C2); a.part[1] = x.PART(i, PS_D_C1); a.part[2] = x.PART(i, PS_D_EO); a.part_stride = (size_t)w.part_stride;
  a.vpart = x.VPART(i, 0);
  const int rc = x.sp.use_seq ? adt_launch_seq_post_bwd(x.hd, 0, a, x.st) : 1;
  if (rc < 0) return rc;
  if (rc && x.sp.parts) return adt_set_error(NO_FALLBACK, x.L, x.hd);
  return rc ? adt_launch_bwdchain(x.prec, 1, a, x.st) : 0;
}

adt::AttnArgs dec_cross_attn_lean_args(const Bwd& x, int i);

// cross attention core: dq2 -> s5, dkv2 -> s4
int dec_cross_attn_bwd(const Bwd& x, int i) {
  const WS& w = x.w; const int d = x.d, B = (int)w.B;
  float* base = x.ws + i * w.d_stride;
  float *q2 = base + w.d_q2, *kv2 = base + w.d_kv2, *o2 = base + w.d_o2, *lse2 = base + w.d_lse2, *s4 = x.s4;
  const uint32_t* mask2 = reinterpret_cast<const uint32_t*>(base + w.d_mask2);
  if (!x.sp.lean)
    return adt_attn_bwd(x.prec, q2, d, kv2, 2 * d, kv2 + d, 2 * d, o2, d, lse2, x.s1, d, B, x.H, x.L, x.hd, 1, x.p, x.seed, dec_site(i, 1), x.b_offset,
                        x.s5, d, s4, 2 * d, s4 + d, 2 * d, mask2, x.st);
  if (x.sp.do_handover) {      // (implies lean and parts) dO2 arrives as bf16 rows + delta: the same launch from the argument block that names them
    const int rc = adt_launch_seq_attn_bwd(x.hd, dec_cross_attn_lean_args(x, i), x.st);
    return rc == 1 ? adt_set_error(NO_FALLBACK, x.L, x.hd) : rc;
  }
  const uint16_t* kvb = reinterpret_cast<const uint16_t*>(kv2);      // rows of 128 bf16: k2 | v2
  // dq2 / dk2 / dv2 go to k_seqtt_mid_bwd only (with `parts` a "not covered" from it is an error), which builds bf16 MFMA operands from
  // them: written as bf16 rows (the same rounding, half the bytes); s4 + d / 2 floats = 64 bf16 elements into the (k | v) row
  return adt_attn_bwd_saved_bf16(q2, d, kvb, 2 * d, kvb + d, 2 * d, o2, d, lse2, x.s1, d, B, x.H, x.L, x.hd, x.p, x.seed, dec_site(i, 1), x.b_offset,
                                 x.s5, d, s4, 2 * d, x.sp.parts ? s4 + d / 2 : s4 + d, 2 * d, mask2, x.sp.parts ? 1 : 0, x.st);
}

// the per-sequence mid chain's argument block (adt_seqpost_tt.cuh: both projections' reverse in one launch)
adt::BwdChainArgs dec_mid_seq_args(const Bwd& x, int i) {
  const WS& w = x.w; const Layout& lo = x.lo; const float* P = x.P; float* const Gq = x.Gq;
  const int d = x.d, dd = d * d;
  float* base = x.ws + i * w.d_stride;
  const float* einw = P + lo.dec(i, D_EINW);
  float* geinw = Gq + lo.dec(i, D_EINW);
  float* geinb = Gq + lo.dec(i, D_EINB);
  adt::BwdChainArgs a = x.BA(x.dec, 0.f, nullptr);
  a.dqkv = x.s5; a.lddqkv = d; a.xin = base + w.d_a1; a.o = base + w.d_o1; a.saved_bf16 = x.sp.lean; a.dkv2 = x.s4; a.f = x.f;
  a.grad_bf16 = (x.sp.lean && x.sp.parts) ? 1 : 0;
  a.W0 = einw; a.W1 = P + lo.dec(i, D_SOW); a.W2 = einw + dd; a.W3 = einw + 2 * dd;
  a.dW0 = geinw; a.dW1 = Gq + lo.dec(i, D_SOW); a.dW2 = geinw + dd; a.dW3 = geinw + 2 * dd;
  a.db0 = geinb; a.db1 = Gq + lo.dec(i, D_SOB); a.db2 = geinb + d; a.db3 = geinb + 2 * d;
  a.out0 = x.s1; a.out1 = x.gf; a.acc1 = 1;
  a.part[0] = x.PART(i, PS_D_EIN); a.part[1] = x.PART(i, PS_D_SO); a.part[2] = x.PART(i, PS_D_EIN + 1); a.part[3] = x.PART(i, PS_D_EIN + 2);
  a.part_stride = (size_t)w.part_stride;
  a.vpart = x.VPART(i, 1);
  a.do_bf16 = x.do_rows(); a.do_delta = x.do_delta(); a.do_scale = x.do_scale(dec_site(i, 0)); a.do_hd = x.hd;      // -> attn_block_bwd(dec)
  a.pad_pre = x.pad_pre(true);
  return a;
}

// the argument block of dec_cross_attn_bwd's launch on the lean path with partials (dq2 / dk2 / dv2 as bf16 rows)
adt::AttnArgs dec_cross_attn_lean_args(const Bwd& x, int i) {
  const WS& w = x.w; const int d = x.d;
  float* base = x.ws + i * w.d_stride;
  const uint16_t* kvb = reinterpret_cast<const uint16_t*>(base + w.d_kv2);      // rows of 128 bf16: k2 | v2
  adt::AttnArgs a = adt_attn_bwd_saved_bf16_args(base + w.d_q2, d, kvb, 2 * d, kvb + d, 2 * d, base + w.d_o2, d, base + w.d_lse2, x.s1, d, (int)w.B, x.H, x.L,
                                                 x.hd, x.p, x.seed, dec_site(i, 1), x.b_offset, x.s5, d, x.s4, 2 * d, x.s4 + d / 2, 2 * d,
                                                 reinterpret_cast<const uint32_t*>(base + w.d_mask2), 1);
  a.do_bf16 = x.do_rows_cross(); a.do_delta = x.do_delta();      // from dec_post_bwd
  a.pad_pre = x.pad_pre(true);      // the queries are the decoder's
  return a;
}

// enc_attn q / k / v projections and slf_attn.out_proj reverse -> dO1 (s1), g_f +=
int dec_mid_bwd(const Bwd& x, int i) {
  const WS& w = x.w; const Layout& lo = x.lo; const float* P = x.P; float* const Gq = x.Gq;
  const int d = x.d, dd = d * d;
  float* base = x.ws + i * w.d_stride;
  float *o1 = base + w.d_o1, *a1 = base + w.d_a1;
  const float* einw = P + lo.dec(i, D_EINW);
  float* geinw = Gq + lo.dec(i, D_EINW);
  float* geinb = Gq + lo.dec(i, D_EINB);
  if (x.sp.use_seq) {   // both projections' reverse in one launch per sequence (adt_seqpost_tt.cuh)
    const int rc = adt_launch_seq_mid_bwd(x.hd, dec_mid_seq_args(x, i), x.st);
    if (rc <= 0) return rc;
    if (x.sp.parts) return adt_set_error(NO_FALLBACK, x.L, x.hd);
  }
  {  // q2 = a1 Wq^T, a1 = o1 Wo1^T  -> dO1 (s1)
    adt::BwdChainArgs a = x.BA(x.dec, 0.f, nullptr);
    a.dqkv = x.s5; a.lddqkv = d; a.xin = a1; a.o = o1; a.saved_bf16 = x.sp.lean;
    a.W0 = einw; a.W1 = P + lo.dec(i, D_SOW);
    a.dW0 = geinw; a.dW1 = Gq + lo.dec(i, D_SOW); a.db0 = geinb; a.db1 = Gq + lo.dec(i, D_SOB);
    a.out0 = x.s1;
    CK(adt_launch_bwdchain(x.prec, 4, a, x.st));
  }
  // [k2, v2] = f Wkv^T  -> g_f +=
  adt::BwdChainArgs a = x.BA(x.dec, 0.f, nullptr);
  a.dkv2 = x.s4; a.f = x.f;
  a.W0 = einw + dd; a.W1 = einw + 2 * dd;
  a.dW0 = geinw + dd; a.dW1 = geinw + 2 * dd; a.db0 = geinb + d; a.db1 = geinb + 2 * d;
  a.out0 = x.gf; a.acc0 = 1;
  return adt_launch_bwdchain(x.prec, 5, a, x.st);
}

// (self-)attention backward + LayerNorm / in-projection backward of one block, decoder (dec) or encoder:
// gx (+)= LN'(dqkv Win + gy * mask)      |      gx += LN'(dq Wq + dh) + dk Wk + dv Wv
int attn_block_bwd(const Bwd& x, int i, bool dec) {
  const WS& w = x.w; const Layout& lo = x.lo; const float* P = x.P; float* const Gq = x.Gq; float* const ws = x.ws;
  const int d = x.d, dd = d * d, nl = x.nl;
  const int32_t* ids = dec ? x.dec : x.seq;
  float* gy = ws + (dec ? w.g_dec_x : w.g_enc_x) + (i + 1) * x.Td;      // d loss / d (output of layer i), complete (the encoder's went into dh = s5)
  float* gx = ws + (dec ? w.g_dec_x : w.g_enc_x) + i * x.Td;            // accumulates d / d (input of layer i) ; encoder: already holds the reconstruction seed
  const float* xi = ws + (dec ? w.dec_x : w.enc_x) + i * x.Td;
  float* base = ws + i * (dec ? w.d_stride : w.e_stride);
  float *qkv = base + (dec ? w.d_qkv : w.e_qkv), *o = base + (dec ? w.d_o1 : w.e_o), *lse = base + (dec ? w.d_lse1 : w.e_lse);
  const uint32_t* mask = reinterpret_cast<const uint32_t*>(base + (dec ? w.d_mask1 : w.e_mask));
  const int64_t lnw = dec ? lo.dec(i, D_LNW) : lo.enc(i, E_LN1W), lnb = dec ? lo.dec(i, D_LNB) : lo.enc(i, E_LN1B);
  const int64_t inw = dec ? lo.dec(i, D_SINW) : lo.enc(i, E_INW), inb = dec ? lo.dec(i, D_SINB) : lo.enc(i, E_INB);
  const uint32_t site = dec ? dec_site(i, 0) : enc_site(i, 0);
  const int acc = dec ? (i > 0 ? 1 : 0) : 1;
  if (x.sp.use_seq) {   // ... in one launch per sequence (adt_seqbwd_tt.cuh)
    adt::SeqBwdArgs a = seq_bwd_args(x.L, (int)w.B, x.H, ids, x.p, x.seed, site, x.b_offset, x.hd);
    a.x = xi; a.gamma = P + lnw; a.beta = P + lnb; a.Win = P + inw; a.bin = P + inb;
    a.dO = x.s1; a.o = o; a.lse = lse; a.mask = mask; a.dres = dec ? gy : x.s5;
    a.do_bf16 = x.do_rows(); a.do_delta = x.do_delta();      // from enc_post_bwd / the decoder's mid chain
    a.pad_pre = x.pad_pre(dec);
    a.gx = gx; a.acc = acc; a.dWin = Gq + inw; a.dbin = Gq + inb; a.dgamma = Gq + lnw; a.dbeta = Gq + lnb;
    if (x.plan.seeds_virtual && dec && i > 0) {      // reconstruction pair (enc_in[nl - i], dec_x[i]): d / d dec_x[i] = -2 lambda (a - b) / n = coef * (x - a)
      a.acc = 0; a.seed_other = ws + w.enc_x + (nl - i) * x.Td; a.seed_coef = ws + w.norms + 8 + (nl - i);
    }
    if (x.plan.seeds_virtual && !dec) {               // reconstruction pair (enc_in[i], dec_x[nl - i]): d / d enc_in[i] = coef * (x - b)
      a.acc = 0; a.seed_other = ws + w.dec_x + (nl - i) * x.Td; a.seed_coef = ws + w.norms + 8 + i;
      if (i > 0) { a.seed_loss = ws + w.loss + 64 * (2 + i); a.seed_norms = ws + w.norms; }      // pair i >= 1 is not touched by the loss pass at all
    }
    a.nrep = NREPP; a.rep_stride = (size_t)w.prep_stride; a.wp_base = P + lo.posw(); a.wp_img = ws + w.wpack; a.saved_bf16 = x.sp.lean;
    a.part = x.PART(i, dec ? PS_D_SIN : PS_E_IN); a.part_stride = (size_t)w.part_stride;
    a.vpart = x.VPART(i, dec ? 2 : 4);
    a.nsplit = a.part ? x.sp.attn_split : 1;
    time_mark(dec ? 2 : 1, i, true, x.st);
    const int rc = adt_launch_seq_attn_pre_bwd(x.hd, dec ? 1 : 0, a, x.st);
    time_mark(dec ? 2 : 1, i, false, x.st);
    if (rc <= 0) return rc;
    // defensive: StepPlan::lean implies adt_covers_attn_pre_bwd (ADT_SEQ_BWD, weight images, L % 4 == 0, L <= ADT_SEQ_MAXLEN, H hd = 64)
    if (x.sp.lean) return adt_set_error("backward: the lean forward needs the fused attention-block backward (L=%d hd=%d)", x.L, x.hd);
  }
  // the staged pair below is the one user of s3, and reads fp32 dO from s1: never beside the hand-over, whose dO1 rows live in s3 (Bwd::do_rows)
  if (x.sp.do_handover) return adt_set_error("backward: the staged attention backward was reached with the dO hand-over on (L=%d hd=%d)", x.L, x.hd);
  CK(adt_attn_bwd(x.prec, qkv, 3 * d, qkv + d, 3 * d, qkv + 2 * d, 3 * d, o, d, lse, x.s1, d, (int)w.B, x.H, x.L, x.hd, 1, x.p, x.seed, site, x.b_offset,
                  x.s3, 3 * d, x.s3 + d, 3 * d, x.s3 + 2 * d, 3 * d, mask, x.st));
  adt::BwdChainArgs a = x.BA(ids, 0.f, nullptr);
  a.dqkv = x.s3; a.lddqkv = 3 * d; a.xin = xi;
  if (dec) a.gy = gy; else a.dh = x.s5;
  a.W0 = P + inw; a.W1 = P + inw + dd; a.W2 = P + inw + 2 * dd; a.gamma = P + lnw; a.beta = P + lnb;
  a.dW0 = Gq + inw; a.dW1 = Gq + inw + dd; a.dW2 = Gq + inw + 2 * dd; a.db0 = Gq + inb; a.db1 = Gq + inb + d; a.db2 = Gq + inb + 2 * d;
  a.dgamma = Gq + lnw; a.dbeta = Gq + lnb;
  a.out0 = gx; a.acc0 = acc;
  return adt_launch_bwdchain(x.prec, dec ? 3 : 2, a, x.st);
}

int dec_block_backward(const Bwd& x, int i, LogitsSide& logits) {
  CK(dec_post_bwd(x, i));
  CK(logits.after_first_chain_kernel(x));
  if (x.sp.use_seq && x.sp.lean && x.sp.parts) {      // dec_cross_attn_bwd + dec_mid_bwd in one launch per sequence where covered (adt_seqxattn_tt.cuh)
    const adt::AttnArgs at = dec_cross_attn_lean_args(x, i);
    const adt::BwdChainArgs mid = dec_mid_seq_args(x, i);
    if (adt_seq_xattn_mid_covered(x.hd, at, mid)) {
      CK(logits.join(x));      // the launch adds into d log_feats: the logits side joins in front of it
      const int rc = adt_launch_seq_xattn_mid_bwd(x.hd, at, mid, x.st);
      // defensive: the launcher asks adt_seq_xattn_mid_covered of the same two argument blocks again
      if (rc) return rc < 0 ? rc : adt_set_error("backward: the fused cross-attention + mid launch refused a shape it covers (L=%d hd=%d)", x.L, x.hd);
      return attn_block_bwd(x, i, true);
    }
  }
  CK(dec_cross_attn_bwd(x, i));
  CK(logits.join(x));
  CK(dec_mid_bwd(x, i));
  return attn_block_bwd(x, i, true);
}

// The decoder's input embedding gradient (sasrec/model.py:53-59) and the sum of the decoder blocks' partials need nothing from the encoder
// chain: in a one-phase backward they run on the side stream under it (joined in front of the last fold); in the two-phase form the sum runs
// beside the embedding gradient.  k_dwpart_reduce adds with atomics and k_replica_reduce2 read-modify-writes the same range of G: the fold
// always comes behind the join.
struct DecSide {
  enum { NONE, MARKED, ENQUEUED } at = NONE;
  bool parts_done = false;      // the decoder blocks' partials were summed here (not left to the encoder's sum)

  int embed(const Bwd& x, void* s) const {
    const WS& w = x.w;
    return adt_embed_bwd_rep(x.dec, x.ws + w.g_dec_x, x.T, x.L, x.d, x.p, x.seed, SITE_EMB_DEC, x.ro, x.G + x.lo.posw(), x.ws + w.rep, NREP, w.rep_stride, s);
  }
  // behind the decoder stack (phase 0 or 1)
  int begin(const Bwd& x) {
    const WS& w = x.w; const Layout& lo = x.lo;
    const int64_t dec_begin = lo.dec(0, 0);
    // (embed3: the decoder embedding's rows go out with the encoder's at the very end -- with the sums left to the optimizer's fold there is then
    // nothing for the side stream here, and no fork)
    if (x.plan.phase == 0 && x.sd && (x.sp.side_sites & 2) && !(x.call.embed3 && (x.call.late_parts || !x.sp.parts))) {
      CK(side_mark(x.sd, 1, x.st));
      at = MARKED;                      // enqueued behind the first kernel of the encoder phase
    } else if (x.plan.phase == 0) {
      if (!x.sp.det && !x.call.embed3) CK(embed(x, x.st));
    } else if (x.sp.det) {      // two-phase form: the decoder blocks' partial sums and the fold of the decoder range (nothing of the tables yet)
      if (x.sp.parts) CK(reduce_partials(x.c, lo, w, x.sp, x.G, x.ws, false, true, x.st));
      CK(adt_replica_reduce(x.G + dec_begin, x.Gq + dec_begin, lo.total - dec_begin, NREPP, w.prep_stride, x.st));
    } else {
      void* s2 = nullptr;
      CK(side_mark(x.sd, 1, x.st));
      if (!x.call.embed3) CK(embed(x, x.st));
      CK(side_enter(x.sd, 1, x.st, &s2));
      if (x.sp.parts) CK(reduce_partials(x.c, lo, w, x.sp, x.G, x.ws, false, true, s2));
      CK(side_join(x.sd, 1, x.st));
      CK(adt_replica_reduce2(x.G + lo.item(), x.ws + w.rep, (int64_t)(x.c->item_num + 1) * x.d, NREP, w.rep_stride, x.G + dec_begin, x.Gq + dec_begin,
                             lo.total - dec_begin, NREPP, w.prep_stride, x.st));
    }
    return 0;
  }
  // behind the first kernel of the encoder phase (which keeps the caller's queue)
  int enter(const Bwd& x) {
    if (at != MARKED) return 0;
    void* s2 = nullptr;
    CK(side_enter(x.sd, 1, x.st, &s2));
    if (!x.sp.det && !x.call.embed3) CK(embed(x, s2));
    if (x.sp.parts && !x.call.late_parts) { CK(reduce_partials(x.c, x.lo, x.w, x.sp, x.G, x.ws, false, true, s2)); parts_done = true; }
    at = ENQUEUED;
    return 0;
  }
  // in front of the table gradients, unless a later join of the (in-order) side stream covers it
  int join(const Bwd& x, bool covered) {
    if (at == ENQUEUED && !covered) CK(side_join(x.sd, 1, x.st));
    at = NONE;
    return 0;
  }
};

// last_layernorm: g_enc_x[nl] = LN'(g_f), unless the last encoder block's first kernel does it (Bwd::lnl_fused)
int last_layernorm_bwd(const Bwd& x) {
  const WS& w = x.w; const Layout& lo = x.lo; float* const ws = x.ws;
  const int d = x.d;
  if (x.sp.lnl_fused) return 0;      // (nothing to launch: BwdChainArgs::lnl_x of the first encoder kernel)
  if (x.call.late_parts) {
    const int nb = adt_layernorm_bwd_parts(x.gf, d, ws + w.enc_x + x.nl * x.Td, d, x.P + lo.lnl_w(), LN_EPS, x.T, d, ws + w.g_enc_x + x.nl * x.Td, d, 0,
                                           ws + w.lnpart, LN_PART_BLOCKS, x.st);
    return nb < 0 ? nb : 0;
  }
  return adt_layernorm_bwd_rep(x.gf, d, ws + w.enc_x + x.nl * x.Td, d, x.P + lo.lnl_w(), LN_EPS, x.T, d, ws + w.g_enc_x + x.nl * x.Td, d, 0,
                               x.Gq + lo.lnl_w(), x.Gq + lo.lnl_b(), NREPP, w.prep_stride, x.st);
}

// ---- one encoder block ---------------------------------------------------------------------------------------------------------------
// FFN + mask + forward_layernorm + out_proj reverse -> dh (s5), dO (s1)  [+ the last LayerNorm in front, + the head classifier]
int enc_post_bwd(const Bwd& x, int i) {
  const WS& w = x.w; const Layout& lo = x.lo; const float* P = x.P; float* const Gq = x.Gq; float* const ws = x.ws;
  const int H = x.H, nl = x.nl;
  float* base = ws + i * w.e_stride;
  adt::BwdChainArgs a = x.BA(x.seq, x.p, x.seed);
  a.site1 = enc_site(i, 1); a.site2 = enc_site(i, 2);
  a.gy = ws + w.g_enc_x + (i + 1) * x.Td; a.u = base + w.e_u; a.xin = base + w.e_h; a.o = base + w.e_o; a.saved_bf16 = x.sp.lean;
  a.W0 = P + lo.enc(i, E_C2W); a.W1 = P + lo.enc(i, E_C1W); a.W2 = P + lo.enc(i, E_OW);
  a.gamma = P + lo.enc(i, E_LN2W); a.beta = P + lo.enc(i, E_LN2B);
  a.dW0 = Gq + lo.enc(i, E_C2W); a.dW1 = Gq + lo.enc(i, E_C1W); a.dW2 = Gq + lo.enc(i, E_OW);
  a.db0 = Gq + lo.enc(i, E_C2B); a.db1 = Gq + lo.enc(i, E_C1B); a.db2 = Gq + lo.enc(i, E_OB);
  a.dgamma = Gq + lo.enc(i, E_LN2W); a.dbeta = Gq + lo.enc(i, E_LN2B);
  a.out0 = x.s5; a.out1 = x.s1;
  int which = 0;
  if (H > 1 && H <= 4) {   // independence-head classifier reverse, fused (sasrec/modules.py:648-649; main.py:160-169)
    which = H <= 2 ? 6 : 7;
    a.rec = base + w.e_rec; a.drec = ws + w.g_rec + i * x.recsz; a.Ws = P + lo.enc(i, E_SW); a.dWs = Gq + lo.enc(i, E_SW);
    a.dbs = Gq + lo.enc(i, E_SB); a.H = H;
  }
  a.part[0] = x.PART(i, PS_E_C2); a.part[1] = x.PART(i, PS_E_C1); a.part[2] = x.PART(i, PS_E_O); a.part_stride = (size_t)w.part_stride;
  a.vpart = x.VPART(i, 3);
  a.do_bf16 = x.do_rows(); a.do_delta = x.do_delta(); a.do_scale = x.do_scale(enc_site(i, 0)); a.do_hd = x.hd;      // -> attn_block_bwd(enc)
  a.pad_pre = x.pad_pre(false);
  if (x.sp.lnl_fused && i == nl - 1) {
    a.gy = x.gf; a.lnl_x = ws + w.enc_x + nl * x.Td; a.lnl_gamma = P + lo.lnl_w(); a.lnl_eps = LN_EPS;
    a.vpart2 = x.call.late_parts ? ws + w.vpart + (int64_t)(5 * nl) * w.vcall : nullptr;
    a.lnl_dgamma = Gq + lo.lnl_w(); a.lnl_dbeta = Gq + lo.lnl_b();
  }
  const int rc = x.sp.use_seq ? adt_launch_seq_post_bwd(x.hd, 1, a, x.st) : 1;
  if (rc < 0) return rc;
  if (rc && x.sp.parts) return adt_set_error(NO_FALLBACK, x.L, x.hd);
  return rc ? adt_launch_bwdchain(x.prec, which, a, x.st) : 0;
}

int enc_block_backward(const Bwd& x, int i, DecSide& dec_side) {
  const WS& w = x.w; const Layout& lo = x.lo;
  CK(enc_post_bwd(x, i));
  if (x.sp.lnl_fused && i == x.nl - 1) CK(dec_side.enter(x));      // the first kernel of the encoder phase
  if (x.H > 4) {   // wider classifiers: separate kernel
    float* base = x.ws + i * w.e_stride;
    CK(adt_headcls_bwd(base + w.e_o, x.d, x.P + lo.enc(i, E_SW), base + w.e_rec, x.ws + w.g_rec + i * x.recsz, (int)w.B, x.L, x.H, x.hd, x.s1, x.d,
                       x.G + lo.enc(i, E_SW), x.G + lo.enc(i, E_SB), x.st));
  }
  return attn_block_bwd(x, i, false);
}

// The table gradients (sasrec/model.py:34-41, :53-59, :72-76 reversed) in their three forms, the sum of the encoder blocks' partials beside
// them, and the last fold.  The side stream is in order: the join behind that sum also covers the decoder's work queued on it earlier -- a
// join of its own in front of the embedding gradient was one more cross-queue wait (5-9 us) on the caller's stream.
int table_gradients(const Bwd& x, DecSide& dec_side) {
  const WS& w = x.w; const Layout& lo = x.lo; float* const ws = x.ws; float* const G = x.G;
  const int phase = x.plan.phase;
  if (phase == 2 && !x.sp.det && adt::zero_f32_async(ws + w.rep, (size_t)NREP * w.rep_stride, (hipStream_t)x.st)) return adt_set_error("replica zero");
  // (nothing to put beside the embedding gradient when the optimizer's fold sums the partials: no empty fork / join pair then)
  SideStream* const sd2 = ((x.sp.side_sites & 4) && x.sp.parts && !x.call.late_parts) ? x.sd : nullptr;
  CK(dec_side.join(x, sd2 != nullptr));
  void* s2 = nullptr;
  CK(side_mark(sd2, 2, x.st));
  if (x.sp.det) {
    // item table: every item's rows (encoder ids, decoder ids, positive / negative items of the logits) summed by one owner in sorted
    // order ; positional table: one owner per position
    if (x.sd_sort && hipStreamWaitEvent((hipStream_t)x.st, x.sd_sort->join_ev[3], 0) != hipSuccess) return adt_set_error("backward: sort join");
    const uint32_t site4[4] = {SITE_EMB_SEQ, SITE_EMB_DEC, 0u, 0u};
    const int32_t* const ids2[2] = {x.seq, x.dec};
    const float* const dx2[2] = {ws + w.g_enc_x, ws + w.g_dec_x};
    CK(adt_item_segsum_posemb(reinterpret_cast<int32_t*>(ws + w.isort), 4, x.T, x.c->item_num + 1, 0xFu, site4, x.p, x.seed, sqrtf((float)x.d), G + lo.item(),
                              x.plan.prep_zeroed ? 0 : 1, ids2, dx2, site4, 2, (int)w.B, x.L, x.ro, G + lo.posw(), x.st));
  } else if (x.call.embed3) {      // encoder + decoder embedding rows + the positive-logit rows: one atomic row-add per token where their ids line up
    const bool by_forward = phase == 2 ? x.plan.seeds_virtual : x.plan.bce_fwd;      // (phase 2: the caller passes the ring only behind such a forward)
    CK(adt_embed_bwd3_prefetch(x.seq, x.dec, x.pos, ws + w.g_enc_x, ws + w.g_dec_x, x.f, ws + w.g_pos, x.T, x.L, x.p, x.seed, SITE_EMB_SEQ, SITE_EMB_DEC, x.ro,
                               G + lo.posw(), ws + w.rep, NREP, w.rep_stride, ring_prefetch_split(x.ring, by_forward, x.sp) ? &x.ring : nullptr, x.st));
  } else {
    CK(adt_embed_bwd_rep(x.seq, ws + w.g_enc_x, x.T, x.L, x.d, x.p, x.seed, SITE_EMB_SEQ, x.ro, G + lo.posw(), ws + w.rep, NREP, w.rep_stride, x.st));
  }
  CK(side_enter(sd2, 2, x.st, &s2));
  if (x.sp.parts && !x.call.late_parts) CK(reduce_partials(x.c, lo, w, x.sp, G, ws, true, phase == 0 && !dec_side.parts_done, s2));
  CK(side_join(sd2, 2, x.st));
  if (x.plan.defer_fold) return 0;
  return adt_replica_reduce2(G + lo.item(), ws + w.rep, (int64_t)(x.c->item_num + 1) * x.d, x.sp.det ? 0 : NREP, w.rep_stride, G + lo.posw(), x.Gq + lo.posw(),
                             (phase == 0 ? lo.total : lo.dec(0, 0)) - lo.posw(), NREPP, w.prep_stride, x.st);
}

// sort of the step's ids + gather plan of the sorted table gradients (a function of the ids and of fixed workspace addresses only), beside the
// decoder's chain kernels; joined in front of the sums (table_gradients)
int item_sort_begin(const Bwd& x) {
  const WS& w = x.w; float* const ws = x.ws;
  const int32_t* const ids4[4] = {x.seq, x.dec, x.pos, x.neg};
  const float* const rows4[4] = {ws + w.g_enc_x, ws + w.g_dec_x, x.f, x.f};
  const float* const coef4[4] = {nullptr, nullptr, ws + w.g_pos, ws + w.g_neg};
  const int kind4[4] = {0, 0, 1, 1};
  void* s2 = x.st;
  if (x.sd_sort) { CK(side_mark(x.sd_sort, 3, x.st)); CK(side_enter(x.sd_sort, 3, x.st, &s2)); }
  CK(adt_item_sort(ids4, 4, x.T, x.c->item_num + 1, rows4, coef4, kind4, x.ro, reinterpret_cast<int32_t*>(ws + w.isort), s2));
  if (x.sd_sort && hipEventRecord(x.sd_sort->join_ev[3], x.sd_sort->s) != hipSuccess) return adt_set_error("backward: sort event");
  return 0;
}

// phase 0 / 1: logits, decoder stack, the decoder-side table work
int decoder_phase(const Bwd& x, DecSide& dec_side) {
  if (x.w.prep != x.w.rep + NREP * x.w.rep_stride) return adt_set_error("workspace layout: replica areas not adjacent");
  if (x.sp.det) CK(item_sort_begin(x));
  LogitsSide logits;
  CK(logits.begin(x));
  for (int i = x.nl - 1; i >= 0; --i) CK(dec_block_backward(x, i, logits));
  return dec_side.begin(x);
}

// phase 0 / 2: last LayerNorm, encoder stack, table gradients, fold
int encoder_phase(const Bwd& x, DecSide& dec_side) {
  CK(last_layernorm_bwd(x));
  if (!x.sp.lnl_fused) CK(dec_side.enter(x));
  for (int i = x.nl - 1; i >= 0; --i) CK(enc_block_backward(x, i, dec_side));
  return table_gradients(x, dec_side);
}

}  // namespace

extern "C" {

int64_t adt_sasrec_param_layout(const adt_sasrec_cfg* cfg, int64_t* offsets) {
  Layout lo;
  if (!make_layout(cfg, &lo)) return adt_set_error("param_layout: bad cfg");
  if (offsets)
    for (int i = 0; i < 4 + 30 * cfg->num_layers; ++i) offsets[i] = lo.off[i];
  return lo.total;
}

int64_t adt_sasrec_workspace_floats(const adt_sasrec_cfg* cfg, int B) {
  WS w;
  make_ws(cfg, B, step_plan(cfg, B), &w);
  return w.total;
}

int64_t adt_sasrec_ws_offset(const adt_sasrec_cfg* cfg, int B, int what, int layer) {
  WS w;
  make_ws(cfg, B, step_plan(cfg, B), &w);
  const int64_t Td = up64(w.T * w.d), rec = up64(w.T * w.H * w.H);
  switch (what) {
    case ADT_WS_ENC_X: return w.enc_x + layer * Td;
    case ADT_WS_DEC_X: return w.dec_x + layer * Td;
    case ADT_WS_REC: return layer * w.e_stride + w.e_rec;
    case ADT_WS_POS_LOGITS: return w.posl;
    case ADT_WS_NEG_LOGITS: return w.negl;
    case ADT_WS_F: return w.f;
    case ADT_WS_G_ENC_X: return w.g_enc_x + layer * Td;
    case ADT_WS_G_DEC_X: return w.g_dec_x + layer * Td;
    case ADT_WS_G_REC: return w.g_rec + layer * rec;
    case ADT_WS_G_POS: return w.g_pos;
    case ADT_WS_G_NEG: return w.g_neg;
    case ADT_WS_LOSS: return w.loss;
    case ADT_WS_NORMS: return w.norms;
    case ADT_WS_SCAL: return w.scal;
  }
  return adt_set_error("ws_offset: unknown id %d", what);
}

int adt_sasrec_forward(const adt_sasrec_cfg* c, const float* P, float* ws, const int32_t* seq, const int32_t* dec,
                       const int32_t* pos, const int32_t* neg, int B, int training, const uint32_t* seed,
                       uint32_t b_offset, void* st) {
  Layout lo;
  WS w;
  StepPlan pl;
  CK(layout_ws(c, B, &lo, &w, &pl));
  const int T = (int)w.T, d = (int)w.d, H = (int)w.H, hd = d / H, L = (int)w.L, prec = c->prec;
  const int64_t Td = up64(w.T * w.d);
  const bool packed = (training & ADT_TRAIN_PACKED) != 0;       // the weight images were packed by adt_sasrec_step_begin* of this step
  training &= ADT_TRAIN_DROPOUT;
  const float p = training ? c->dropout : 0.f;
  const uint32_t ro = b_offset * (uint32_t)L;
  if (pl.pad_elide && !dec) return adt_set_error("forward: the pad prefixes need the decoder's ids");
  CK(encoder_forward(c, lo, w, pl, P, ws, seq, pos, neg, p, seed, b_offset, true, st, packed, dec));
  const float* f = ws + w.f;
  const int dd = d * d;
  const int B_ = (int)w.B;
  for (int i = 0; i < c->num_layers; ++i) {
    float* x = ws + w.dec_x + i * Td;
    float* y = ws + w.dec_x + (i + 1) * Td;
    float* base = ws + i * w.d_stride;   // d_* offsets are absolute for layer 0
    float *dn = base + w.d_dn, *qkv = base + w.d_qkv, *o1 = base + w.d_o1, *lse1 = base + w.d_lse1, *a1 = base + w.d_a1,
          *q2 = base + w.d_q2, *kv2 = base + w.d_kv2, *o2 = base + w.d_o2, *lse2 = base + w.d_lse2, *a2 = base + w.d_a2,
          *u = base + w.d_u;
    const float* sinw = P + lo.dec(i, D_SINW);
    const float* sinb = P + lo.dec(i, D_SINB);
    const float* einw = P + lo.dec(i, D_EINW);
    const float* einb = P + lo.dec(i, D_EINB);
    if (pl.use_seq) {   // the whole layer in one launch, one workgroup per sequence (adt_seqfwd.cuh)
      CK(dec_layer_seq_fwd(lo, w, pl, P, ws, dec, p, seed, b_offset, i, st));
      continue;
    }
    {  // [gather] ; D = LN(x) ; qkv = D Win^T + b                          (sasrec/model.py:53-59, modules.py:668-670)
      adt::FwdChainArgs a = fwd_args(T, L, B_, H, dec, p, seed, ro);
      a.x = i == 0 ? nullptr : x; a.E = P + lo.item(); a.P = P + lo.posw(); a.emb_scale = sqrtf((float)d); a.site0 = SITE_EMB_DEC;
      a.gamma = P + lo.dec(i, D_LNW); a.beta = P + lo.dec(i, D_LNB);
      for (int j = 0; j < 3; ++j) { a.W[j] = sinw + j * dd; a.b[j] = sinb + j * d; }
      a.o0 = x; a.ld0 = d; a.o1 = dn; a.ld1 = d; a.o2 = qkv; a.ld2 = 3 * d;
      CK(adt_launch_fwdchain(prec, 1, a, st));
    }
    CK(adt_attn_fwd(prec, qkv, 3 * d, qkv + d, 3 * d, qkv + 2 * d, 3 * d, B_, H, L, hd, 1, p, seed, dec_site(i, 0), b_offset, o1, d,
                    lse1, reinterpret_cast<uint32_t*>(base + w.d_mask1), st));
    {  // a1 = out_proj(o1); q2 = a1 Wq^T + bq
      adt::FwdChainArgs a = fwd_args(T, L, B_, H, dec, 0.f, nullptr, ro);
      a.x = o1; a.W[0] = P + lo.dec(i, D_SOW); a.b[0] = P + lo.dec(i, D_SOB); a.W[1] = einw; a.b[1] = einb;
      a.o0 = a1; a.ld0 = d; a.o2 = q2; a.ld2 = d;
      CK(adt_launch_fwdchain(prec, 3, a, st));
    }
    CK(adt_attn_fwd(prec, q2, d, kv2, 2 * d, kv2 + d, 2 * d, B_, H, L, hd, 1, p, seed, dec_site(i, 1), b_offset, o2, d, lse2,
                    reinterpret_cast<uint32_t*>(base + w.d_mask2), st));
    {  // a2 = out_proj(o2); y = (D + a2 + drop2(conv2 relu(drop1(conv1 a2)))) * mask       (:673-676, :629-633)
      adt::FwdChainArgs a = fwd_args(T, L, B_, H, dec, p, seed, ro);
      a.x = o2; a.r0 = dn; a.site1 = dec_site(i, 2); a.site2 = dec_site(i, 3);
      a.W[0] = P + lo.dec(i, D_EOW); a.b[0] = P + lo.dec(i, D_EOB);
      a.W[1] = P + lo.dec(i, D_C1W); a.b[1] = P + lo.dec(i, D_C1B);
      a.W[2] = P + lo.dec(i, D_C2W); a.b[2] = P + lo.dec(i, D_C2B);
      a.o0 = a2; a.ld0 = d; a.o1 = u; a.ld1 = d; a.o2 = y; a.ld2 = d;
      CK(adt_launch_fwdchain(prec, 4, a, st));
    }
  }
  return 0;
}

// adt_sasrec_forward (training) + adt_sasrec_loss_seed_nz in one call; on the lean per-sequence path (adt_sasrec_bce_deferred) without the
// k_final_fwd launch and without the BCE block of the loss assembly: the caller must then run adt_sasrec_backward with ADT_PHASE_BCE_HERE.
// The loss slots must have been zeroed (adt_sasrec_step_begin*).
int adt_sasrec_bce_deferred(const adt_sasrec_cfg* c) {
  const StepPlan pl = step_plan(c, 1);      // (no rule behind bce_deferred reads the batch size)
  if (pl.cfg_error[0]) (void)adt_set_error("%s", pl.cfg_error);
  return !pl.cfg_error[0] && pl.bce_deferred ? 1 : 0;
}
int adt_sasrec_forward_loss(const adt_sasrec_cfg* c, const float* P, float* ws, const int32_t* seq, const int32_t* dec, const int32_t* pos,
                            const int32_t* neg, int B, int training, const uint32_t* seed, uint32_t b_offset, const float* lambdas1,
                            const float* lambdas2, void* st) {
  return adt_sasrec_forward_loss_prefetch(c, P, ws, seq, dec, pos, neg, B, training, seed, b_offset, lambdas1, lambdas2, nullptr, 0, 0, nullptr, nullptr,
                                          nullptr, st);
}

int adt_sasrec_forward_loss_prefetch(const adt_sasrec_cfg* c, const float* P, float* ws, const int32_t* seq, const int32_t* dec, const int32_t* pos,
                                     const int32_t* neg, int B, int training, const uint32_t* seed, uint32_t b_offset, const float* lambdas1,
                                     const float* lambdas2, const int32_t* ring, int64_t slot_ints, int nslots, uint32_t* state, uint32_t* consumed,
                                     int32_t* staging, void* st) {
  Layout lo;
  WS w;
  StepPlan pl;
  CK(layout_ws(c, B, &lo, &w, &pl));
  if ((training & ADT_TRAIN_DROPOUT) && (training & ADT_TRAIN_PACKED)) {      // training forward on weight images packed by this step's adt_sasrec_step_begin*
    const adt::RingPrefetchArgs rr{ring, (size_t)slot_ints, nslots, (size_t)(4 * w.T + 4), state, consumed, staging, 0, 0};
    const int rc = forward_loss_lean(c, lo, w, pl, P, ws, seq, dec, pos, neg, (training & ADT_TRAIN_BCE_SIDE) != 0, c->dropout, seed, b_offset, lambdas1, lambdas2, rr, st);
    if (rc <= 0) return rc;
  }
  CK(adt_sasrec_forward(c, P, ws, seq, dec, pos, neg, B, training, seed, b_offset, st));
  return adt_sasrec_loss_seed_nz(c, ws, pos, B, lambdas1, lambdas2, st);
}

// Measurement hook (bench.py roofline): launches ONLY the fused forward of decoder layer `layer` on the workspace of a completed
// adt_sasrec_forward of the same batch (its inputs -- log_feats, the layer input, the packed weight images -- are read from there).
int adt_sasrec_probe_dec_layer_fwd(const adt_sasrec_cfg* c, const float* P, float* ws, const int32_t* dec, int B, int training,
                                   const uint32_t* seed, uint32_t b_offset, int layer, void* st) {
  Layout lo;
  WS w;
  StepPlan pl;
  CK(layout_ws(c, B, &lo, &w, &pl));
  if (layer < 0 || layer >= c->num_layers) return adt_set_error("probe: layer %d", layer);
  if (!pl.use_seq) return adt_set_error("probe: the fused decoder layer does not cover this configuration");
  return dec_layer_seq_fwd(lo, w, pl, P, ws, dec, training ? c->dropout : 0.f, seed, b_offset, layer, st);
}

int adt_sasrec_step_begin(const adt_sasrec_cfg* c, float* ws, int B, uint32_t* seed, uint32_t seed_inc, const float* norms_src, const float* P,
                          float* G, int64_t n, float* scal, void* st) {
  Layout lo;
  WS w;
  StepPlan pl;
  CK(layout_ws(c, B, &lo, &w, &pl));
  int offs[256];
  const int npack = pack_offsets(c, lo, offs);
  return adt_step_begin_launch(seed, seed_inc, ws + w.norms, norms_src, ws + w.loss, 64 * (2 + 2 * c->num_layers), scal, G, n, P + lo.item(),
                               (int64_t)(c->item_num + 1) * c->hidden, ws + w.rep, (int64_t)NREP * w.rep_stride + (int64_t)NREPP * w.prep_stride,
                               P + lo.posw(), ws + w.wpack, offs, npack, st);      // item-table replicas + parameter replicas (adjacent): one fill
}

int adt_sasrec_step_begin_ring(const adt_sasrec_cfg* c, float* ws, int B, uint32_t* seed, uint32_t seed_inc, const int32_t* ring, int64_t slot_ints,
                               int nslots, int32_t* ids_dst, uint32_t* state, uint32_t* consumed, const float* P, float* G, int64_t n, float* scal,
                               void* st) {
  return adt_sasrec_step_begin_ring_staged(c, ws, B, seed, seed_inc, ring, slot_ints, nslots, ids_dst, state, consumed, nullptr, nullptr, P, G, n, scal, st);
}

int adt_sasrec_step_begin_ring_staged(const adt_sasrec_cfg* c, float* ws, int B, uint32_t* seed, uint32_t seed_inc, const int32_t* ring,
                                      int64_t slot_ints, int nslots, int32_t* ids_dst, uint32_t* state, uint32_t* consumed, const int32_t* staging,
                                      const uint32_t* produced, const float* P, float* G, int64_t n, float* scal, void* st) {
  Layout lo;
  WS w;
  StepPlan pl;
  CK(layout_ws(c, B, &lo, &w, &pl));
  int offs[256];
  const int npack = pack_offsets(c, lo, offs);
  return adt_step_begin_ring_launch(seed, seed_inc, ws + w.norms, ws + w.loss, 64 * (2 + 2 * c->num_layers), scal, G, n, P + lo.item(),
                                    (int64_t)(c->item_num + 1) * c->hidden, ring, slot_ints, nslots, ids_dst, 4 * (int64_t)w.T + 4, state, consumed,
                                    staging, produced, ws + w.rep, (int64_t)NREP * w.rep_stride + (int64_t)NREPP * w.prep_stride, P + lo.posw(),
                                    ws + w.wpack, offs, npack, st);
}

static int loss_seed_impl(const adt_sasrec_cfg* c, float* ws, const int32_t* pos, int B, const float* lambdas1, const float* lambdas2,
                          bool zero_loss, void* st);
int adt_sasrec_loss_seed(const adt_sasrec_cfg* c, float* ws, const int32_t* pos, int B, const float* lambdas1,
                         const float* lambdas2, void* st) {
  return loss_seed_impl(c, ws, pos, B, lambdas1, lambdas2, true, st);
}
int adt_sasrec_loss_seed_nz(const adt_sasrec_cfg* c, float* ws, const int32_t* pos, int B, const float* lambdas1,
                            const float* lambdas2, void* st) {
  return loss_seed_impl(c, ws, pos, B, lambdas1, lambdas2, false, st);
}
static int loss_seed_impl(const adt_sasrec_cfg* c, float* ws, const int32_t* pos, int B, const float* lambdas1, const float* lambdas2,
                          bool zero_loss, void* st) {
  WS w;
  const StepPlan pl = step_plan(c, B);
  make_ws(c, B, pl, &w);
  const int nl = c->num_layers, T = (int)w.T, H = (int)w.H;
  const int64_t Td = up64(w.T * w.d), rec = up64(w.T * w.H * w.H);
  float* loss = ws + w.loss;
  const float* norms = ws + w.norms;
  if (zero_loss && adt::zero_f32_async(loss, (size_t)64 * (2 + 2 * nl), (hipStream_t)st)) return adt_set_error("loss zero");
  if (pl.loss_one_launch) {   // one launch for all of them (adt_misc.cuh: k_loss_seeds)
    LossPtrs q;
    AdtLossSeedsJob job = loss_terms(w, ws, lambdas1, lambdas2, true, &q);
    job.pos_logits = ws + w.posl; job.neg_logits = ws + w.negl; job.pos = pos; job.dpos = ws + w.g_pos; job.dneg = ws + w.g_neg;
    return adt_loss_seeds_prefetch(job, st);
  }
  CK(adt_bce_seed(ws + w.posl, ws + w.negl, pos, T, norms, ws + w.g_pos, ws + w.g_neg, loss, st));
  for (int i = 0; i < nl; ++i)   // enc_in[i] pairs with dec_out_rev[i] = DEC_X[nl - i]      (sasrec/main.py:155-158)
    CK(adt_mse_seed(ws + w.enc_x + i * Td, ws + w.dec_x + (nl - i) * Td, w.T * w.d, lambdas1[i], norms, ws + w.g_enc_x + i * Td, 0,
                    ws + w.g_dec_x + (nl - i) * Td, loss + 64 * (2 + i), st));
  if (H > 1)
    for (int l = 0; l < nl; ++l)   // stale loop index: lambdas2[nl-1] for every layer          (sasrec/main.py:169)
      CK(adt_nll_seed(ws + l * w.e_stride + w.e_rec, T, H, lambdas2[nl - 1], norms, ws + w.g_rec + l * rec, loss + 64 * (2 + nl + l), st));
  return 0;
}

// the measurement hook of time_mark above
int adt_debug_time_launch(int which, int layer, void* ev_start, void* ev_stop) {
  g_time_which = which; g_time_layer = layer; g_time_ev0 = (hipEvent_t)ev_start; g_time_ev1 = (hipEvent_t)ev_stop;
  return 0;
}

int adt_sasrec_backward(const adt_sasrec_cfg* c, const float* P, float* G, float* ws, const int32_t* seq,
                        const int32_t* dec, const int32_t* pos, const int32_t* neg, int B, int training,
                        const uint32_t* seed, uint32_t b_offset, int phase, void* st) {
  return adt_sasrec_backward_prefetch(c, P, G, ws, seq, dec, pos, neg, B, training, seed, b_offset, phase, nullptr, 0, 0, nullptr, nullptr, nullptr, st);
}

int adt_sasrec_backward_prefetch(const adt_sasrec_cfg* c, const float* P, float* G, float* ws, const int32_t* seq, const int32_t* dec,
                                 const int32_t* pos, const int32_t* neg, int B, int training, const uint32_t* seed, uint32_t b_offset, int phase,
                                 const int32_t* ring, int64_t slot_ints, int nslots, uint32_t* state, uint32_t* consumed, int32_t* staging, void* st) {
  Bwd x;
  const adt::RingPrefetchArgs rr{ring, (size_t)slot_ints, nslots, (size_t)(4 * (int64_t)B * c->maxlen + 4), state, consumed, staging, 1, 2};
  CK(bwd_init(x, c, P, G, ws, seq, dec, pos, neg, B, training, seed, b_offset, phase, rr, st));
  DecSide dec_side;
  if (x.plan.phase == 0 || x.plan.phase == 1) CK(decoder_phase(x, dec_side));
  if (x.plan.phase == 0 || x.plan.phase == 2) CK(encoder_phase(x, dec_side));
  return 0;
}

static int fold_impl(bool adam, const adt_sasrec_cfg* c, float* ws, int B, float* P, float* G, float* M, float* V, float wd, float clip, float lr,
                     float b1, float b2, float eps, float* scal, void* st) {
  Layout lo;
  WS w;
  StepPlan pl;
  CK(layout_ws(c, B, &lo, &w, &pl));
  float* const Gq = ws + w.prep - lo.posw();
  if (pl.fold_parts) {      // single-GPU step: the partials are summed by the optimizer's first kernel, not by k_dwpart_reduce launches
    int slots[256], offs[256];
    const int ns = partial_slots(c, lo, true, true, slots, offs);
    int nwg[256];
    for (int i = 0; i < ns; ++i) nwg[i] = partial_nwg(pl, slots[i], B);
    // the stored bias / LayerNorm / classifier sums (BwdChainArgs::vpart: the kernels' sRed layouts) -> 64-float chunks of G
    int vsrc[128], vnwg[128], vstr[128], voff[128];
    int nv = 0;
    const int nsplit_wg = B * pl.seq_split, nattn_wg = B * pl.attn_split, d = c->hidden;
    auto chunk = [&](int layer, int k, int t0, int nw, int64_t goff) {
      vsrc[nv] = (int)((int64_t)(5 * layer + k) * w.vcall + t0); vnwg[nv] = nw; vstr[nv] = 512; voff[nv] = (int)goff; ++nv;
    };
    for (int i = 0; i < c->num_layers; ++i) {
      chunk(i, 0, 256, nsplit_wg, lo.dec(i, D_C2B)); chunk(i, 0, 320, nsplit_wg, lo.dec(i, D_C1B)); chunk(i, 0, 384, nsplit_wg, lo.dec(i, D_EOB));
      chunk(i, 1, 0, nsplit_wg, lo.dec(i, D_EINB)); chunk(i, 1, 64, nsplit_wg, lo.dec(i, D_SOB));
      chunk(i, 1, 128, nsplit_wg, lo.dec(i, D_EINB) + d); chunk(i, 1, 192, nsplit_wg, lo.dec(i, D_EINB) + 2 * d);
      chunk(i, 2, 0, nattn_wg, lo.dec(i, D_LNW)); chunk(i, 2, 64, nattn_wg, lo.dec(i, D_LNB));
      for (int j = 0; j < 3; ++j) chunk(i, 2, 128 + 64 * j, nattn_wg, lo.dec(i, D_SINB) + j * d);
      chunk(i, 3, 0, nsplit_wg, lo.enc(i, E_LN2W)); chunk(i, 3, 64, nsplit_wg, lo.enc(i, E_LN2B));
      if (c->num_heads > 1) { chunk(i, 3, 128, nsplit_wg, lo.enc(i, E_SW)); chunk(i, 3, 192, nsplit_wg, lo.enc(i, E_SB)); }
      chunk(i, 3, 256, nsplit_wg, lo.enc(i, E_C2B)); chunk(i, 3, 320, nsplit_wg, lo.enc(i, E_C1B)); chunk(i, 3, 384, nsplit_wg, lo.enc(i, E_OB));
      chunk(i, 4, 0, nattn_wg, lo.enc(i, E_LN1W)); chunk(i, 4, 64, nattn_wg, lo.enc(i, E_LN1B));
      for (int j = 0; j < 3; ++j) chunk(i, 4, 128 + 64 * j, nattn_wg, lo.enc(i, E_INB) + j * d);
    }
    if (pl.lnl_fused) {      // the last LayerNorm: per-workgroup sums of the first encoder kernel of the backward (BwdChainArgs::vpart2)
      chunk(c->num_layers, 0, 0, nsplit_wg, lo.lnl_w()); chunk(c->num_layers, 0, 64, nsplit_wg, lo.lnl_b());
    } else {      // per-block sums of k_ln_bwd (dgamma | dbeta, 128 floats per block)
      const int T = B * c->maxlen, nb = (T + 15) / 16 < LN_PART_BLOCKS ? (T + 15) / 16 : LN_PART_BLOCKS;
      const int base = (int)(w.lnpart - w.vpart);
      vsrc[nv] = base; vnwg[nv] = nb; vstr[nv] = 128; voff[nv] = (int)lo.lnl_w(); ++nv;
      vsrc[nv] = base + 64; vnwg[nv] = nb; vstr[nv] = 128; voff[nv] = (int)lo.lnl_b(); ++nv;
    }
    if (!adam)
      return adt_fold_parts(P, G, lo.total, G + lo.item(), ws + w.rep, (int64_t)(c->item_num + 1) * c->hidden, pl.det ? 0 : NREP, w.rep_stride,
                            G + lo.posw(), Gq + lo.posw(), lo.total - lo.posw(), 0, w.prep_stride, ws + w.part, w.part_stride, nwg, slots, offs, ns,
                            ws + w.vpart, vsrc, vnwg, vstr, voff, nv, ws + w.gnpart, scal, st);
    return adt_fold_parts_clip_adam(P, G, M, V, lo.total, G + lo.item(), ws + w.rep, (int64_t)(c->item_num + 1) * c->hidden, pl.det ? 0 : NREP,
                                    w.rep_stride, G + lo.posw(), Gq + lo.posw(), lo.total - lo.posw(), 0 /* no replicas: partials */, w.prep_stride,
                                    ws + w.part, w.part_stride, nwg, slots, offs, ns, ws + w.vpart, vsrc, vnwg, vstr, voff, nv, ws + w.gnpart,
                                    wd, clip, lr, b1, b2, eps, scal, st);
  }
  if (!adam)      // the replica fold the backward left out (phase bit 8)
    return adt_replica_reduce2(G + lo.item(), ws + w.rep, (int64_t)(c->item_num + 1) * c->hidden, pl.det ? 0 : NREP, w.rep_stride, G + lo.posw(),
                               Gq + lo.posw(), lo.total - lo.posw(), NREPP, w.prep_stride, st);
  return adt_fold_clip_adam(P, G, M, V, lo.total, G + lo.item(), ws + w.rep, (int64_t)(c->item_num + 1) * c->hidden, pl.det ? 0 : NREP, w.rep_stride, G + lo.posw(),
                            Gq + lo.posw(), lo.total - lo.posw(), NREPP, w.prep_stride, wd, clip, lr, b1, b2, eps, scal, st);
}

int adt_sasrec_fold_clip_adam(const adt_sasrec_cfg* c, float* ws, int B, float* P, float* G, float* M, float* V, float wd, float clip, float lr,
                              float b1, float b2, float eps, float* scal, void* st) {
  return fold_impl(true, c, ws, B, P, G, M, V, wd, clip, lr, b1, b2, eps, scal, st);
}

int adt_sasrec_fold_grads(const adt_sasrec_cfg* c, float* ws, int B, float* P, float* G, float* scal, void* st) {
  return fold_impl(false, c, ws, B, P, G, nullptr, nullptr, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, scal, st);
}

int adt_sasrec_predict(const adt_sasrec_cfg* c, const float* P, float* ws, const int32_t* seq, const int32_t* cand,
                       int B, int C, float* logits, int32_t* rank, void* st) {
  Layout lo;
  WS w;
  StepPlan pl;
  CK(layout_ws(c, B, &lo, &w, &pl));
  const int T = (int)w.T, d = (int)w.d, L = (int)w.L;
  CK(encoder_forward(c, lo, w, pl, P, ws, seq, nullptr, nullptr, 0.f, nullptr, 0, false, st));
  // final_feat = log_feats[:, -1, :]  (sasrec/model.py:89): row b*L + L-1, i.e. ld = L*d starting at (L-1)*d
  return adt_score_rank(ws + w.f + (int64_t)(L - 1) * d, L * d, P + lo.item(), cand, B, C, d, logits, rank, st);
}


// ---- one layer per call (the supernet's candidate layers): include/adt_hip.h --------------------------------------------------------
namespace {
struct LayerSave { float *o, *h, *u, *lse, *mask, *a1, *q2, *kv2, *o2, *lse2, *mask2; int64_t total; };
// the plan of one layer per call: the shape alone (no tables, one layer)
static StepPlan layer_plan(int prec, int L, int d, int hd, int B) {
  const int H = (hd > 0 && d % hd == 0) ? d / hd : 0;
  const StepFacts f{prec, L, d, H, 1, B, 0, false, H > 0 ? adt_seq_attn_bwd_lds(L, H) : 0};
  return adt_step_plan(f, adt_seq_switches());
}
LayerSave layer_save(float* base, int B, int L, int H, int dec) {
  const int64_t T = (int64_t)B * L, row = up64(T * 32), ls = up64((int64_t)B * H * L), mk = up64((int64_t)B * H * L * 8);
  LayerSave s{};
  int64_t o = 0;
  auto take = [&](int64_t n) { float* r = base ? base + o : nullptr; o += n; return r; };
  s.o = take(row); s.h = take(row); s.u = take(row); s.lse = take(ls); s.mask = take(mk);
  if (dec) { s.a1 = take(row); s.q2 = take(row); s.kv2 = take(2 * row); s.o2 = take(row); s.lse2 = take(ls); s.mask2 = take(mk); }
  s.total = o;
  return s;
}
}  // namespace

// the lean path with all five per-sequence backward kernels (StepPlan::parts)
int adt_seq_layer_supported(int prec, int L, int d, int hd) { return layer_plan(prec, L, d, hd, 1).parts ? 1 : 0; }

int64_t adt_seq_layer_save_floats(int B, int L, int H, int dec) { return layer_save(nullptr, B, L, H, dec).total; }

int adt_seq_enc_layer_fwd(int B, int L, int H, const int32_t* ids, const float* x, const adt_enc_layer_ptrs* P, const float* wp_base,
                          const void* wp_img, float p, const uint32_t* seed, uint32_t site_attn, uint32_t site_ffn1, uint32_t site_ffn2,
                          uint32_t b_offset, int training, float* save, float* y, float y_scale, int y_acc, float* rec, void* st) {
  if (H != 1 && H != 2 && H != 4) return adt_set_error("seq_enc_layer_fwd: H=%d (d = 64 takes 1, 2 or 4 heads)", H);
  const int hd = 64 / H;
  const StepPlan pl = layer_plan(ADT_PREC_BF16, L, 64, hd, B);
  if (!pl.parts) return adt_set_error("seq_enc_layer_fwd: L=%d H=%d is not covered", L, H);
  const LayerSave s = layer_save(save, B, L, H, 0);
  adt::SeqFwdArgs a = seq_args(pl.seq_split, L, B, H, ids, p, seed, b_offset, hd);
  a.x = x; a.site_attn = site_attn; a.site1 = site_ffn1; a.site2 = site_ffn2;
  a.gamma = P->ln1_w; a.beta = P->ln1_b; a.Win = P->in_w; a.bin = P->in_b; a.Wo = P->out_w; a.bo = P->out_b;
  a.gamma2 = P->ln2_w; a.beta2 = P->ln2_b; a.W1 = P->c1_w; a.b1 = P->c1_b; a.W2 = P->c2_w; a.b2 = P->c2_b;
  a.y = y; a.y_scale = y_scale; a.y_acc = y_acc; a.wp_base = wp_base; a.wp_img = wp_img;
  if (training) { a.o = s.o; a.h = s.h; a.u = s.u; a.lse = s.lse; a.mask = reinterpret_cast<uint32_t*>(s.mask); a.saved_bf16 = 1; }
  else { a.lse = s.lse; }
  if (rec && H > 1) { a.rec = rec; a.Ws = P->cls_w; a.bs = P->cls_b; }
  return adt_launch_seq_enc_fwd(hd, a, st);
}

int adt_seq_enc_layer_bwd(int B, int L, int H, const int32_t* ids, const float* x, const adt_enc_layer_ptrs* P, const adt_enc_layer_ptrs* G,
                          const float* wp_base, const void* wp_img, float p, const uint32_t* seed, uint32_t site_attn, uint32_t site_ffn1,
                          uint32_t site_ffn2, uint32_t b_offset, const float* save, const float* gy, float gy_scale, const float* rec,
                          const float* drec, float* gx, int gx_acc, float* scratch, void* st) {
  if (H != 1 && H != 2 && H != 4) return adt_set_error("seq_enc_layer_bwd: H=%d (d = 64 takes 1, 2 or 4 heads)", H);
  const int hd = 64 / H, T = B * L;
  const StepPlan pl = layer_plan(ADT_PREC_BF16, L, 64, hd, B);
  if (!pl.parts) return adt_set_error("seq_enc_layer_bwd: L=%d H=%d is not covered", L, H);
  const LayerSave s = layer_save(const_cast<float*>(save), B, L, H, 0);
  float *dO = scratch, *dh = scratch + up64((int64_t)T * 64);
  {  // FFN + mask + forward_layernorm + out_proj (+ head classifier) reverse -> dh, dO
    adt::BwdChainArgs a = bwd_args(T, L, B, ids, p, seed, b_offset * (uint32_t)L);
    a.site1 = site_ffn1; a.site2 = site_ffn2; a.gy = gy; a.gy_scale = gy_scale; a.u = s.u; a.xin = s.h; a.o = s.o; a.saved_bf16 = 1;
    a.W0 = P->c2_w; a.W1 = P->c1_w; a.W2 = P->out_w; a.gamma = P->ln2_w; a.beta = P->ln2_b;
    a.dW0 = G->c2_w; a.dW1 = G->c1_w; a.dW2 = G->out_w; a.db0 = G->c2_b; a.db1 = G->c1_b; a.db2 = G->out_b; a.dgamma = G->ln2_w; a.dbeta = G->ln2_b;
    a.out0 = dh; a.out1 = dO; a.wp_base = wp_base; a.wp_img = wp_img;
    if (H > 1 && drec) { a.rec = rec; a.drec = drec; a.Ws = P->cls_w; a.dWs = G->cls_w; a.dbs = G->cls_b; a.H = H; }
    const int rc = adt_launch_seq_post_bwd(hd, 1, a, st);
    if (rc) return rc < 0 ? rc : adt_set_error("seq_enc_layer_bwd: post chain not covered");
  }
  adt::SeqBwdArgs a = seq_bwd_args(L, B, H, ids, p, seed, site_attn, b_offset, hd);
  a.x = x; a.gamma = P->ln1_w; a.beta = P->ln1_b; a.Win = P->in_w; a.bin = P->in_b;
  a.dO = dO; a.o = s.o; a.lse = s.lse; a.mask = reinterpret_cast<const uint32_t*>(s.mask); a.dres = dh; a.saved_bf16 = 1;
  a.gx = gx; a.acc = gx_acc; a.dWin = G->in_w; a.dbin = G->in_b; a.dgamma = G->ln1_w; a.dbeta = G->ln1_b;
  a.wp_base = wp_base; a.wp_img = wp_img;
  const int rc = adt_launch_seq_attn_pre_bwd(hd, 0, a, st);
  return rc <= 0 ? rc : adt_set_error("seq_enc_layer_bwd: attention block not covered");
}

int adt_seq_dec_layer_fwd(int B, int L, int H, const int32_t* ids, const float* x, const float* feats, const adt_dec_layer_ptrs* P,
                          const float* wp_base, const void* wp_img, float p, const uint32_t* seed, uint32_t site_slf, uint32_t site_enc,
                          uint32_t site_ffn1, uint32_t site_ffn2, uint32_t b_offset, float* save, float* y, float y_scale, int y_acc, void* st) {
  if (H != 1 && H != 2 && H != 4) return adt_set_error("seq_dec_layer_fwd: H=%d (d = 64 takes 1, 2 or 4 heads)", H);
  const int hd = 64 / H;
  const StepPlan pl = layer_plan(ADT_PREC_BF16, L, 64, hd, B);
  if (!pl.parts) return adt_set_error("seq_dec_layer_fwd: L=%d H=%d is not covered", L, H);
  const LayerSave s = layer_save(save, B, L, H, 1);
  adt::SeqFwdArgs a = seq_args(pl.seq_split, L, B, H, ids, p, seed, b_offset, hd);
  a.x = x; a.f = feats; a.site_attn = site_slf; a.site_attn2 = site_enc; a.site1 = site_ffn1; a.site2 = site_ffn2;
  a.gamma = P->ln_w; a.beta = P->ln_b; a.Win = P->sin_w; a.bin = P->sin_b; a.Wo = P->so_w; a.bo = P->so_b;
  a.Win2 = P->ein_w; a.bin2 = P->ein_b; a.Wo2 = P->eo_w; a.bo2 = P->eo_b; a.W1 = P->c1_w; a.b1 = P->c1_b; a.W2 = P->c2_w; a.b2 = P->c2_b;
  a.o = s.o; a.lse = s.lse; a.mask = reinterpret_cast<uint32_t*>(s.mask); a.a1 = s.a1; a.q2 = s.q2; a.kv2 = s.kv2; a.o2 = s.o2;
  a.lse2 = s.lse2; a.mask2 = reinterpret_cast<uint32_t*>(s.mask2); a.h = s.h; a.u = s.u; a.saved_bf16 = 1;
  a.y = y; a.y_scale = y_scale; a.y_acc = y_acc; a.wp_base = wp_base; a.wp_img = wp_img;
  return adt_launch_seq_dec_fwd(hd, a, st);
}

int adt_seq_dec_layer_bwd(int B, int L, int H, const int32_t* ids, const float* x, const float* feats, const adt_dec_layer_ptrs* P,
                          const adt_dec_layer_ptrs* G, const float* wp_base, const void* wp_img, float p, const uint32_t* seed,
                          uint32_t site_slf, uint32_t site_enc, uint32_t site_ffn1, uint32_t site_ffn2, uint32_t b_offset, const float* save,
                          const float* gy, float gy_scale, float* gx, int gx_acc, float* gfeats, float* scratch, void* st) {
  if (H != 1 && H != 2 && H != 4) return adt_set_error("seq_dec_layer_bwd: H=%d (d = 64 takes 1, 2 or 4 heads)", H);
  const int hd = 64 / H, T = B * L, d = 64;
  const StepPlan pl = layer_plan(ADT_PREC_BF16, L, 64, hd, B);
  if (!pl.parts) return adt_set_error("seq_dec_layer_bwd: L=%d H=%d is not covered", L, H);
  const LayerSave s = layer_save(const_cast<float*>(save), B, L, H, 1);
  const int64_t Td = up64((int64_t)T * 64);
  float *s1 = scratch, *s5 = scratch + Td, *s4 = scratch + 2 * Td;      // dO (T x 64), dq2 (T x 64), dk2 | dv2 (T x 128)
  const uint32_t ro = b_offset * (uint32_t)L;
  {  // FFN + mask + enc_attn.out_proj reverse -> dO2 (s1)
    adt::BwdChainArgs a = bwd_args(T, L, B, ids, p, seed, ro);
    a.site1 = site_ffn1; a.site2 = site_ffn2; a.gy = gy; a.gy_scale = gy_scale; a.u = s.u; a.xin = s.h; a.o = s.o2; a.saved_bf16 = 1;
    a.W0 = P->c2_w; a.W1 = P->c1_w; a.W2 = P->eo_w; a.dW0 = G->c2_w; a.dW1 = G->c1_w; a.dW2 = G->eo_w;
    a.db0 = G->c2_b; a.db1 = G->c1_b; a.db2 = G->eo_b; a.out0 = s1; a.wp_base = wp_base; a.wp_img = wp_img;
    const int rc = adt_launch_seq_post_bwd(hd, 0, a, st);
    if (rc) return rc < 0 ? rc : adt_set_error("seq_dec_layer_bwd: post chain not covered");
  }
  {  // cross attention core: dq2 -> s5, dk2 | dv2 -> s4
    const uint16_t* kvb = reinterpret_cast<const uint16_t*>(s.kv2);
    CK(adt_attn_bwd_saved_bf16(s.q2, d, kvb, 2 * d, kvb + d, 2 * d, s.o2, d, s.lse2, s1, d, B, H, L, hd, p, seed, site_enc, b_offset, s5, d, s4,
                               2 * d, s4 + d / 2, 2 * d, reinterpret_cast<const uint32_t*>(s.mask2), 1, st));      // bf16 rows for k_seqtt_mid_bwd below
  }
  {  // enc_attn q / k / v projections and slf_attn.out_proj reverse -> dO1 (s1), d feats +=
    adt::BwdChainArgs a = bwd_args(T, L, B, ids, 0.f, nullptr, ro);
    a.dqkv = s5; a.lddqkv = d; a.xin = s.a1; a.o = s.o; a.saved_bf16 = 1; a.dkv2 = s4; a.f = feats; a.grad_bf16 = 1;
    a.W0 = P->ein_w; a.W1 = P->so_w; a.W2 = P->ein_w + d * d; a.W3 = P->ein_w + 2 * d * d;
    a.dW0 = G->ein_w; a.dW1 = G->so_w; a.dW2 = G->ein_w + d * d; a.dW3 = G->ein_w + 2 * d * d;
    a.db0 = G->ein_b; a.db1 = G->so_b; a.db2 = G->ein_b + d; a.db3 = G->ein_b + 2 * d;
    a.out0 = s1; a.out1 = gfeats; a.acc1 = 1; a.wp_base = wp_base; a.wp_img = wp_img;
    const int rc = adt_launch_seq_mid_bwd(hd, a, st);
    if (rc) return rc < 0 ? rc : adt_set_error("seq_dec_layer_bwd: mid chain not covered");
  }
  adt::SeqBwdArgs a = seq_bwd_args(L, B, H, ids, p, seed, site_slf, b_offset, hd);
  a.x = x; a.gamma = P->ln_w; a.beta = P->ln_b; a.Win = P->sin_w; a.bin = P->sin_b;
  a.dO = s1; a.o = s.o; a.lse = s.lse; a.mask = reinterpret_cast<const uint32_t*>(s.mask); a.dres = gy; a.dres_scale = gy_scale; a.saved_bf16 = 1;
  a.gx = gx; a.acc = gx_acc; a.dWin = G->sin_w; a.dbin = G->sin_b; a.dgamma = G->ln_w; a.dbeta = G->ln_b;
  a.wp_base = wp_base; a.wp_img = wp_img;
  const int rc = adt_launch_seq_attn_pre_bwd(hd, 1, a, st);
  return rc <= 0 ? rc : adt_set_error("seq_dec_layer_bwd: attention block not covered");
}

}  // extern "C"
