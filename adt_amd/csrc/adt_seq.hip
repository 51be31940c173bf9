// Launchers of the per-sequence fused layer kernels (adt_seqfwd.cuh, adt_seqbwd.cuh): one workgroup per user sequence.
#include "adt_host.h"
#include <limits.h>
#include <atomic>
#include "adt_seqfwd.cuh"
#include "adt_seqfwd_tt.cuh"
#include "adt_seqattn.cuh"
#include "adt_seqbwd_tt.cuh"
#include "adt_seqpost_tt.cuh"
#include "adt_seqxattn_tt.cuh"

using namespace adt;

template <class Args>
static int seq_launch(const void* fn, size_t smem, AdtLdsOptIn& slot, int grid, const Args* args, hipStream_t s, const char* what, int nwaves = SQ_NW,
                      size_t optin = 0) {
  return adt_launch_lds1(fn, dim3(grid), dim3(nwaves * 64), smem, *args, s, what, slot, optin);
}

// ---- pre-packed weight images (adt_wave.cuh: WPack) -----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pack_wimg(PackArgs a) { pack_wimg_block(a, blockIdx.x); }      // adt_wave.cuh

extern "C" int adt_pack_wimg(const float* base, void* img, const int* offs, int n, void* stream) {
  if (n < 1 || n > 256) return adt_set_error("pack_wimg: %d blocks", n);
  PackArgs a;
  a.base = base; a.img = reinterpret_cast<__bf16*>(img); a.n = n;
  for (int i = 0; i < n; ++i) a.off[i] = offs[i];
  hipLaunchKernelGGL(k_pack_wimg, dim3(n), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("pack_wimg");
}

static_assert(ADT_SEQ_MAXLEN == SQ_LP && ADT_SEQ_MAXLEN == SB_R, "adt_step_plan.h restates the image rows of these kernels");

// The one place that reads the flagship switches from the environment: all of them, at the first flagship call of the process.
const SeqSwitches& adt_seq_switches() {
  static const SeqSwitches sw = [] {
    SeqSwitches s;
    s.seq = adt_env_on("ADT_SEQ"); s.seq_lean = adt_env_on("ADT_SEQ_LEAN"); s.seq_tt = adt_env_on("ADT_SEQ_TT"); s.seq_bwd = adt_env_on("ADT_SEQ_BWD");
    s.seq_attn_bwd = adt_env_on("ADT_SEQ_ATTN_BWD"); s.seq_post_bwd = adt_env_on("ADT_SEQ_POST_BWD"); s.seq_partials = adt_env_on("ADT_SEQ_PARTIALS");
    s.xattn_fused = adt_env_on("ADT_XATTN_FUSED"); s.do_bf16 = adt_env_on("ADT_DO_BF16"); s.pad_elide = adt_env_on("ADT_PAD_ELIDE");
    s.seq_ablate = adt_env_int("ADT_SEQ_ABLATE", 0); s.seq_ablate_set = adt_env_int("ADT_SEQ_ABLATE", INT_MIN) != INT_MIN;
    s.seq_split = adt_env_int("ADT_SEQ_SPLIT", 0); s.attn_split = adt_env_on("ADT_ATTN_SPLIT");
    s.side_stream = adt_env_int("ADT_SIDE_STREAM", 7); s.side_stream_dp = adt_env_int("ADT_SIDE_STREAM_DP", 0) != 0;
    s.item_sort = adt_env_int("ADT_ITEM_SORT", 0) != 0;      // opt-in: +12 us per flagship step (0.637 against 0.625 ms: DESIGN.md "item-table gradient")
    s.lnl_fused = adt_env_on("ADT_LNL_FUSED"); s.fold_parts = adt_env_on("ADT_FOLD_PARTS"); s.fwd_fused = adt_env_on("ADT_FWD_FUSED");
    s.embed3 = adt_env_on("ADT_EMBED3"); s.bce_merged = adt_env_on("ADT_BCE_MERGED");
    return s;
  }();
  return sw;
}

// the shape of an argument block, as the coverage rules of adt_step_plan.h read it
static SeqAttnFacts attn_facts(const AttnArgs& a) {
  return {a.L, a.H, a.B, a.causal != 0, a.in_bf16 != 0, a.out_bf16 != 0, a.ldq, a.ldk, a.ldv, a.ldo, a.lddo, a.drop.thr != 0, a.mask != nullptr,
          sab_lds_bytes(a.L, a.H), xm_lds_bytes(a.L, a.H)};
}
size_t adt_seq_attn_bwd_lds(int L, int H) { return sab_lds_bytes(L, H); }      // StepFacts::sab_lds
static SeqChainFacts chain_facts(const BwdChainArgs& a) {
  return {a.L, a.H, a.B, a.T, a.wp_img != nullptr, a.saved_bf16 != 0, a.grad_bf16 != 0, a.part[0] && a.part[1] && a.part[2] && a.part[3], a.nsplit, a.ablate,
          a.drec != nullptr};
}

static unsigned long long* g_stamps = nullptr;

extern "C" int adt_seq_stamps_read(unsigned long long* out, int n) {      // debugging aid of tools/seq_stamps.py, not part of include/adt_hip.h
  if (!g_stamps) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  return hipMemcpy(out, g_stamps, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}

// ADT_SEQ_STAMPS=1: forward kernels; =2: the attention backward; =3: the encoder post chain backward; =4: the decoder cross-attention backward
// alone (k_seq_attn_bwd); =5: the decoder mid chain (k_seqtt_mid_bwd); =6: the two in one launch (k_seqtt_xattn_mid_bwd)
static int seq_stamps_mode() {
  static const int st = [] {
    const int v = adt_env_int("ADT_SEQ_STAMPS", 0);
    return (v && hipMalloc(&g_stamps, 16 * 16 * sizeof(unsigned long long)) != hipSuccess) ? 0 : v;
  }();
  return st;
}
static unsigned long long* seq_stamp_buffer(bool for_attention) { return seq_stamps_mode() == (for_attention ? 2 : 1) ? g_stamps : nullptr; }
static unsigned long long* seq_stamp_buffer_post() { return seq_stamps_mode() == 3 ? g_stamps : nullptr; }
static unsigned long long* seq_stamp_buffer_mode(int mode) { return seq_stamps_mode() == mode ? g_stamps : nullptr; }

static void seq_ablate(SeqFwdArgs& a) {
  a.stamps = seq_stamp_buffer(false);
  const int ab = adt_seq_switches().seq_ablate;
  a.ablate = ab;
  if (ab & 1) { a.qkv = nullptr; a.o = nullptr; a.h = nullptr; a.u = nullptr; a.a1 = nullptr; a.q2 = nullptr; a.kv2 = nullptr; a.o2 = nullptr; a.mask = nullptr; a.mask2 = nullptr; }
}

static bool seq_use_tt(const SeqFwdArgs& a) {     // register-resident transposed chains (adt_seqfwd_tt.cuh); ADT_SEQ_TT=0: the row-major fused form
  return adt_seq_fwd_tt(adt_seq_switches(), a.wp_img != nullptr, a.L);
}

// Launches of a chain kernel ISSUED by this process that were given the pad prefixes (SeqFwdArgs / SeqBwdArgs / BwdChainArgs / AttnArgs::pad_pre;
// StepPlan::pad_elide): like adt_seq_do_handover_launches below a debugging aid of the tests, not part of include/adt_hip.h
static std::atomic<unsigned long long> g_pad_elide_launches{0};
extern "C" unsigned long long adt_seq_pad_elide_launches() { return g_pad_elide_launches.load(); }
static int pad_refused(int hd, const void* pad_pre) {      // the 16-wide-head instantiations ignore the prefixes: StepPlan::pad_elide never names them there
  return (pad_pre && hd == 16) ? adt_set_error("per-sequence kernels: pad prefixes with 16-wide heads") : 0;
}
static int pad_counted(int rc, const void* pad_pre) {
  if (rc == 0 && pad_pre) ++g_pad_elide_launches;
  return rc;
}

int adt_launch_seq_enc_fwd(int hd, const SeqFwdArgs& a, void* stream) {
  static AdtLdsOptIn optin[3], optin_tt[3];
  if (pad_refused(hd, a.pad_pre)) return -1;
  SeqFwdArgs args = a;
  seq_ablate(args);
  hipStream_t s = (hipStream_t)stream;
  if (seq_use_tt(args)) {
    const int nsp = args.nsplit > 1 ? args.nsplit : 1;
    const size_t smem_tt = SeqTtLds<6>::bytes;
    if (hd == 64) return pad_counted(seq_launch((const void*)k_seqtt_enc_fwd<64>, smem_tt, optin_tt[0], a.B * nsp, &args, s, "seqtt_enc_fwd<64>", TQ_FWD_NW), a.pad_pre);
    if (hd == 32) return pad_counted(seq_launch((const void*)k_seqtt_enc_fwd<32>, smem_tt, optin_tt[1], a.B * nsp, &args, s, "seqtt_enc_fwd<32>", TQ_FWD_NW), a.pad_pre);
    if (hd == 16) return pad_counted(seq_launch((const void*)k_seqtt_enc_fwd<16>, smem_tt, optin_tt[2], a.B * nsp, &args, s, "seqtt_enc_fwd<16>", TQ_FWD_NW), a.pad_pre);
  }
  if (a.pad_pre) return adt_set_error("seq_enc_fwd: the pad prefixes belong to the transposed-chain kernels (L=%d hd=%d)", a.L, hd);
  args.nsplit = 0;
  const size_t smem = SeqFwdLds<6>::bytes;
  if (hd == 64) return seq_launch((const void*)k_seq_enc_fwd<64, 2>, smem, optin[0], a.B, &args, s, "seq_enc_fwd<64>");
  if (hd == 32) return seq_launch((const void*)k_seq_enc_fwd<32, 2>, smem, optin[1], a.B, &args, s, "seq_enc_fwd<32>");
  if (hd == 16) return seq_launch((const void*)k_seq_enc_fwd<16, 4>, smem, optin[2], a.B, &args, s, "seq_enc_fwd<16>");
  return adt_set_error("seq_enc_fwd: head size %d", hd);
}

int adt_launch_seq_dec_fwd(int hd, const SeqFwdArgs& a, void* stream) {
  static AdtLdsOptIn optin[3], optin_tt[3];
  if (pad_refused(hd, a.pad_pre)) return -1;
  SeqFwdArgs args = a;
  seq_ablate(args);
  hipStream_t s = (hipStream_t)stream;
  if (seq_use_tt(args)) {
    const int nsp = args.nsplit > 1 ? args.nsplit : 1;
    const size_t smem_tt = SeqTtLds<5>::bytes;
    if (hd == 64) return pad_counted(seq_launch((const void*)k_seqtt_dec_fwd<64>, smem_tt, optin_tt[0], a.B * nsp, &args, s, "seqtt_dec_fwd<64>", TQ_FWD_NW), a.pad_pre);
    if (hd == 32) return pad_counted(seq_launch((const void*)k_seqtt_dec_fwd<32>, smem_tt, optin_tt[1], a.B * nsp, &args, s, "seqtt_dec_fwd<32>", TQ_FWD_NW), a.pad_pre);
    if (hd == 16) return pad_counted(seq_launch((const void*)k_seqtt_dec_fwd<16>, smem_tt, optin_tt[2], a.B * nsp, &args, s, "seqtt_dec_fwd<16>", TQ_FWD_NW), a.pad_pre);
  }
  if (a.pad_pre) return adt_set_error("seq_dec_fwd: the pad prefixes belong to the transposed-chain kernels (L=%d hd=%d)", a.L, hd);
  args.nsplit = 0;
  const size_t smem = SeqFwdLds<5>::bytes;
  if (hd == 64) return seq_launch((const void*)k_seq_dec_fwd<64>, smem, optin[0], a.B, &args, s, "seq_dec_fwd<64>");
  if (hd == 32) return seq_launch((const void*)k_seq_dec_fwd<32>, smem, optin[1], a.B, &args, s, "seq_dec_fwd<32>");
  if (hd == 16) return seq_launch((const void*)k_seq_dec_fwd<16>, smem, optin[2], a.B, &args, s, "seq_dec_fwd<16>");
  return adt_set_error("seq_dec_fwd: head size %d", hd);
}

// Launches of an attention backward (k_seqtt_attn_pre_bwd, k_seq_attn_bwd, k_seqtt_xattn_mid_bwd) ISSUED by this process that took dO as
// handed-over bf16 rows + delta (SeqBwdArgs / AttnArgs::do_bf16); like adt_seq_xattn_fused_launches below a debugging aid of the tests, not
// part of include/adt_hip.h
static std::atomic<unsigned long long> g_do_handover_launches{0};
extern "C" unsigned long long adt_seq_do_handover_launches() { return g_do_handover_launches.load(); }

// causal attention backward, one workgroup per sequence (adt_seqattn.cuh); returns 1 when the shape is not covered (caller falls back)
int adt_launch_seq_attn_bwd(int hd, const AttnArgs& a, void* stream) {
  if (!adt_covers_attn_bwd(adt_seq_switches(), hd, attn_facts(a))) return 1;
  if (a.do_bf16 && (!a.do_delta || !a.in_bf16)) return adt_set_error("seq_attn_bwd: handed-over dO rows need their delta and bf16 operand rows");
  const size_t smem = sab_lds_bytes(a.L, a.H);
  const int mode = a.drop.thr == 0 ? 0 : (a.mask != nullptr ? 1 : 2);
  static AdtLdsOptIn optin[9];
  const void* fns[9] = {(const void*)k_seq_attn_bwd<64, 0>, (const void*)k_seq_attn_bwd<64, 1>, (const void*)k_seq_attn_bwd<64, 2>,
                        (const void*)k_seq_attn_bwd<32, 0>, (const void*)k_seq_attn_bwd<32, 1>, (const void*)k_seq_attn_bwd<32, 2>,
                        (const void*)k_seq_attn_bwd<16, 0>, (const void*)k_seq_attn_bwd<16, 1>, (const void*)k_seq_attn_bwd<16, 2>};
  const int slot = (hd == 64 ? 0 : hd == 32 ? 3 : 6) + mode;
  AttnArgs args = a;
  args.stamps = seq_stamp_buffer(true);
  if (!args.stamps) args.stamps = seq_stamp_buffer_mode(4);
  // smem varies with L: opt in once to the most this kernel may ask for
  const int rc = adt_launch_lds1(fns[slot], dim3(a.B), dim3(SAB_NW * 64), smem, args, (hipStream_t)stream, "seq_attn_bwd", optin[slot], ADT_LDS_MAX);
  if (rc == 0 && a.do_bf16) ++g_do_handover_launches;
  return rc;
}

// fused backward of one attention block (adt_seqbwd_tt.cuh); dec = 0: encoder block, 1: decoder self-attention block.
// Returns 1 when the shape is not covered (the caller runs the staged kernels).
template <int HD, bool DEC>
static int seq_attn_pre_bwd_t(int mode, const SeqBwdArgs& a, hipStream_t s) {
  constexpr int H = 64 / HD;
  const size_t smem = SeqBwdLds<H>::bytes;
  static AdtLdsOptIn optin[3];
  const void* fns[3] = {(const void*)k_seqtt_attn_pre_bwd<HD, 0, DEC>, (const void*)k_seqtt_attn_pre_bwd<HD, 1, DEC>,
                        (const void*)k_seqtt_attn_pre_bwd<HD, 2, DEC>};
  SeqBwdArgs args = a;
  args.stamps = seq_stamp_buffer(true);
  if (a.nsplit == 2 && !a.part) return adt_set_error("seqtt_attn_pre_bwd: two workgroups per sequence need the weight-gradient partials");
  if (a.nsplit != 2) args.nsplit = 1;
  const int rc = seq_launch(fns[mode], smem, optin[mode], a.B * args.nsplit, &args, s, "seqtt_attn_pre_bwd");
  if (rc == 0 && a.do_bf16) ++g_do_handover_launches;
  return pad_counted(rc, a.pad_pre);
}

int adt_launch_seq_attn_pre_bwd(int hd, int dec, const SeqBwdArgs& a, void* stream) {
  SeqChainFacts f{};
  f.L = a.L; f.H = a.H; f.B = a.B; f.T = a.B * a.L; f.wimg = a.wp_img != nullptr;
  if (!adt_covers_attn_pre_bwd(adt_seq_switches(), hd, f)) return 1;
  if (a.do_bf16 && !a.do_delta) return adt_set_error("seqtt_attn_pre_bwd: handed-over dO rows without their delta");
  if (pad_refused(hd, a.pad_pre)) return -1;
  const int mode = a.drop.thr == 0 ? 0 : (a.mask != nullptr ? 1 : 2);
  hipStream_t s = (hipStream_t)stream;
  if (hd == 32) return dec ? seq_attn_pre_bwd_t<32, true>(mode, a, s) : seq_attn_pre_bwd_t<32, false>(mode, a, s);
  if (hd == 64) return dec ? seq_attn_pre_bwd_t<64, true>(mode, a, s) : seq_attn_pre_bwd_t<64, false>(mode, a, s);
  return dec ? seq_attn_pre_bwd_t<16, true>(mode, a, s) : seq_attn_pre_bwd_t<16, false>(mode, a, s);
}

// per-sequence backward of the token-wise chains (adt_seqpost_tt.cuh); 0 launched, 1 not covered (the caller runs the row-major chain kernels)
int adt_launch_seq_post_bwd(int hd, int enc, const BwdChainArgs& a, void* stream) {
  if (!adt_covers_post_bwd(adt_seq_switches(), hd, enc != 0, chain_facts(a))) return 1;
  if (pad_refused(hd, a.pad_pre)) return -1;
  static AdtLdsOptIn optin[6];
  const void* fns[6] = {(const void*)k_seqtt_post_bwd<64, false>, (const void*)k_seqtt_post_bwd<64, true>, (const void*)k_seqtt_post_bwd<32, false>,
                        (const void*)k_seqtt_post_bwd<32, true>, (const void*)k_seqtt_post_bwd<16, false>, (const void*)k_seqtt_post_bwd<16, true>};
  const int slot = (hd == 64 ? 0 : hd == 32 ? 2 : 4) + (enc ? 1 : 0);
  BwdChainArgs args = a;
  args.stamps = enc ? seq_stamp_buffer_post() : nullptr;
  return pad_counted(seq_launch(fns[slot], SeqPostLds<3>::bytes, optin[slot], a.B * (a.nsplit > 1 ? a.nsplit : 1), &args, (hipStream_t)stream, "seqtt_post_bwd", SP_NW), a.pad_pre);
}

int adt_launch_seq_mid_bwd(int hd, const BwdChainArgs& a, void* stream) {
  if (!adt_covers_mid_bwd(adt_seq_switches(), hd, chain_facts(a))) return 1;
  static AdtLdsOptIn optin;
  BwdChainArgs args = a;
  args.stamps = seq_stamp_buffer_mode(5);
  return seq_launch((const void*)k_seqtt_mid_bwd, SeqPostLds<4>::bytes, optin, a.B * (a.nsplit > 1 ? a.nsplit : 1), &args, (hipStream_t)stream, "seqtt_mid_bwd", SP_MID_NW);
}

// ---- decoder cross-attention backward + mid chain in one launch per sequence (adt_seqxattn_tt.cuh) ----------------------------------------
// `at` and `ch` are the argument blocks of the two launches it stands for (adt_launch_seq_attn_bwd, adt_launch_seq_mid_bwd); the hand-over
// buffers at.dQ / dK / dV == ch.dqkv / dkv2 are neither written nor read.  Covered: the lean bf16 path with private weight-gradient partials,
// one workgroup per sequence, causal, H * hd = 64, L % 4 = 0, L <= 224, saved keep bits (or no dropout), LDS within the limit.
// ADT_XATTN_FUSED=0: never covered.
// Launches ISSUED by this process (eager steps, warm-up and the one capture of a graph), not replays of a captured graph: a debugging aid of
// the tests, not part of include/adt_hip.h.  Atomic: data-parallel trainers may step from several host threads.
static std::atomic<unsigned long long> g_xattn_fused_launches{0};
extern "C" unsigned long long adt_seq_xattn_fused_launches() { return g_xattn_fused_launches.load(); }

int adt_seq_xattn_mid_covered(int hd, const AttnArgs& at, const BwdChainArgs& ch) {
  const bool handover = ch.dqkv == at.dQ && ch.lddqkv == at.lddq && at.lddq == 64 && ch.dkv2 == at.dK && at.lddk == 128 && at.lddv == 128 &&
                        reinterpret_cast<const __bf16*>(at.dV) == reinterpret_cast<const __bf16*>(at.dK) + 64;
  return adt_covers_xattn_mid(adt_seq_switches(), hd, attn_facts(at), chain_facts(ch), handover);
}

int adt_launch_seq_xattn_mid_bwd(int hd, const AttnArgs& at, const BwdChainArgs& ch, void* stream) {
  if (!adt_seq_xattn_mid_covered(hd, at, ch)) return 1;
  XattnMidArgs a{};
  a.Q = reinterpret_cast<const __bf16*>(at.Q); a.K = reinterpret_cast<const __bf16*>(at.K); a.V = reinterpret_cast<const __bf16*>(at.V);
  a.O = reinterpret_cast<const __bf16*>(at.O); a.ldq = at.ldq; a.ldk = at.ldk; a.ldv = at.ldv; a.ldo = at.ldo;
  a.LSE = at.LSE; a.dO = at.dO; a.lddo = at.lddo; a.L = at.L; a.mask = at.mask; a.scale = at.scale; a.drop = at.drop;
  a.xin = ch.xin; a.o = ch.o; a.f = ch.f; a.wp_base = ch.wp_base; a.wp_img = ch.wp_img;
  a.W0 = ch.W0; a.W1 = ch.W1; a.W2 = ch.W2; a.W3 = ch.W3;
  a.out0 = ch.out0; a.out1 = ch.out1; a.acc1 = ch.acc1; a.nrep = ch.nrep; a.rep_stride = ch.rep_stride;
  a.db0 = ch.db0; a.db1 = ch.db1; a.db2 = ch.db2; a.db3 = ch.db3; a.vpart = ch.vpart;
  for (int k = 0; k < 4; ++k) a.part[k] = ch.part[k];
  a.part_stride = ch.part_stride;
  a.do_bf16 = ch.do_bf16; a.do_delta = ch.do_delta; a.do_scale = ch.do_scale;
  a.dO_bf16 = reinterpret_cast<const __bf16*>(at.do_bf16); a.dO_delta = at.do_delta;
  if (at.pad_pre && ch.pad_pre && at.pad_pre != ch.pad_pre) return adt_set_error("seqtt_xattn_mid_bwd: the two argument blocks name different pad prefixes");
  a.pad_pre = at.pad_pre ? at.pad_pre : ch.pad_pre;      // the queries' stack is the mid chain's: the decoder
  if (pad_refused(hd, a.pad_pre)) return -1;
  if (at.do_bf16 && !at.do_delta) return adt_set_error("seqtt_xattn_mid_bwd: handed-over dO rows without their delta");
  a.stamps = seq_stamp_buffer_mode(6);
  const int mode = at.drop.thr == 0 ? 0 : 1;
  static AdtLdsOptIn optin[6];
  const void* fns[6] = {(const void*)k_seqtt_xattn_mid_bwd<64, 0>, (const void*)k_seqtt_xattn_mid_bwd<64, 1>, (const void*)k_seqtt_xattn_mid_bwd<32, 0>,
                        (const void*)k_seqtt_xattn_mid_bwd<32, 1>, (const void*)k_seqtt_xattn_mid_bwd<16, 0>, (const void*)k_seqtt_xattn_mid_bwd<16, 1>};
  const int slot = (hd == 64 ? 0 : hd == 32 ? 2 : 4) + mode;
  // smem takes one of two values with L: opt in once (during warm-up, not under capture) to the larger one this head count admits
  const size_t most = xm_lds_bytes(ADT_SEQ_MAXLEN, at.H) <= ADT_LDS_MAX ? xm_lds_bytes(ADT_SEQ_MAXLEN, at.H) : xm_lds_bytes(128, at.H);
  const int rc = seq_launch(fns[slot], xm_lds_bytes(at.L, at.H), optin[slot], at.B, &a, (hipStream_t)stream, "seqtt_xattn_mid_bwd", XM_NW, most);
  if (rc == 0) ++g_xattn_fused_launches;
  if (rc == 0 && at.do_bf16) ++g_do_handover_launches;
  return pad_counted(rc, a.pad_pre);
}

// ---- sum of the per-workgroup weight-gradient partials (adt_seqbwd_tt.cuh: sb_dw_tiles) --------------------------------------------
// G[off[slot] + n * 64 + k] += sum_wg part[wg * stride + slot * 4096 + e], e = ((4 nt + kt) * 4 + r) * 64 + lane <-> n = 16 nt + 4 (lane >> 4) + r,
// k = 16 kt + (lane & 15).  grid (slots * 4, NSPLIT): a thread owns four consecutive elements (one float4 of the partial layout = four
// consecutive k of one row n) and a contiguous range of workgroups, summed in ascending order; the NSPLIT range sums meet in G by atomics.
struct PartReduceArgs {
  float* G; const float* part; size_t stride; int nwg; int nslots;
  int slot[256]; int off[256];      // slot index inside a workgroup's partial ; float offset of the 64 x 64 block in G
  int nwg_slot[256];                // workgroups that wrote this slot (kernels with several workgroups per sequence write B * S partials)
};
constexpr int PR_SPLIT = 4;
// bf16 partials (adt_seqbwd_tt.cuh: sb_dw_tiles): element (tile, lane, r) of a slot at (tile * 64 + lane) * 4 + r.  A thread owns 16
// consecutive elements (32 bytes: lanes l .. l + 3 of one tile, r = 0 .. 3 -> four rows n, four columns k) and a contiguous range of
// workgroups, summed in ascending order in fp32; the PR_SPLIT range sums meet in G by atomics.  grid (slots, PR_SPLIT), 256 threads.
__global__ __launch_bounds__(256) void k_dwpart_reduce(PartReduceArgs a) {
  typedef unsigned u4v __attribute__((ext_vector_type(4)));
  const int j = blockIdx.x, item = threadIdx.x;
  const int nwg = a.nwg_slot[j];
  const int per = (nwg + PR_SPLIT - 1) / PR_SPLIT, w0 = blockIdx.y * per, w1 = min(nwg, w0 + per);
  const __bf16* p = reinterpret_cast<const __bf16*>(a.part + (size_t)a.slot[j] * 4096) + item * 16;
  const size_t strideb = a.stride * 2;
  float sum[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) sum[i] = 0.f;
  int wg = w0;
  for (; wg + 4 <= w1; wg += 4) {
    u4v lo[4], hi[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const u4v* src = reinterpret_cast<const u4v*>(p + (size_t)(wg + u) * strideb);
      lo[u] = src[0]; hi[u] = src[1];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned wds[8] = {lo[u].x, lo[u].y, lo[u].z, lo[u].w, hi[u].x, hi[u].y, hi[u].z, hi[u].w};
#pragma unroll
      for (int i = 0; i < 8; ++i) { sum[2 * i] += __uint_as_float(wds[i] << 16); sum[2 * i + 1] += __uint_as_float(wds[i] & 0xFFFF0000u); }
    }
  }
  for (; wg < w1; ++wg) {
    const u4v* src = reinterpret_cast<const u4v*>(p + (size_t)wg * strideb);
    const u4v lo = src[0], hi = src[1];
    const unsigned wds[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) { sum[2 * i] += __uint_as_float(wds[i] << 16); sum[2 * i + 1] += __uint_as_float(wds[i] & 0xFFFF0000u); }
  }
  const int tile = item >> 4, lane0 = (item & 15) * 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float* dst = a.G + a.off[j] + (16 * (tile >> 2) + 4 * (lane0 >> 4) + r) * 64 + 16 * (tile & 3) + (lane0 & 15);
#pragma unroll
    for (int k = 0; k < 4; ++k) atomicAdd(dst + k, sum[4 * k + r]);
  }
}

int adt_dwpart_reduce(float* G, const float* part, size_t stride, int nwg, const int* slots, const int* offs, int nslots, void* stream) {
  return adt_dwpart_reduce_n(G, part, stride, nwg, nullptr, slots, offs, nslots, stream);
}
int adt_dwpart_reduce_n(float* G, const float* part, size_t stride, int nwg, const int* nwg_slot, const int* slots, const int* offs, int nslots, void* stream) {
  if (nslots < 1 || nslots > 256) return adt_set_error("dwpart_reduce: %d slots", nslots);
  PartReduceArgs a;
  a.G = G; a.part = part; a.stride = stride; a.nwg = nwg; a.nslots = nslots;
  for (int i = 0; i < nslots; ++i) { a.slot[i] = slots[i]; a.off[i] = offs[i]; a.nwg_slot[i] = nwg_slot ? nwg_slot[i] : nwg; }
  hipLaunchKernelGGL(k_dwpart_reduce, dim3(nslots, PR_SPLIT), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("dwpart_reduce");
}
