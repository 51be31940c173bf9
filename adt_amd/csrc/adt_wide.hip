// C ABI (include/adt_hip.h, "wide" section): launch wrappers for the general dense layers, the masked attention and
// the row kernels used by the BERT4Rec-ADT and STOSA-ADT paths.  Host code only enqueues work on the caller's stream.
#include <cstdlib>
#include "adt_host.h"

#include "adt_attn_gen.cuh"
#include "adt_attn_long_launch.h"
#include "adt_gemm.cuh"
#include "adt_dense_rows.cuh"
#include "adt_stosa.cuh"
#include "adt_klattn.cuh"
#include "adt_wattn_mfma.cuh"
#include "adt_lanes.cuh"
#include "adt_wide.cuh"

using namespace adt;

static_assert(PREC_F32 == ADT_PREC_F32 && PREC_BF16 == ADT_PREC_BF16, "adt_wide_plan.h speaks of the ABI's prec values");

// ---- masked attention: adt_attn_masked_plan (adt_wide_plan.h) chooses; these name the instantiation and pass its numbers -------------------
template <int PREC, int HD, int MAXKT, bool CSK = false>
static int launch_attn_gen(const AttnPlan& p, bool bwd, const AttnGenArgs& a, hipStream_t s) {
  constexpr int NWF = attn_resident_waves(PREC, HD, false), NWB = attn_resident_waves(PREC, HD, true);
  static_assert(attn_resident_lds(PREC, HD, MAXKT, false) == AttnGenLds<PREC, HD, MAXKT>::fwd_bytes, "plan and kernel disagree on the LDS footprint");
  static_assert(attn_resident_lds(PREC, HD, MAXKT, true) == AttnGenLds<PREC, HD, MAXKT>::bwd_bytes, "plan and kernel disagree on the LDS footprint");
  const void* fn = bwd ? (const void*)k_attn_gen_bwd<PREC, HD, MAXKT, NWB> : (const void*)k_attn_gen_fwd<PREC, HD, MAXKT, NWF, CSK>;
  static AdtLdsOptIn optin[2];
  return adt_launch_lds1(fn, dim3(a.a.B * a.a.H), dim3(p.waves * 64), p.lds_bytes, a, s, bwd ? "attn_masked_bwd" : "attn_masked_fwd", optin[bwd ? 1 : 0]);
}

// backward staged in NCH chunks of the sequence (k_attn_gen_bwd_chunked)
template <int PREC, int HD, int MAXKT, int NCH>
static int launch_attn_gen_bwd_chunked(const AttnPlan& p, const AttnGenArgs& a, hipStream_t s) {
  static_assert(attn_chunked_lds(PREC, HD, MAXKT, NCH) == AttnChunkLds<PREC, HD, MAXKT, NCH>::bwd_bytes, "plan and kernel disagree on the LDS footprint");
  // <PREC_F32, 128, 16, 2> (272 KB) is in the code object only: the plan streams that shape, and the host keeps no handle for what cannot be launched
  if (attn_chunked_lds(PREC, HD, MAXKT, NCH) > ADT_LDS_MAX) return adt_set_error("masked attention bwd: the chunked backward of this shape does not fit the LDS");
  static AdtLdsOptIn optin;
  return adt_launch_lds1((const void*)k_attn_gen_bwd_chunked<PREC, HD, MAXKT, NCH, ATTN_CHUNKED_NW>, dim3(a.a.B * a.a.H), dim3(p.waves * 64), p.lds_bytes, a, s,
                         "attn_masked_bwd(chunked)", optin);
}

// hd 16 / 32 / 64 by MAXKT; the chunked backward exists for exact fp32 at hd = 64 only
template <int PREC, int HD>
static int launch_attn_gen_l(const AttnPlan& p, bool bwd, const AttnGenArgs& a, hipStream_t s) {
  if (p.maxkt == 4) return launch_attn_gen<PREC, HD, 4>(p, bwd, a, s);
  if (p.maxkt == 8) return launch_attn_gen<PREC, HD, 8>(p, bwd, a, s);
  if constexpr (PREC == PREC_F32 && HD == 64) {
    if (p.family == ATTN_CHUNKED) return launch_attn_gen_bwd_chunked<PREC, HD, 16, 2>(p, a, s);
  }
  return launch_attn_gen<PREC, HD, 14>(p, bwd, a, s);
}

// key / query chunks streamed through LDS: the 256-row instantiations of adt_attn_long.cuh, grid (B*H, groups of NW 16-row tiles)
template <int PREC, int HD>
static int launch_attn_stream(const AttnPlan& p, bool bwd, const AttnGenArgs& a, hipStream_t s) {
  return launch_attn_long<PREC, HD, ATTN_STREAMED_LMAX>(p, bwd, a, s, "attn_masked_fwd(streamed)", "attn_masked_bwd(streamed)");
}

// hd = 128: streamed (exact fp32 only), resident forward with or without the causal tile skip, chunked backward
template <int PREC, int MAXKT, int NCH>
static int launch_attn_gen_128(const AttnPlan& p, bool bwd, const AttnGenArgs& a, hipStream_t s) {
  constexpr int HD = 128;
  if constexpr (PREC == PREC_F32) {
    if (p.family == ATTN_STREAMED) return launch_attn_stream<PREC, HD>(p, bwd, a, s);
  }
  if (p.family == ATTN_RESIDENT) return p.csk ? launch_attn_gen<PREC, HD, MAXKT, true>(p, false, a, s) : launch_attn_gen<PREC, HD, MAXKT, false>(p, false, a, s);
  return launch_attn_gen_bwd_chunked<PREC, HD, MAXKT, NCH>(p, a, s);
}

template <int PREC>
static int launch_attn(const AttnPlan& p, bool bwd, int hd, const AttnGenArgs& a, hipStream_t s) {
  if (hd == 16) return launch_attn_gen_l<PREC, 16>(p, bwd, a, s);
  if (hd == 32) return launch_attn_gen_l<PREC, 32>(p, bwd, a, s);
  if (hd == 64) return launch_attn_gen_l<PREC, 64>(p, bwd, a, s);
  if (hd == 128) return p.maxkt == 4 ? launch_attn_gen_128<PREC, 4, 1>(p, bwd, a, s) : launch_attn_gen_128<PREC, 16, 2>(p, bwd, a, s);
  return launch_attn_stream<PREC, 256>(p, bwd, a, s);
}

// ---- row-streaming kernels (adt_dense_rows.cuh): bf16 operands, contraction 64 / 128 / 256 ---------------------------------------
template <class Args>
static int rows_launch(const void* kernel, const Args& a, int n_panels, int pc, int row_groups, size_t smem, hipStream_t s, const char* what, AdtLdsOptIn& optin) {
  void* kargs[] = {const_cast<Args*>(&a), &n_panels, &pc};      // smem grows with the run-time panel width: the high-water mark in optin follows it
  return adt_launch_lds(kernel, dim3(row_groups * n_panels), dim3(ROWS_NW * 64), smem, kargs, s, what, optin);
}

static int launch_dense_fwd_rows(const DenseFwdPlan& p, const DenseFwdArgs& a, hipStream_t s) {
  static const void* const fns[6] = {(const void*)k_dense_fwd_rows<2, 4>, (const void*)k_dense_fwd_rows<4, 4>, (const void*)k_dense_fwd_rows<8, 4>,
                                     (const void*)k_dense_fwd_rows<2, 8>, (const void*)k_dense_fwd_rows<4, 8>, (const void*)k_dense_fwd_rows<8, 8>};
  static AdtLdsOptIn optin[6];
  const int i = (p.ch == 4 ? 0 : 3) + (p.kb == 2 ? 0 : (p.kb == 4 ? 1 : 2));      // k_dense_fwd_rows<KB, CH>
  return rows_launch(fns[i], a, p.n_panels, p.pc, p.row_groups, p.lds_bytes, s, "dense_fwd(rows)", optin[i]);
}

// one launch per contraction piece: its columns of G and U, its rows of W, the layer's own dropout indices; dX only
static int launch_dense_dx_rows(const DenseBwdPlan& p, const DenseBwdArgs& a0, hipStream_t s) {
  static const void* const fns[5] = {(const void*)k_dense_dx_rows<2, true>, (const void*)k_dense_dx_rows<4, true>, (const void*)k_dense_dx_rows<2, false>,
                                     (const void*)k_dense_dx_rows<4, false>, (const void*)k_dense_dx_rows<8, false>};
  static AdtLdsOptIn optin[5];
  for (int i = 0; i < p.n_pieces; ++i) {
    const DxPiece& pc = p.piece[i];
    DenseBwdArgs a = a0;
    a.G.dY = a0.G.dY + pc.n0; a.G.U = a0.G.U ? a0.G.U + pc.n0 : nullptr; a.G.N = pc.chunk; a.G.idx_off = a0.G.idx_off + pc.n0;
    a.W = a0.W + (size_t)pc.n0 * a0.ldw;
    a.beta = i ? pc.beta : a0.beta;      // the first piece keeps the caller's word
    a.dW = nullptr; a.db = nullptr;
    const int k = p.has_u ? (pc.kb == 2 ? 0 : 1) : (pc.kb == 2 ? 2 : (pc.kb == 4 ? 3 : 4));      // k_dense_dx_rows<KB, has_u>
    if (rows_launch(fns[k], a, p.n_panels, p.pc, pc.row_groups, pc.lds_bytes, s, "dense_bwd_dx(rows)", optin[k])) return -1;
  }
  return 0;
}

// ---- STOSA-ADT attention (adt_stosa.cuh, adt_klattn.cuh, adt_wattn_mfma.cuh) ------------------------------------------------------------
// Ahead of the dense entry points on purpose: kernel templates land in the code object in the order the host code first uses them, and
// tools/device_asm.sh compares that byte for byte.

// One argument block for every STOSA attention entry point (adt_stosa.cuh: WAttnArgs), forward ...
static WAttnArgs make_wattn_args(const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                                 const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float p,
                                 const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc, float* LSE) {
  WAttnArgs a{};
  a.Qm = Qm; a.ldqm = ldqm; a.Qc = Qc; a.ldqc = ldqc; a.Km = Km; a.ldkm = ldkm; a.Kc = Kc; a.ldkc = ldkc; a.Vm = Vm; a.ldvm = ldvm;
  a.Vc = Vc; a.ldvc = ldvc; a.kid = key_ids; a.B = B; a.H = H; a.L = L; a.hd = hd; a.scale = 1.0f / sqrtf((float)hd);
  a.drop = adt_make_drop(p, seed, site); a.bh_offset = b_offset * (uint32_t)H; a.Om = Om; a.ldom = ldom; a.Oc = Oc; a.ldoc = ldoc; a.LSE = LSE;
  return a;
}

// ... and backward: the forward's block (its outputs now inputs) plus the output gradients and the six input gradients
static WAttnArgs make_wattn_args_bwd(const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                                     const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, const float* Om, int ldom,
                                     const float* Oc, int ldoc, const float* LSE, const float* dOm, int lddom, const float* dOc, int lddoc, int B, int H,
                                     int L, int hd, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQm, float* dQc, float* dKm,
                                     float* dKc, float* dVm, float* dVc, int ldd) {
  WAttnArgs a = make_wattn_args(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, p, seed, site, b_offset,
                                const_cast<float*>(Om), ldom, const_cast<float*>(Oc), ldoc, const_cast<float*>(LSE));
  a.dOm = dOm; a.lddom = lddom; a.dOc = dOc; a.lddoc = lddoc;
  a.dQm = dQm; a.dQc = dQc; a.dKm = dKm; a.dKc = dKc; a.dVm = dVm; a.dVc = dVc; a.ldd = ldd;
  return a;
}

// Both metrics of the vector-ALU STOSA attention share this launcher (adt_stosa.cuh: Wasserstein, adt_klattn.cuh: KL divergence;
// the same shapes, arguments and LDS footprint)
template <int MET>
static int stosa_attn(bool bwd, const WAttnArgs& a, void* stream) {
  const char* nm = wm_kl(MET) ? "klattn" : "wattn";
  if (a.hd != 16 && a.hd != 32 && a.hd != 64) return adt_set_error("%s: head_dim=%d unsupported (16/32/64)", nm, a.hd);
  if (a.L > 256) return adt_set_error("%s: L=%d > 256 unsupported", nm, a.L);
  const void* fn = MET == WM_KLP ? (bwd ? (const void*)k_klattn_bwd<true> : (const void*)k_klattn_fwd<true>)
                   : MET == WM_KL ? (bwd ? (const void*)k_klattn_bwd<false> : (const void*)k_klattn_fwd<false>)
                                  : (bwd ? (const void*)k_wattn_bwd : (const void*)k_wattn_fwd);
  const char* what = wm_kl(MET) ? (bwd ? "klattn_bwd" : "klattn_fwd") : (bwd ? "wattn_bwd" : "wattn_fwd");
  static AdtLdsOptIn optin[2];
  return adt_launch_lds1(fn, dim3(a.B * a.H), dim3(256), wattn_lds_bytes(a.L, a.hd, bwd), a, (hipStream_t)stream, what, optin[bwd], ADT_LDS_MAX);
}

// The same attention on the matrix cores (adt_wattn_mfma.cuh): hd 16 or 32, L <= 128; prec picks bf16 operands or the exact fp32 MFMA.
static bool wattn_mfma_ok(const WAttnArgs& a) {
  static const int on = adt_env_on("ADT_WATTN_MFMA");
  if (!on || (a.hd != 16 && a.hd != 32) || a.L > 128) return false;
  const int lds[11] = {a.ldqm, a.ldqc, a.ldkm, a.ldkc, a.ldvm, a.ldvc, a.ldom, a.ldoc, a.lddom, a.lddoc, a.ldd};      // the last three: 0 in a forward
  for (int ld : lds)
    if (ld % 4) return false;
  return true;
}

template <int PREC, int HD, int MET>
static int wattn_mfma_launch(bool bwd, const WAttnArgs& a, hipStream_t s) {
  const void* fn = bwd ? (const void*)k_wattn_mfma_bwd<PREC, HD, MET> : (const void*)k_wattn_mfma_fwd<PREC, HD, 8, MET>;
  const size_t smem = wattn_mfma_lds_bytes(a.L, HD, bwd);
  if (smem > ADT_LDS_MAX) return 1;
  static AdtLdsOptIn optin[2];
  return adt_launch_lds1(fn, dim3(a.B * a.H), dim3(WM_NW * 64), smem, a, s, bwd ? "wattn_mfma_bwd" : "wattn_mfma_fwd", optin[bwd], ADT_LDS_MAX);
}

// MET = WM_W: the Wasserstein score; WM_KL: the KL-divergence score on the same kernels, shapes and LDS; WM_KLP: the KL score on padded
// heads (the adt_klattn_*_scaled_* entry points: hd_live live lanes, the pad lanes gated by selects).
// Returns 1 when the shape is not covered (the caller uses the vector-ALU entry point).
template <int MET>
static int wattn_mfma_dispatch(int prec, bool bwd, const WAttnArgs& a, hipStream_t s) {
  if (!wattn_mfma_ok(a)) return 1;
  if (prec == ADT_PREC_BF16) return a.hd == 16 ? wattn_mfma_launch<PREC_BF16, 16, MET>(bwd, a, s) : wattn_mfma_launch<PREC_BF16, 32, MET>(bwd, a, s);
  return a.hd == 16 ? wattn_mfma_launch<PREC_F32, 16, MET>(bwd, a, s) : wattn_mfma_launch<PREC_F32, 32, MET>(bwd, a, s);
}

// The entry points below differ in the metric (wattn: Wasserstein, klattn: KL divergence; the same shapes, arguments and LDS footprint) and
// in the unit: adt_*_fwd / adt_*_bwd run on the vector ALU, adt_*_mfma_* on the matrix cores (1 = shape not covered).
extern "C" {

int adt_wattn_fwd(const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                  const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float p,
                  const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc, float* LSE,
                  void* stream) {
  return stosa_attn<WM_W>(false, make_wattn_args(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, p, seed, site, b_offset, Om, ldom, Oc, ldoc, LSE), stream);
}

int adt_wattn_bwd(const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                  const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, const float* Om, int ldom, const float* Oc,
                  int ldoc, const float* LSE, const float* dOm, int lddom, const float* dOc, int lddoc, int B, int H, int L, int hd, float p,
                  const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQm, float* dQc, float* dKm, float* dKc, float* dVm,
                  float* dVc, int ldd, void* stream) {
  return stosa_attn<WM_W>(true, make_wattn_args_bwd(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, Om, ldom, Oc, ldoc, LSE, dOm, lddom, dOc, lddoc,
                                                    B, H, L, hd, p, seed, site, b_offset, dQm, dQc, dKm, dKc, dVm, dVc, ldd), stream);
}

int adt_wattn_mfma_fwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                       const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float p,
                       const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc, float* LSE,
                       void* stream) {
  return wattn_mfma_dispatch<WM_W>(prec, false, make_wattn_args(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, p, seed, site, b_offset, Om, ldom, Oc, ldoc, LSE), (hipStream_t)stream);
}

int adt_wattn_mfma_bwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                       const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, const float* Om, int ldom, const float* Oc,
                       int ldoc, const float* LSE, const float* dOm, int lddom, const float* dOc, int lddoc, int B, int H, int L, int hd, float p,
                       const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQm, float* dQc, float* dKm, float* dKc, float* dVm,
                       float* dVc, int ldd, void* stream) {
  return wattn_mfma_dispatch<WM_W>(prec, true, make_wattn_args_bwd(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, Om, ldom, Oc, ldoc, LSE, dOm, lddom, dOc, lddoc,
                                                                   B, H, L, hd, p, seed, site, b_offset, dQm, dQc, dKm, dKc, dVm, dVc, ldd), (hipStream_t)stream);
}

int adt_klattn_fwd(const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                   const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float p,
                   const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc, float* LSE,
                   void* stream) {
  return stosa_attn<WM_KL>(false, make_wattn_args(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, p, seed, site, b_offset, Om, ldom, Oc, ldoc, LSE), stream);
}

int adt_klattn_bwd(const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                   const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, const float* Om, int ldom, const float* Oc,
                   int ldoc, const float* LSE, const float* dOm, int lddom, const float* dOc, int lddoc, int B, int H, int L, int hd, float p,
                   const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQm, float* dQc, float* dKm, float* dKc, float* dVm,
                   float* dVc, int ldd, void* stream) {
  return stosa_attn<WM_KL>(true, make_wattn_args_bwd(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, Om, ldom, Oc, ldoc, LSE, dOm, lddom, dOc, lddoc,
                                                     B, H, L, hd, p, seed, site, b_offset, dQm, dQc, dKm, dKc, dVm, dVc, ldd), stream);
}

int adt_klattn_mfma_fwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                        const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float p,
                        const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc, float* LSE,
                        void* stream) {
  return wattn_mfma_dispatch<WM_KL>(prec, false, make_wattn_args(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, p, seed, site, b_offset, Om, ldom, Oc, ldoc, LSE), (hipStream_t)stream);
}

int adt_klattn_mfma_bwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                        const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, const float* Om, int ldom, const float* Oc,
                        int ldoc, const float* LSE, const float* dOm, int lddom, const float* dOc, int lddoc, int B, int H, int L, int hd, float p,
                        const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQm, float* dQc, float* dKm, float* dKc, float* dVm,
                        float* dVc, int ldd, void* stream) {
  return wattn_mfma_dispatch<WM_KL>(prec, true, make_wattn_args_bwd(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, Om, ldom, Oc, ldoc, LSE, dOm, lddom, dOc, lddoc,
                                                                    B, H, L, hd, p, seed, site, b_offset, dQm, dQc, dKm, dKc, dVm, dVc, ldd), (hipStream_t)stream);
}

}  // extern "C"

// ---- dense layers: adt_dense_fwd_plan / adt_dense_bwd_plan (adt_wide_plan.h) choose the kernel and its numbers; the launchers pass them -----
// Below the STOSA entry points, each entry point behind its launchers, for the same reason: the order of first use.
static float* g_dense_ws = nullptr;      // scratch registered by the host (adt_dense_workspace): private partials of the 256 x 256 weight gradients
static int64_t g_dense_ws_bytes = 0;
static int g_rows_enabled = 1;      // adt_dense_rows_enable(0) routes everything to the tiled kernels (A/B measurements, tests)
// ADT_STAGE256=0 in the environment keeps the 256-wide forward / input-gradient stage kernels (k_dense_fwd256, k_dense_dx256) off: A/B runs
static bool stage_kernels_on() {
  static const int on = adt_env_on("ADT_STAGE256");
  return on != 0;
}

// what the vectorised kernels ask of an operand: a 16-byte aligned base and a row stride that is a multiple of 4 floats
static bool operand_ok(const void* p, int ld) { return (ld % 4) == 0 && adt_aligned16(p); }

static DenseFacts dense_facts(int prec, int T, int K, int N) {
  DenseFacts f{};
  f.prec = prec; f.T = T; f.K = K; f.N = N;
  f.rows_on = g_rows_enabled != 0; f.stage256_on = stage_kernels_on(); f.ws_bytes = g_dense_ws ? g_dense_ws_bytes : 0;
  return f;
}

static DenseFacts dense_fwd_facts(int prec, const DenseFwdArgs& a) {
  DenseFacts f = dense_facts(prec, a.T, a.K, a.N);
  f.has_bias = a.b != nullptr; f.has_u = a.U != nullptr; f.has_r = a.R != nullptr; f.has_r2 = a.R2 != nullptr; f.has_mask = a.ids != nullptr;
  f.has_drop = a.drop.thr != 0; f.has_act = a.act != ACT_NONE;
  f.x_ok = operand_ok(a.X, a.ldx); f.w_ok = operand_ok(a.W, a.ldw); f.g_ok = operand_ok(a.Y, a.ldy); f.bias_ok = adt_aligned16(a.b);
  f.u_ok = operand_ok(a.U, a.ldu); f.r_ok = operand_ok(a.R, a.ldr); f.r2_ok = operand_ok(a.R2, a.ldr2);
  return f;
}

static DenseFacts dense_bwd_facts(int prec, const DenseBwdArgs& a) {
  DenseFacts f = dense_facts(prec, a.G.T, a.K, a.G.N);
  f.has_u = a.G.U != nullptr; f.has_mask = a.G.ids != nullptr; f.has_drop = a.G.drop.thr != 0; f.has_act = a.G.act != ACT_NONE;
  f.has_dx = a.dX != nullptr; f.has_dw = a.dW != nullptr; f.beta = a.beta != 0;
  f.x_ok = operand_ok(a.X, a.ldx); f.w_ok = operand_ok(a.W, a.ldw); f.g_ok = operand_ok(a.G.dY, a.G.lddy); f.u_ok = operand_ok(a.G.U, a.G.ldu);
  f.dx_ok = operand_ok(a.dX, a.lddx);
  return f;
}

static int launch_dense_fwd256(const DenseFwdPlan& p, const DenseFwdArgs& a, hipStream_t s) {
  static const void* const fns[8] = {(const void*)k_dense_fwd256<0>, (const void*)k_dense_fwd256<1>, (const void*)k_dense_fwd256<2>, (const void*)k_dense_fwd256<3>,
                                     (const void*)k_dense_fwd256<4>, (const void*)k_dense_fwd256<5>, (const void*)k_dense_fwd256<6>, (const void*)k_dense_fwd256<7>};
  static AdtLdsOptIn none;      // static LDS only
  int chunk = p.chunk;
  void* kargs[] = {const_cast<DenseFwdArgs*>(&a), &chunk};
  return adt_launch_lds(fns[p.epi], dim3(p.grid_x, p.grid_y), dim3(p.block), 0, kargs, s, "dense_fwd(256)", none);
}

template <int PREC>
static int launch_dense_fwd(const DenseFwdPlan& p, const DenseFwdArgs& a0, hipStream_t s) {
  static_assert(gemm_tile_lds_bytes(PREC == PREC_BF16, 128) == gemm_lds_bytes<PREC, 128>() && gemm_tile_lds_bytes(PREC == PREC_BF16, 64) == gemm_lds_bytes<PREC, 64>(),
                "plan and kernel disagree on the LDS footprint");
  if (p.arm == F256) return launch_dense_fwd256(p, a0, s);
  if (p.arm == FROWS) return launch_dense_fwd_rows(p, a0, s);
  DenseFwdArgs a = a0;
  a.nt_n = p.nt_n; a.nt_m = p.nt_m;
  static AdtLdsOptIn optin[2];
  if (p.bn == 128) return adt_launch_lds1((const void*)k_dense_fwd<PREC, 128>, dim3(p.grid_x), dim3(p.block), p.lds_bytes, a, s, "dense_fwd", optin[0]);
  return adt_launch_lds1((const void*)k_dense_fwd<PREC, 64>, dim3(p.grid_x), dim3(p.block), p.lds_bytes, a, s, "dense_fwd", optin[1]);
}

extern "C" {

int adt_dense_workspace(void* ws, int64_t bytes) {
  g_dense_ws = static_cast<float*>(ws);
  g_dense_ws_bytes = ws ? bytes : 0;
  return 0;
}

int adt_dense_rows_enable(int on) {
  const int was = g_rows_enabled;
  g_rows_enabled = on ? 1 : 0;
  return was;
}

int64_t adt_dense_bwd_ws_bytes(int prec, int T, int K, int N) { return adt_dense_bwd_ws_need(prec, T, K, N); }

int adt_dense_fwd(int prec, const float* X, int ldx, const float* W, int ldw, const float* b, int T, int K, int N, int act, float* U,
                  int ldu, float p, const uint32_t* seed, uint32_t site, uint32_t row_offset, const float* R, int ldr,
                  const float* R2, int ldr2, const int32_t* mask_ids, float* Y, int ldy, const int32_t* t_dev, void* stream) {
  if (T <= 0 || K <= 0 || N <= 0) return adt_set_error("dense_fwd: empty shape");
  if ((ldx % 4) || (ldw % 4) || !adt_aligned16(X) || !adt_aligned16(W)) return adt_set_error("dense_fwd: operands must be 16-byte aligned with ld %% 4 == 0");
  if (act < 0 || act > ACT_ELU1) return adt_set_error("dense_fwd: act=%d", act);
  DenseFwdArgs a{};
  a.X = X; a.ldx = ldx; a.W = W; a.ldw = ldw; a.b = b; a.T = T; a.K = K; a.N = N; a.Y = Y; a.ldy = ldy; a.U = U; a.ldu = ldu; a.act = act;
  a.drop = adt_make_drop(p, seed, site); a.row_offset = row_offset; a.R = R; a.ldr = ldr; a.R2 = R2; a.ldr2 = ldr2; a.ids = mask_ids; a.t_dev = t_dev;
  const DenseFwdPlan plan = adt_dense_fwd_plan(dense_fwd_facts(prec, a));
  return prec == ADT_PREC_F32 ? launch_dense_fwd<PREC_F32>(plan, a, (hipStream_t)stream) : launch_dense_fwd<PREC_BF16>(plan, a, (hipStream_t)stream);
}

}  // extern "C"

static void launch_dense_dx256(const DenseBwdPlan& p, const DenseBwdArgs& a0, hipStream_t s) {
  DenseBwdArgs a = a0;
  a.t_chunk = p.dx_chunk;
  const dim3 grid(p.dx_grid_x, p.dx_grid_y), block(p.dx_block);
  if (p.nb == 1) hipLaunchKernelGGL(k_dense_dx256<1>, grid, block, p.dx_lds_bytes, s, a);
  else if (p.nb == 2) hipLaunchKernelGGL(k_dense_dx256<2>, grid, block, p.dx_lds_bytes, s, a);
  else hipLaunchKernelGGL(k_dense_dx256<3>, grid, block, p.dx_lds_bytes, s, a);
}

// the tiled dX kernel's block: its tile counts and the split of N
static DenseBwdArgs dense_dx_tiled_args(const DenseBwdPlan& p, const DenseBwdArgs& a0) {
  DenseBwdArgs a = a0;
  a.n_chunk = p.n_chunk; a.nt_a = p.gx; a.nt_b = p.gy; a.nt_z = p.dx_splits;
  return a;
}

template <int PREC>
static int launch_dense_dx_tiled(const DenseBwdPlan& p, const DenseBwdArgs& a, hipStream_t s) {
  // The splits add their partials with atomics in no order, so none of them can do the clearing: a launch ahead of them does, and it stops at
  // *t_dev like every other arm (rows at or beyond it stay untouched, DenseFwdArgs::t_dev).
  if (p.dx_zero_fill && adt::zero_rows_f32_async(a.dX, (size_t)a.lddx, a.K, (size_t)a.G.T, s, a.t_dev)) return adt_set_error("dense_bwd: zero");
  static AdtLdsOptIn optin[2];
  if (p.dx_bn == 128) return adt_launch_lds1((const void*)k_dense_bwd_dx<PREC, 128>, dim3(p.dx_grid_x), dim3(p.dx_block), p.dx_lds_bytes, a, s, "dense_bwd_dx", optin[0]);
  return adt_launch_lds1((const void*)k_dense_bwd_dx<PREC, 64>, dim3(p.dx_grid_x), dim3(p.dx_block), p.dx_lds_bytes, a, s, "dense_bwd_dx", optin[1]);
}

static void launch_dense_dw256(const DenseBwdPlan& p, const DenseBwdArgs& a0, hipStream_t s) {
  DenseBwdArgs a = a0;
  a.t_chunk = p.dw_chunk;
  hipLaunchKernelGGL(k_dense_dw256, dim3(p.dw_grid_x, p.dw_grid_y), dim3(p.dw_block), 0, s, a, g_dense_ws);
  hipLaunchKernelGGL(k_dense_dw256_reduce, dim3(64, p.reduce_groups, p.blocks), dim3(256), 0, s, (const float*)g_dense_ws, p.nwg, p.per, a.dW, a.lddw, p.kblocks);
}

static int launch_dense_dw_rows(const DenseBwdPlan& p, const DenseBwdArgs& a0, hipStream_t s) {
  DenseBwdArgs a = a0;
  a.t_chunk = p.dw_chunk; a.nt_z = p.dw_splits;
  int nb = p.n_blocks, kb = p.k_blocks;
  void* kargs[] = {&a, &nb, &kb};
  static AdtLdsOptIn optin;
  return adt_launch_lds((const void*)k_dense_dw_rows, dim3(p.dw_grid_x), dim3(p.dw_block), p.dw_lds_bytes, kargs, s, "dense_bwd_dw(rows)", optin);
}

static void launch_dense_dw64(const DenseBwdPlan& p, const DenseBwdArgs& a0, hipStream_t s) {
  DenseBwdArgs a = a0;
  a.t_chunk = p.dw_chunk;
  float* const part = p.partials ? g_dense_ws : nullptr;
  hipLaunchKernelGGL(k_dense_dw64, dim3(p.dw_grid_x, p.dw_grid_y), dim3(p.dw_block), 0, s, a, part);
  if (part)
    hipLaunchKernelGGL(k_dense_dw64_reduce, dim3(17, p.blocks), dim3(1024), 0, s, (const float*)part, p.nwg, a.t_dev, a.G.T, p.dw_chunk, a.dW, a.lddw, p.kblocks, a.db);
}

template <int PREC>
static int launch_dense_dw_tiled(const DenseBwdPlan& p, const DenseBwdArgs& a0, hipStream_t s) {
  DenseBwdArgs a = a0;
  a.t_chunk = p.dw_chunk; a.nt_a = p.dw_gx; a.nt_b = p.dw_gy; a.nt_z = p.dw_splits;
  static AdtLdsOptIn optin[2];
  if (p.dw_bn == 128) return adt_launch_lds1((const void*)k_dense_bwd_dw<PREC, 128>, dim3(p.dw_grid_x), dim3(p.dw_block), p.dw_lds_bytes, a, s, "dense_bwd_dw", optin[0]);
  return adt_launch_lds1((const void*)k_dense_bwd_dw<PREC, 64>, dim3(p.dw_grid_x), dim3(p.dw_block), p.dw_lds_bytes, a, s, "dense_bwd_dw", optin[1]);
}

template <int PREC>
static int launch_dense_bwd(const DenseBwdPlan& p, const DenseBwdArgs& a0, hipStream_t s) {
  // The dW kernels' block.  They read neither dX nor the dX kernel's tile counts; both stay in it as those kernels have always received them.
  DenseBwdArgs w = a0;
  switch (p.dx) {
    case DX256: launch_dense_dx256(p, a0, s); w.dX = nullptr; break;
    case DXROWS: if (launch_dense_dx_rows(p, a0, s)) return -1; w.dX = nullptr; break;
    case DXTILED: w = dense_dx_tiled_args(p, a0); if (launch_dense_dx_tiled<PREC>(p, w, s)) return -1; break;
    case DXNONE: break;
  }
  switch (p.dw) {
    case DW256: launch_dense_dw256(p, w, s); break;
    case DWROWS: if (launch_dense_dw_rows(p, w, s)) return -1; break;
    case DW64: launch_dense_dw64(p, w, s); break;
    case DWTILED: if (launch_dense_dw_tiled<PREC>(p, w, s)) return -1; break;
    case DWNONE: break;
  }
  return adt_check_launch("dense_bwd");
}

extern "C" {

int adt_dense_bwd(int prec, const float* dY, int lddy, int T, int K, int N, const int32_t* mask_ids, float p, const uint32_t* seed,
                  uint32_t site, uint32_t row_offset, int act, const float* U, int ldu, const float* X, int ldx, const float* W, int ldw,
                  float* dX, int lddx, int beta, float* dW, int lddw, float* db, const int32_t* t_dev, void* stream) {
  if (T <= 0 || K <= 0 || N <= 0) return adt_set_error("dense_bwd: empty shape");
  if ((lddy % 4) || !adt_aligned16(dY) || (dW && ((ldx % 4) || !adt_aligned16(X))) || (dX && ((ldw % 4) || !adt_aligned16(W))))
    return adt_set_error("dense_bwd: operands must be 16-byte aligned with ld %% 4 == 0");
  if (act != ACT_NONE && !U) return adt_set_error("dense_bwd: activation gradient needs the saved pre-activation U");
  DenseBwdArgs a{};
  a.G.dY = dY; a.G.lddy = lddy; a.G.T = T; a.G.N = N; a.G.U = U; a.G.ldu = ldu; a.G.act = act;
  a.G.drop = adt_make_drop(p, seed, site); a.G.row_offset = row_offset; a.G.ids = mask_ids; a.G.idx_ld = N; a.G.idx_off = 0;
  a.X = X; a.ldx = ldx; a.W = W; a.ldw = ldw; a.K = K; a.dX = dX; a.lddx = lddx; a.beta = beta; a.dW = dW; a.lddw = lddw; a.db = db; a.t_dev = t_dev;
  const DenseBwdPlan plan = adt_dense_bwd_plan(dense_bwd_facts(prec, a));
  return prec == ADT_PREC_F32 ? launch_dense_bwd<PREC_F32>(plan, a, (hipStream_t)stream) : launch_dense_bwd<PREC_BF16>(plan, a, (hipStream_t)stream);
}

static int fill_attn(AttnGenArgs& g, const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, int B, int H, int L, int hd,
                     int causal, const int32_t* kid, float fill, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset) {
  if ((ldq % 4) || (ldk % 4) || (ldv % 4) || (hd % 8)) return adt_set_error("masked attention: ld %% 4, hd %% 8");
  g.a.Q = Q; g.a.ldq = ldq; g.a.K = K; g.a.ldk = ldk; g.a.V = V; g.a.ldv = ldv; g.a.B = B; g.a.H = H; g.a.L = L; g.a.causal = causal;
  g.a.scale = 1.0f / sqrtf((float)hd); g.a.drop = adt_make_drop(p, seed, site); g.a.bh_offset = b_offset * (uint32_t)H;
  g.kid = kid; g.fill = fill;
  return 0;
}

// adt_attn_masked_plan (adt_wide_plan.h) chooses, launch_attn names the instantiation
static int attn_masked_launch(int prec, bool bwd, int hd, const AttnGenArgs& g, void* stream) {
  const AttnPlan p = adt_attn_masked_plan(prec, hd, g.a.L, bwd, g.a.causal != 0, g.kid != nullptr, g.fill);
  if (p.error[0]) return adt_set_error("%s", p.error);
  return prec == ADT_PREC_F32 ? launch_attn<PREC_F32>(p, bwd, hd, g, (hipStream_t)stream) : launch_attn<PREC_BF16>(p, bwd, hd, g, (hipStream_t)stream);
}

// scale <= 0: the kernels' own 1 / sqrt(hd) (fill_attn); else the caller's score scale (heads padded with zero lanes)
static int attn_masked_fwd_impl(int prec, const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, int B, int H, int L, int hd,
                                float scale, int causal, const int32_t* key_ids, float fill, float p, const uint32_t* seed, uint32_t site,
                                uint32_t b_offset, float* O, int ldo, float* LSE, void* stream) {
  AttnGenArgs g{};
  if (fill_attn(g, Q, ldq, K, ldk, V, ldv, B, H, L, hd, causal, key_ids, fill, p, seed, site, b_offset)) return -1;
  if (scale > 0.f) g.a.scale = scale;
  g.a.O = O; g.a.ldo = ldo; g.a.LSE = LSE;
  return attn_masked_launch(prec, false, hd, g, stream);
}

static int attn_masked_bwd_impl(int prec, const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, const float* O, int ldo,
                                const float* LSE, const float* dO, int lddo, int B, int H, int L, int hd, float scale, int causal,
                                const int32_t* key_ids, float fill, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQ,
                                int lddq, float* dK, int lddk, float* dV, int lddv, void* stream) {
  AttnGenArgs g{};
  if (fill_attn(g, Q, ldq, K, ldk, V, ldv, B, H, L, hd, causal, key_ids, fill, p, seed, site, b_offset)) return -1;
  if ((ldo % 4) || (lddo % 4) || (lddq % 4) || (lddk % 4) || (lddv % 4)) return adt_set_error("masked attention bwd: ld %% 4");
  if (scale > 0.f) g.a.scale = scale;
  g.a.O = const_cast<float*>(O); g.a.ldo = ldo; g.a.LSE = const_cast<float*>(LSE); g.a.dO = dO; g.a.lddo = lddo;
  g.a.dQ = dQ; g.a.lddq = lddq; g.a.dK = dK; g.a.lddk = lddk; g.a.dV = dV; g.a.lddv = lddv;
  return attn_masked_launch(prec, true, hd, g, stream);
}

int adt_attn_masked_fwd(int prec, const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, int B, int H, int L, int hd,
                        int causal, const int32_t* key_ids, float fill, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset,
                        float* O, int ldo, float* LSE, void* stream) {
  return attn_masked_fwd_impl(prec, Q, ldq, K, ldk, V, ldv, B, H, L, hd, 0.f, causal, key_ids, fill, p, seed, site, b_offset, O, ldo, LSE, stream);
}

int adt_attn_masked_bwd(int prec, const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, const float* O, int ldo,
                        const float* LSE, const float* dO, int lddo, int B, int H, int L, int hd, int causal, const int32_t* key_ids,
                        float fill, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQ, int lddq, float* dK,
                        int lddk, float* dV, int lddv, void* stream) {
  return attn_masked_bwd_impl(prec, Q, ldq, K, ldk, V, ldv, O, ldo, LSE, dO, lddo, B, H, L, hd, 0.f, causal, key_ids, fill, p, seed, site, b_offset,
                              dQ, lddq, dK, lddk, dV, lddv, stream);
}

int adt_embed_sum_fwd(const int32_t* ids, const float* E, const float* P, const float* S0, float scale, int T, int L, int d, float* X,
                      void* stream) {
  if (d % 4) return adt_set_error("embed_sum_fwd: d %% 4");
  EmbedSumArgs a{ids, E, P, S0, scale, T, L, d, X};
  hipLaunchKernelGGL(k_embed_sum_fwd, dim3(adt_grid_for((size_t)T * d / 4, 256, 2048)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("embed_sum_fwd");
}

int adt_dropact_fwd(const float* X, int64_t n, float p, const uint32_t* seed, uint32_t site, uint32_t idx_offset, int act, float* Y,
                    void* stream) {
  if (n % 4) return adt_set_error("dropact_fwd: n %% 4");
  DropActArgs a{};
  a.X = X; a.Y = Y; a.n = (size_t)n; a.drop = adt_make_drop(p, seed, site); a.idx_offset = idx_offset; a.act = act;
  hipLaunchKernelGGL(k_dropact<false>, dim3(adt_grid_for((size_t)n / 4, 256, 2048)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("dropact_fwd");
}

int adt_dropact_bwd(const float* dY, const float* X, int64_t n, float p, const uint32_t* seed, uint32_t site, uint32_t idx_offset, int act,
                    float* dX, int accumulate, void* stream) {
  if (n % 4) return adt_set_error("dropact_bwd: n %% 4");
  DropActArgs a{};
  a.X = X; a.dY = dY; a.dX = dX; a.n = (size_t)n; a.drop = adt_make_drop(p, seed, site); a.idx_offset = idx_offset; a.act = act;
  a.accumulate = accumulate;
  hipLaunchKernelGGL(k_dropact<true>, dim3(adt_grid_for((size_t)n / 4, 256, 2048)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("dropact_bwd");
}

int adt_gather_rows(const float* F, int ldf, const int32_t* rows, int M, const int32_t* m_dev, int d, float* out, int ldo, void* stream) {
  if (M <= 0) return 0;
  if ((d % 4) || (ldf % 4) || (ldo % 4)) return adt_set_error("gather_rows: d, ld %% 4");
  RowsArgs a{F, ldf, out, ldo, rows, M, d, 0, 0, m_dev};
  hipLaunchKernelGGL(k_rows, dim3(adt_grid_for((size_t)M * d / 4, 256, 2048)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("gather_rows");
}

int adt_scatter_rows(const float* G, int ldg, const int32_t* rows, int M, const int32_t* m_dev, int d, float* dF, int lddf, int accumulate,
                     void* stream) {
  if (M <= 0) return 0;
  if ((d % 4) || (ldg % 4) || (lddf % 4)) return adt_set_error("scatter_rows: d, ld %% 4");
  RowsArgs a{G, ldg, dF, lddf, rows, M, d, 1, accumulate, m_dev};
  hipLaunchKernelGGL(k_rows, dim3(adt_grid_for((size_t)M * d / 4, 256, 2048)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("scatter_rows");
}

int adt_ce_rows(float* logits, int ld, const int32_t* labels, int M, const int32_t* m_dev, int V, const float* inv_count, float* loss64,
                void* stream) {
  if (M <= 0) return 0;
  CeArgs a{logits, ld, labels, M, V, inv_count, loss64, m_dev};
  const size_t smem = ((size_t)(V + 3) / 4 * 4 + 16) * sizeof(float);
  if (smem <= 150 * 1024 && (ld % 4) == 0 && adt_aligned16(logits)) {      // row resident in LDS: one read + one write per element
    static AdtLdsOptIn optin;      // smem follows V: opt in once to the 150 KB this branch admits
    return adt_launch_lds1((const void*)k_ce_rows_lds, dim3(M < 1024 ? M : 1024), dim3(CE_NTH), smem, a, (hipStream_t)stream, "ce_rows(lds)", optin, 150 * 1024);
  }
  hipLaunchKernelGGL(k_ce_rows, dim3(M < 4096 ? M : 4096), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("ce_rows");
}

int adt_axpy(float* dst, const float* src, float alpha, int accumulate, int64_t n, const int32_t* mask_ids, int d, void* stream) {
  if (n % 4 || (mask_ids && (d <= 0 || d % 4))) return adt_set_error("axpy: n, d %% 4");
  AxpyArgs a{dst, src, alpha, accumulate, (size_t)n, mask_ids, d};
  hipLaunchKernelGGL(k_axpy, dim3(adt_grid_for((size_t)n / 4, 256, 2048)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("axpy");
}

int adt_log_softmax_fwd(const float* X, int64_t rows, int H, float* Y, void* stream) {
  if (H < 1 || H > 8) return adt_set_error("log_softmax: H=%d (1..8)", H);
  LsmArgs a{X, Y, nullptr, nullptr, (size_t)rows, H, 0};
  hipLaunchKernelGGL(k_logsoftmax_rows<false>, dim3(adt_grid_for((size_t)rows, 256, 2048)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("log_softmax_fwd");
}

int adt_log_softmax_bwd(const float* Y, const float* dY, int64_t rows, int H, float* dX, int accumulate, void* stream) {
  if (H < 1 || H > 8) return adt_set_error("log_softmax: H=%d (1..8)", H);
  LsmArgs a{nullptr, const_cast<float*>(Y), dY, dX, (size_t)rows, H, accumulate};
  hipLaunchKernelGGL(k_logsoftmax_rows<true>, dim3(adt_grid_for((size_t)rows, 256, 2048)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("log_softmax_bwd");
}

int adt_grad_sumsq(const float* G, int64_t n, float* out64, void* stream) {
  RangeOptArgs a{};
  a.G = const_cast<float*>(G); a.n = (size_t)n; a.out64 = out64;
  if (adt::zero_f32_async(out64, 64, (hipStream_t)stream)) return adt_set_error("grad_sumsq: zero");
  hipLaunchKernelGGL(k_sumsq64, dim3(adt_grid_for((size_t)n, 256, 512)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("grad_sumsq");
}

int adt_adam_range(float* P, float* G, float* M, float* V, int64_t n, float l2, float clip, float lr, float b1, float b2, float eps, float step,
                   const float* gn2_slots, void* stream) {
  if (n <= 0) return 0;
  RangeOptArgs a{P, G, M, V, (size_t)n, l2, clip, lr, b1, b2, eps, step, gn2_slots, nullptr, 0.f};
  hipLaunchKernelGGL(k_adam_range, dim3(adt_grid_for((size_t)n, 256, 1024)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("adam_range");
}

int adt_adamw_range(float* P, float* G, float* M, float* V, int64_t n, float wd, float clip, float lr, float b1, float b2, float eps, float step,
                    const float* gn2_slots, void* stream) {
  if (n <= 0) return 0;
  RangeOptArgs a{P, G, M, V, (size_t)n, 0.f, clip, lr, b1, b2, eps, step, gn2_slots, nullptr, wd};
  hipLaunchKernelGGL(k_adam_range, dim3(adt_grid_for((size_t)n, 256, 1024)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("adamw_range");
}

// ---- STOSA-ADT losses and scores (adt_stosa.cuh, adt_klattn.cuh) ------------------------------------------------------------------------
int adt_wdist_bpr(const float* Sm, const float* Sc, int lds, const float* Em, const float* Ec, const int32_t* pos, const int32_t* neg, int T,
                  int d, float pvn_weight, const float* inv_count, float* dSm, float* dSc, int ldds, float* dEm, float* dEc, float* loss3,
                  void* stream) {
  if (d % 64) return adt_set_error("wdist_bpr: d=%d must be a multiple of 64", d);
  WBprArgs a{Sm, Sc, lds, Em, Ec, pos, neg, T, d, pvn_weight, inv_count, dSm, dSc, ldds, dEm, dEc, loss3};
  hipLaunchKernelGGL(k_wdist_bpr<false>, dim3(adt_grid_for(T, 4, 2048)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("wdist_bpr");
}

int adt_wdist_full(const float* Sm, const float* Sc, int lds, const float* Em, const float* Ec, int B, int V, int d, float* dist, int ldo,
                   void* stream) {
  if (d % 4) return adt_set_error("wdist_full: d %% 4");
  WFullArgs a{Sm, Sc, lds, Em, Ec, B, V, d, dist, ldo};
  hipLaunchKernelGGL(k_wdist_full<false>, dim3(adt_grid_for((size_t)B * V, 16, 4096)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("wdist_full");
}

// row-wise KL loss and the chunked full-sort score (adt_klattn.cuh); arguments as adt_wdist_bpr / adt_wdist_full
int adt_kldist_bpr(const float* Sm, const float* Sc, int lds, const float* Em, const float* Ec, const int32_t* pos, const int32_t* neg, int T,
                  int d, float pvn_weight, const float* inv_count, float* dSm, float* dSc, int ldds, float* dEm, float* dEc, float* loss3,
                  void* stream) {
  if (d % 64) return adt_set_error("kldist_bpr: d=%d must be a multiple of 64", d);
  WBprArgs a{Sm, Sc, lds, Em, Ec, pos, neg, T, d, pvn_weight, inv_count, dSm, dSc, ldds, dEm, dEc, loss3};
  hipLaunchKernelGGL(k_kldist_bpr<false>, dim3(adt_grid_for(T, 4, 2048)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("kldist_bpr");
}

int adt_kldist_full(const float* Sm, const float* Sc, int lds, const float* Em, const float* Ec, int B, int V, int d, float* dist, int ldo,
                   void* stream) {
  if (B <= 0 || V <= 0) return 0;
  WFullArgs a{Sm, Sc, lds, Em, Ec, B, V, d, dist, ldo};
  hipLaunchKernelGGL(k_kldist_full<false>, dim3(adt_grid_for((size_t)B * V, 16, 4096)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("kldist_full");
}

int adt_topk_masked(float* dist, int ld, int B, int N, const int32_t* indptr, const int32_t* indices, int k, int32_t* out_idx,
                    float* out_val, void* stream) {
  if (B <= 0) return 0;
  if (k <= 0 || k > N) return adt_set_error("topk_masked: need 0 < k <= N");
  if (ld < N) return adt_set_error("topk_masked: ld < N");
  if ((indptr == nullptr) != (indices == nullptr)) return adt_set_error("topk_masked: indptr and indices go together");
  TopkArgs a{dist, ld, B, N, indptr, indices, k, out_idx, out_val};
  hipLaunchKernelGGL(k_topk_masked, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("topk_masked");
}

int adt_dense_gradsrc(const float* dY, int lddy, int T, int N, const int32_t* mask_ids, float p, const uint32_t* seed, uint32_t site,
                      uint32_t row_offset, int act, const float* U, int ldu, float* G, int ldg, const int32_t* t_dev, void* stream) {
  if (T <= 0 || N <= 0) return 0;
  if ((N % 4) || (lddy % 4) || (ldg % 4) || !adt_aligned16(dY) || !adt_aligned16(G)) return adt_set_error("dense_gradsrc: N, ld %% 4 and 16-byte alignment required");
  if (act != ACT_NONE && (!U || (ldu % 4) || !adt_aligned16(U))) return adt_set_error("dense_gradsrc: activation needs the saved pre-activation");
  GradSrcOutArgs a{};
  a.G.dY = dY; a.G.lddy = lddy; a.G.T = T; a.G.N = N; a.G.U = U; a.G.ldu = ldu; a.G.act = act;
  a.G.drop = adt_make_drop(p, seed, site); a.G.row_offset = row_offset; a.G.ids = mask_ids; a.G.idx_ld = N; a.G.idx_off = 0;
  a.out = G; a.ldo = ldg; a.t_dev = t_dev;
  hipLaunchKernelGGL(k_gradsrc, dim3(adt_grid_for((size_t)T * (N / 4), 1024, 4096)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("dense_gradsrc");
}

}  // extern "C"

// ---- widths that are not multiples of 64: padded lanes, true-width arithmetic (adt_lanes.cuh) -----------------------------------------
static int make_lanes(Lanes& ln, int H, int hd, int hd_pad, const char* what) { return adt_make_lanes(ln, H, hd, hd_pad, what); }

template <typename K64, typename K128, typename K192, typename K256, typename Args>
static void launch_by_width(int dp, K64 k64, K128 k128, K192 k192, K256 k256, int grid, hipStream_t s, const Args& a) {
  if (dp == 64) hipLaunchKernelGGL(k64, dim3(grid), dim3(LN_LANES_THREADS), 0, s, a);
  else if (dp == 128) hipLaunchKernelGGL(k128, dim3(grid), dim3(LN_LANES_THREADS), 0, s, a);
  else if (dp == 192) hipLaunchKernelGGL(k192, dim3(grid), dim3(LN_LANES_THREADS), 0, s, a);
  else hipLaunchKernelGGL(k256, dim3(grid), dim3(LN_LANES_THREADS), 0, s, a);
}

extern "C" {

int adt_layernorm_lanes_fwd(const float* X, int ldx, const float* gamma, const float* beta, float eps, int T, int H, int hd, int hd_pad,
                            float* Y, int ldy, void* stream) {
  LnLanesArgs a{};
  if (make_lanes(a.ln, H, hd, hd_pad, "layernorm_lanes_fwd")) return -1;
  if (T <= 0) return 0;
  if ((ldx % 4) || (ldy % 4) || ldx < H * hd_pad || ldy < H * hd_pad || !adt_aligned16(X) || !adt_aligned16(Y) || !adt_aligned16(gamma) || !adt_aligned16(beta))
    return adt_set_error("layernorm_lanes_fwd: ld %% 4, ld >= d_pad and 16-byte alignment required");
  a.X = X; a.ldx = ldx; a.gamma = gamma; a.beta = beta; a.eps = eps; a.Y = Y; a.ldy = ldy; a.T = T;
  launch_by_width(H * hd_pad, k_ln_lanes_fwd<64>, k_ln_lanes_fwd<128>, k_ln_lanes_fwd<192>, k_ln_lanes_fwd<256>, adt_grid_for(T, 16, 2048),
                  (hipStream_t)stream, a);
  return adt_check_launch("layernorm_lanes_fwd");
}

int adt_layernorm_lanes_bwd(const float* dY, int lddy, const float* X, int ldx, const float* gamma, float eps, int T, int H, int hd, int hd_pad,
                            float* dX, int lddx, int accumulate, float* dgamma, float* dbeta, void* stream) {
  LnLanesArgs a{};
  if (make_lanes(a.ln, H, hd, hd_pad, "layernorm_lanes_bwd")) return -1;
  if (T <= 0) return 0;
  const int dp = H * hd_pad;
  if ((ldx % 4) || (lddy % 4) || (lddx % 4) || ldx < dp || lddy < dp || lddx < dp || !adt_aligned16(X) || !adt_aligned16(dY) || !adt_aligned16(dX) || !adt_aligned16(gamma))
    return adt_set_error("layernorm_lanes_bwd: ld %% 4, ld >= d_pad and 16-byte alignment required");
  a.X = X; a.ldx = ldx; a.gamma = gamma; a.eps = eps; a.T = T; a.dY = dY; a.lddy = lddy; a.dX = dX; a.lddx = lddx;
  a.acc = accumulate; a.dgamma = dgamma; a.dbeta = dbeta;
  launch_by_width(dp, k_ln_lanes_bwd<64>, k_ln_lanes_bwd<128>, k_ln_lanes_bwd<192>, k_ln_lanes_bwd<256>, adt_grid_for(T, 16, 256), (hipStream_t)stream, a);
  return adt_check_launch("layernorm_lanes_bwd");
}

int adt_drop_lanes(const float* S, int lds, const float* R, int ldr, const float* R2, int ldr2, const int32_t* mask_ids, int T, int H, int hd,
                   int hd_pad, float p, const uint32_t* seed, uint32_t site, uint32_t row_offset, float* out, int ldo, void* stream) {
  DropLanesArgs a{};
  if (make_lanes(a.ln, H, hd, hd_pad, "drop_lanes")) return -1;
  if (T <= 0) return 0;
  const int dp = H * hd_pad;
  if ((lds % 4) || (ldo % 4) || lds < dp || ldo < dp || !adt_aligned16(S) || !adt_aligned16(out) || (R && ((ldr % 4) || ldr < dp || !adt_aligned16(R))) ||
      (R2 && ((ldr2 % 4) || ldr2 < dp || !adt_aligned16(R2))))
    return adt_set_error("drop_lanes: ld %% 4, ld >= d_pad and 16-byte alignment required");
  a.S = S; a.lds = lds; a.R = R; a.ldr = ldr; a.R2 = R2; a.ldr2 = ldr2; a.ids = mask_ids; a.out = out; a.ldo = ldo; a.T = T;
  a.drop = adt_make_drop(p, seed, site); a.row_offset = row_offset;
  hipLaunchKernelGGL(k_drop_lanes, dim3(adt_grid_for((size_t)T * (dp / 4), 1024, 4096)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("drop_lanes");
}

int adt_drn_lanes_fwd(const float* S, int lds, const float* R, int ldr, const float* gamma, const float* beta, float eps, int T, int H, int hd,
                      int hd_pad, float p, const uint32_t* seed, uint32_t site, uint32_t row_offset, float* Z, int ldz, float* Y, int ldy,
                      void* stream) {
  DrnLanesArgs a{};
  if (make_lanes(a.ln, H, hd, hd_pad, "drn_lanes_fwd")) return -1;
  if (T <= 0) return 0;
  const int dp = H * hd_pad;
  if (!S || !R || !Z || !Y || !gamma || !beta) return adt_set_error("drn_lanes_fwd: S, R, gamma, beta, Z and Y are required");
  if ((lds % 4) || (ldr % 4) || (ldz % 4) || (ldy % 4) || lds < dp || ldr < dp || ldz < dp || ldy < dp || !adt_aligned16(S) || !adt_aligned16(R) ||
      !adt_aligned16(Z) || !adt_aligned16(Y) || !adt_aligned16(gamma) || !adt_aligned16(beta))
    return adt_set_error("drn_lanes_fwd: ld %% 4, ld >= d_pad and 16-byte alignment required");
  a.S = S; a.lds = lds; a.R = R; a.ldr = ldr; a.gamma = gamma; a.beta = beta; a.eps = eps; a.Z = Z; a.ldz = ldz; a.Y = Y; a.ldy = ldy; a.T = T;
  a.drop = adt_make_drop(p, seed, site); a.row_offset = row_offset;
  launch_by_width(dp, k_drn_lanes_fwd<64>, k_drn_lanes_fwd<128>, k_drn_lanes_fwd<192>, k_drn_lanes_fwd<256>, adt_grid_for(T, 16, 2048),
                  (hipStream_t)stream, a);
  return adt_check_launch("drn_lanes_fwd");
}

int adt_drn_lanes_bwd(const float* dY, int lddy, const float* Z, int ldz, const float* gamma, float eps, int T, int H, int hd, int hd_pad, float p,
                      const uint32_t* seed, uint32_t site, uint32_t row_offset, float* dR, int lddr, int accumulate, float* dS, int ldds,
                      float* dgamma, float* dbeta, void* stream) {
  DrnLanesArgs a{};
  if (make_lanes(a.ln, H, hd, hd_pad, "drn_lanes_bwd")) return -1;
  if (T <= 0) return 0;
  const int dp = H * hd_pad;
  if (!dY || !Z || !gamma || !dR || !dS || !dgamma || !dbeta) return adt_set_error("drn_lanes_bwd: dY, Z, gamma, dR, dS, dgamma and dbeta are required");
  if ((lddy % 4) || (ldz % 4) || (lddr % 4) || (ldds % 4) || lddy < dp || ldz < dp || lddr < dp || ldds < dp || !adt_aligned16(dY) || !adt_aligned16(Z) ||
      !adt_aligned16(dR) || !adt_aligned16(dS) || !adt_aligned16(gamma))
    return adt_set_error("drn_lanes_bwd: ld %% 4, ld >= d_pad and 16-byte alignment required");
  // the backward only reads Z
  a.dY = dY; a.lddy = lddy; a.Z = const_cast<float*>(Z); a.ldz = ldz; a.gamma = gamma; a.eps = eps; a.T = T; a.dR = dR; a.lddr = lddr; a.acc = accumulate;
  a.dS = dS; a.ldds = ldds; a.dgamma = dgamma; a.dbeta = dbeta;
  a.drop = adt_make_drop(p, seed, site); a.row_offset = row_offset;
  launch_by_width(dp, k_drn_lanes_bwd<64>, k_drn_lanes_bwd<128>, k_drn_lanes_bwd<192>, k_drn_lanes_bwd<256>, adt_grid_for(T, 16, 256),
                  (hipStream_t)stream, a);
  return adt_check_launch("drn_lanes_bwd");
}

int adt_lane_map(float* padded, float* compact, const int32_t* map, int64_t n, int scatter, void* stream) {
  if (n <= 0) return 0;
  LaneMapArgs a{padded, compact, map, (size_t)n, scatter};
  hipLaunchKernelGGL(k_lane_map, dim3(adt_grid_for((size_t)n, 1024, 4096)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("lane_map");
}

int adt_attn_masked_scaled_fwd(int prec, const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, int B, int H, int L, int hd,
                               float scale, int causal, const int32_t* key_ids, float fill, float p, const uint32_t* seed, uint32_t site,
                               uint32_t b_offset, float* O, int ldo, float* LSE, void* stream) {
  if (!(scale > 0.f)) return adt_set_error("attn_masked_scaled_fwd: scale %g must be positive", (double)scale);
  return attn_masked_fwd_impl(prec, Q, ldq, K, ldk, V, ldv, B, H, L, hd, scale, causal, key_ids, fill, p, seed, site, b_offset, O, ldo, LSE, stream);
}

int adt_attn_masked_scaled_bwd(int prec, const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, const float* O, int ldo,
                               const float* LSE, const float* dO, int lddo, int B, int H, int L, int hd, float scale, int causal,
                               const int32_t* key_ids, float fill, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQ,
                               int lddq, float* dK, int lddk, float* dV, int lddv, void* stream) {
  if (!(scale > 0.f)) return adt_set_error("attn_masked_scaled_bwd: scale %g must be positive", (double)scale);
  return attn_masked_bwd_impl(prec, Q, ldq, K, ldk, V, ldv, O, ldo, LSE, dO, lddo, B, H, L, hd, scale, causal, key_ids, fill, p, seed, site, b_offset,
                              dQ, lddq, dK, lddk, dV, lddv, stream);
}

// ---- STOSA-ADT at padded widths --------------------------------------------------------------------------------
// The Wasserstein attention with the score scale given (1 / sqrt(true head size)) and only lanes [0, hd_live) of a head live: arguments
// as adt_wattn_fwd / _bwd and adt_wattn_mfma_fwd / _bwd with (scale, hd_live) after hd.  The forward and the backward take the same scale.
static int wattn_scaled_check(const char* what, float scale, int hd_live, int hd) {
  if (!(scale > 0.f) || hd_live < 1 || hd_live > hd) return adt_set_error("%s: scale %g must be positive and 1 <= hd_live=%d <= hd=%d", what, (double)scale, hd_live, hd);
  return 0;
}

int adt_wattn_scaled_fwd(const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                         const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float scale,
                         int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc,
                         float* LSE, void* stream) {
  if (wattn_scaled_check("wattn_scaled_fwd", scale, hd_live, hd)) return -1;
  WAttnArgs a = make_wattn_args(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, p, seed, site, b_offset, Om, ldom, Oc, ldoc, LSE);
  a.xscale = scale; a.hd_live = hd_live;
  return stosa_attn<WM_W>(false, a, stream);
}

int adt_wattn_scaled_bwd(const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                         const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, const float* Om, int ldom, const float* Oc,
                         int ldoc, const float* LSE, const float* dOm, int lddom, const float* dOc, int lddoc, int B, int H, int L, int hd,
                         float scale, int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQm, float* dQc,
                         float* dKm, float* dKc, float* dVm, float* dVc, int ldd, void* stream) {
  if (wattn_scaled_check("wattn_scaled_bwd", scale, hd_live, hd)) return -1;
  WAttnArgs a = make_wattn_args_bwd(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, Om, ldom, Oc, ldoc, LSE, dOm, lddom, dOc, lddoc,
                                    B, H, L, hd, p, seed, site, b_offset, dQm, dQc, dKm, dKc, dVm, dVc, ldd);
  a.xscale = scale; a.hd_live = hd_live;
  return stosa_attn<WM_W>(true, a, stream);
}

int adt_wattn_mfma_scaled_fwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                              const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float scale,
                              int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc,
                              float* LSE, void* stream) {
  if (wattn_scaled_check("wattn_mfma_scaled_fwd", scale, hd_live, hd)) return -1;
  WAttnArgs a = make_wattn_args(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, p, seed, site, b_offset, Om, ldom, Oc, ldoc, LSE);
  a.xscale = scale; a.hd_live = hd_live;
  return wattn_mfma_dispatch<WM_W>(prec, false, a, (hipStream_t)stream);
}

int adt_wattn_mfma_scaled_bwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                              const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, const float* Om, int ldom, const float* Oc,
                              int ldoc, const float* LSE, const float* dOm, int lddom, const float* dOc, int lddoc, int B, int H, int L, int hd,
                              float scale, int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQm, float* dQc,
                              float* dKm, float* dKc, float* dVm, float* dVc, int ldd, void* stream) {
  if (wattn_scaled_check("wattn_mfma_scaled_bwd", scale, hd_live, hd)) return -1;
  WAttnArgs a = make_wattn_args_bwd(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, Om, ldom, Oc, ldoc, LSE, dOm, lddom, dOc, lddoc,
                                    B, H, L, hd, p, seed, site, b_offset, dQm, dQc, dKm, dKc, dVm, dVc, ldd);
  a.xscale = scale; a.hd_live = hd_live;
  return wattn_mfma_dispatch<WM_W>(prec, true, a, (hipStream_t)stream);
}

// adt_wdist_bpr / adt_wdist_full on padded rows and tables (d_pad = H * hd_pad columns each): the pad lanes stay out of every sum, and
// dSm / dSc get +0.0 there; the tables' pad lanes receive no atomic.
int adt_wdist_bpr_lanes(const float* Sm, const float* Sc, int lds, const float* Em, const float* Ec, const int32_t* pos, const int32_t* neg, int T,
                        int H, int hd, int hd_pad, float pvn_weight, const float* inv_count, float* dSm, float* dSc, int ldds, float* dEm, float* dEc,
                        float* loss3, void* stream) {
  WBprArgs a{Sm, Sc, lds, Em, Ec, pos, neg, T, H * hd_pad, pvn_weight, inv_count, dSm, dSc, ldds, dEm, dEc, loss3};
  if (make_lanes(a.ln, H, hd, hd_pad, "wdist_bpr_lanes")) return -1;
  if (lds < a.d || ldds < a.d) return adt_set_error("wdist_bpr_lanes: lds=%d and ldds=%d must be >= d_pad=%d", lds, ldds, a.d);
  hipLaunchKernelGGL(k_wdist_bpr<true>, dim3(adt_grid_for(T, 4, 2048)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("wdist_bpr_lanes");
}

int adt_wdist_full_lanes(const float* Sm, const float* Sc, int lds, const float* Em, const float* Ec, int B, int V, int H, int hd, int hd_pad,
                         float* dist, int ldo, void* stream) {
  WFullArgs a{Sm, Sc, lds, Em, Ec, B, V, H * hd_pad, dist, ldo};
  if (make_lanes(a.ln, H, hd, hd_pad, "wdist_full_lanes")) return -1;
  if (lds < a.d || ldo < V) return adt_set_error("wdist_full_lanes: lds=%d must be >= d_pad=%d and ldo=%d >= V=%d", lds, a.d, ldo, V);
  if (B <= 0 || V <= 0) return 0;
  hipLaunchKernelGGL(k_wdist_full<true>, dim3(adt_grid_for((size_t)B * V, 16, 4096)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("wdist_full_lanes");
}

// Activation (with its dropout site) on padded lanes: adt_lanes.cuh, k_act_lanes
int adt_act_lanes_fwd(const float* X, int ldx, int T, int H, int hd, int hd_pad, float p, const uint32_t* seed, uint32_t site, uint32_t row_offset,
                      int act, float* Y, int ldy, void* stream) {
  ActLanesArgs a{};
  if (make_lanes(a.ln, H, hd, hd_pad, "act_lanes_fwd")) return -1;
  if (T <= 0) return 0;
  const int dp = H * hd_pad;
  if (!X || !Y) return adt_set_error("act_lanes_fwd: X and Y are required");
  if ((ldx % 4) || (ldy % 4) || ldx < dp || ldy < dp || !adt_aligned16(X) || !adt_aligned16(Y))
    return adt_set_error("act_lanes_fwd: ld %% 4, ld >= d_pad and 16-byte alignment required");
  a.X = X; a.ldx = ldx; a.out = Y; a.ldo = ldy; a.T = T; a.drop = adt_make_drop(p, seed, site); a.row_offset = row_offset; a.act = act;
  hipLaunchKernelGGL(k_act_lanes<false>, dim3(adt_grid_for((size_t)T * (dp / 4), 1024, 4096)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("act_lanes_fwd");
}

int adt_act_lanes_bwd(const float* dY, int lddy, const float* X, int ldx, int T, int H, int hd, int hd_pad, float p, const uint32_t* seed,
                      uint32_t site, uint32_t row_offset, int act, float* dX, int lddx, int accumulate, void* stream) {
  ActLanesArgs a{};
  if (make_lanes(a.ln, H, hd, hd_pad, "act_lanes_bwd")) return -1;
  if (T <= 0) return 0;
  const int dp = H * hd_pad;
  if (!dY || !X || !dX) return adt_set_error("act_lanes_bwd: dY, X and dX are required");
  if ((ldx % 4) || (lddy % 4) || (lddx % 4) || ldx < dp || lddy < dp || lddx < dp || !adt_aligned16(X) || !adt_aligned16(dY) || !adt_aligned16(dX))
    return adt_set_error("act_lanes_bwd: ld %% 4, ld >= d_pad and 16-byte alignment required");
  a.X = X; a.ldx = ldx; a.dY = dY; a.lddy = lddy; a.out = dX; a.ldo = lddx; a.acc = accumulate; a.T = T;
  a.drop = adt_make_drop(p, seed, site); a.row_offset = row_offset; a.act = act;
  hipLaunchKernelGGL(k_act_lanes<true>, dim3(adt_grid_for((size_t)T * (dp / 4), 1024, 4096)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("act_lanes_bwd");
}

// ---- STOSA-ADT under KL at padded widths -----------------------------------------------------------------------
// The KL attention with the score scale given and lanes [0, hd_live) of a head live: the same launchers as adt_klattn_* / adt_klattn_mfma_*.
// A pad lane holds cov = 0: the kernels leave it out of 1 / ck, of both log-determinants and of the subtracted head size, and write +0.0
// to it in all six gradients, by selects on the lane index.
int adt_klattn_scaled_fwd(const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                          const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float scale,
                          int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc,
                          float* LSE, void* stream) {
  if (wattn_scaled_check("klattn_scaled_fwd", scale, hd_live, hd)) return -1;
  WAttnArgs a = make_wattn_args(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, p, seed, site, b_offset, Om, ldom, Oc, ldoc, LSE);
  a.xscale = scale; a.hd_live = hd_live;
  return stosa_attn<WM_KLP>(false, a, stream);
}

int adt_klattn_scaled_bwd(const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                          const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, const float* Om, int ldom, const float* Oc,
                          int ldoc, const float* LSE, const float* dOm, int lddom, const float* dOc, int lddoc, int B, int H, int L, int hd,
                          float scale, int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQm, float* dQc,
                          float* dKm, float* dKc, float* dVm, float* dVc, int ldd, void* stream) {
  if (wattn_scaled_check("klattn_scaled_bwd", scale, hd_live, hd)) return -1;
  WAttnArgs a = make_wattn_args_bwd(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, Om, ldom, Oc, ldoc, LSE, dOm, lddom, dOc, lddoc,
                                    B, H, L, hd, p, seed, site, b_offset, dQm, dQc, dKm, dKc, dVm, dVc, ldd);
  a.xscale = scale; a.hd_live = hd_live;
  return stosa_attn<WM_KLP>(true, a, stream);
}

int adt_klattn_mfma_scaled_fwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                               const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float scale,
                               int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc,
                               float* LSE, void* stream) {
  if (wattn_scaled_check("klattn_mfma_scaled_fwd", scale, hd_live, hd)) return -1;
  WAttnArgs a = make_wattn_args(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, p, seed, site, b_offset, Om, ldom, Oc, ldoc, LSE);
  a.xscale = scale; a.hd_live = hd_live;
  return wattn_mfma_dispatch<WM_KLP>(prec, false, a, (hipStream_t)stream);
}

int adt_klattn_mfma_scaled_bwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                               const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, const float* Om, int ldom, const float* Oc,
                               int ldoc, const float* LSE, const float* dOm, int lddom, const float* dOc, int lddoc, int B, int H, int L, int hd,
                               float scale, int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQm, float* dQc,
                               float* dKm, float* dKc, float* dVm, float* dVc, int ldd, void* stream) {
  if (wattn_scaled_check("klattn_mfma_scaled_bwd", scale, hd_live, hd)) return -1;
  WAttnArgs a = make_wattn_args_bwd(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, Om, ldom, Oc, ldoc, LSE, dOm, lddom, dOc, lddoc,
                                    B, H, L, hd, p, seed, site, b_offset, dQm, dQc, dKm, dKc, dVm, dVc, ldd);
  a.xscale = scale; a.hd_live = hd_live;
  return wattn_mfma_dispatch<WM_KLP>(prec, true, a, (hipStream_t)stream);
}

// adt_kldist_bpr / adt_kldist_full on padded rows and tables (d_pad = H * hd_pad columns each): the pad lanes stay out of every sum and
// log, the divergences subtract the true d = H * hd, dSm / dSc get +0.0 on them and the tables' pad lanes receive no atomic.
int adt_kldist_bpr_lanes(const float* Sm, const float* Sc, int lds, const float* Em, const float* Ec, const int32_t* pos, const int32_t* neg, int T,
                         int H, int hd, int hd_pad, float pvn_weight, const float* inv_count, float* dSm, float* dSc, int ldds, float* dEm, float* dEc,
                         float* loss3, void* stream) {
  WBprArgs a{Sm, Sc, lds, Em, Ec, pos, neg, T, H * hd_pad, pvn_weight, inv_count, dSm, dSc, ldds, dEm, dEc, loss3};
  if (make_lanes(a.ln, H, hd, hd_pad, "kldist_bpr_lanes")) return -1;
  if (lds < a.d || ldds < a.d) return adt_set_error("kldist_bpr_lanes: lds=%d and ldds=%d must be >= d_pad=%d", lds, ldds, a.d);
  hipLaunchKernelGGL(k_kldist_bpr<true>, dim3(adt_grid_for(T, 4, 2048)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("kldist_bpr_lanes");
}

int adt_kldist_full_lanes(const float* Sm, const float* Sc, int lds, const float* Em, const float* Ec, int B, int V, int H, int hd, int hd_pad,
                          float* dist, int ldo, void* stream) {
  WFullArgs a{Sm, Sc, lds, Em, Ec, B, V, H * hd_pad, dist, ldo};
  if (make_lanes(a.ln, H, hd, hd_pad, "kldist_full_lanes")) return -1;
  if (lds < a.d || ldo < V) return adt_set_error("kldist_full_lanes: lds=%d must be >= d_pad=%d and ldo=%d >= V=%d", lds, a.d, ldo, V);
  if (B <= 0 || V <= 0) return 0;
  hipLaunchKernelGGL(k_kldist_full<true>, dim3(adt_grid_for((size_t)B * V, 16, 4096)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("kldist_full_lanes");
}

}  // extern "C"
