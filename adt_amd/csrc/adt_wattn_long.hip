// C ABI (include/adt_hip.h): STOSA-ADT distance attention at 1 <= L <= 1024 (adt_wattn_long.cuh), head size 16 / 32 / 64, both metrics,
// either precision.  A translation unit of its own: the code objects of the shorter lengths (adt_wide.hip) stay as they are.  Host code only
// enqueues work on the caller's stream.
#include "adt_host.h"

#include "adt_wattn_long.cuh"

using namespace adt;

static_assert(PREC_F32 == ADT_PREC_F32 && PREC_BF16 == ADT_PREC_BF16, "adt_wide_plan.h speaks of the ABI's prec values");
static_assert(wattn_long_lds(64, wattn_long_kc(true), true) <= ADT_LDS_MAX && wattn_long_lds(64, wattn_long_kc(false), false) <= ADT_LDS_MAX,
              "the tightest instantiations fit the LDS");
static_assert(W_KPL * 64 == WATTN_VALU_LMAX, "adt_wide_plan.h restates the vector-ALU kernels' length bound");

// adt_wattn_long_plan (adt_wide_plan.h) chooses the grid and the footprint; this names the instantiation
template <int PREC, int HD, int MET>
static int launch_wattn_long(const AttnPlan& p, bool bwd, const WAttnArgs& a, hipStream_t s) {
  constexpr int CHF = wattn_long_kc(false), CHB = wattn_long_kc(true);
  static_assert(wattn_long_lds(HD, CHF, false) == WattnLongLds<HD, CHF>::fwd_bytes, "plan and kernel disagree on the LDS footprint");
  static_assert(wattn_long_lds(HD, CHB, true) == WattnLongLds<HD, CHB>::bwd_bytes, "plan and kernel disagree on the LDS footprint");
  static_assert(ATTN_STREAMED_NW == WM_NW, "plan and kernel disagree on the waves of a workgroup");
  const void* fn = bwd ? (const void*)k_wattn_long_bwd<PREC, HD, MET, CHB> : (const void*)k_wattn_long_fwd<PREC, HD, MET, CHF>;
  static AdtLdsOptIn optin[2];
  return adt_launch_lds1(fn, dim3(a.B * a.H, p.grid_y), dim3(p.waves * 64), p.lds_bytes, a, s,
                         wm_kl(MET) ? (bwd ? "klattn_long_bwd" : "klattn_long_fwd") : (bwd ? "wattn_long_bwd" : "wattn_long_fwd"), optin[bwd ? 1 : 0]);
}

template <int PREC, int MET>
static int launch_wattn_long_hd(const AttnPlan& p, bool bwd, const WAttnArgs& a, hipStream_t s) {
  if (a.hd == 16) return launch_wattn_long<PREC, 16, MET>(p, bwd, a, s);
  if (a.hd == 32) return launch_wattn_long<PREC, 32, MET>(p, bwd, a, s);
  return launch_wattn_long<PREC, 64, MET>(p, bwd, a, s);
}

// The checks both directions share, the plan's refusals (precision, head size, length, LDS) first; then the launch.  lds: every row stride of
// the call (16-byte loads and stores along the features).
template <int MET>
static int wattn_long(int prec, bool bwd, const WAttnArgs& a, float p, uint32_t b_offset, const int* lds, int nlds, void* stream) {
  const char* what = wm_kl(MET) ? (bwd ? "klattn_long_bwd" : "klattn_long_fwd") : (bwd ? "wattn_long_bwd" : "wattn_long_fwd");
  const AttnPlan plan = adt_wattn_long_plan(prec, a.hd, a.L, bwd);
  if (plan.error[0]) return adt_set_error("%s: %s", what, plan.error);
  if (a.B <= 0 || a.H <= 0) return adt_set_error("%s: empty shape", what);
  if (!a.kid) return adt_set_error("%s: key_ids is null", what);
  for (int i = 0; i < nlds; ++i)
    if (lds[i] % 4) return adt_set_error("%s: ld %% 4", what);
  // the dropout element index ((b_offset + b) * H + h) * L * L + i * L + j is a uint32: past 2^32 two elements would share a draw
  if (p > 0.f && ((uint64_t)b_offset + (uint64_t)a.B) * (uint64_t)a.H * (uint64_t)a.L * (uint64_t)a.L >= (1ull << 32))
    return adt_set_error("%s: dropout index space (b_offset + B) * H * L * L = (%u + %d) * %d * %d * %d reaches 2^32", what, b_offset, a.B, a.H, a.L, a.L);
  return prec == ADT_PREC_F32 ? launch_wattn_long_hd<PREC_F32, MET>(plan, bwd, a, (hipStream_t)stream)
                              : launch_wattn_long_hd<PREC_BF16, MET>(plan, bwd, a, (hipStream_t)stream);
}

static WAttnArgs wattn_long_args(const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                                 const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float p,
                                 const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc, float* LSE, float xscale, int hd_live) {
  WAttnArgs a{};
  a.Qm = Qm; a.ldqm = ldqm; a.Qc = Qc; a.ldqc = ldqc; a.Km = Km; a.ldkm = ldkm; a.Kc = Kc; a.ldkc = ldkc; a.Vm = Vm; a.ldvm = ldvm;
  a.Vc = Vc; a.ldvc = ldvc; a.kid = key_ids; a.B = B; a.H = H; a.L = L; a.hd = hd; a.scale = 1.0f / sqrtf((float)(hd > 0 ? hd : 1));
  a.drop = adt_make_drop(p, seed, site); a.bh_offset = b_offset * (uint32_t)H; a.Om = Om; a.ldom = ldom; a.Oc = Oc; a.ldoc = ldoc; a.LSE = LSE;
  a.xscale = xscale; a.hd_live = hd_live;      // 0, 0: the scale and the live lanes follow hd
  return a;
}

template <int MET>
static int wattn_long_fwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                          const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float p,
                          const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc, float* LSE, void* stream,
                          float xscale = 0.f, int hd_live = 0) {
  const WAttnArgs a = wattn_long_args(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, p, seed, site, b_offset, Om, ldom,
                                      Oc, ldoc, LSE, xscale, hd_live);
  const int lds[8] = {ldqm, ldqc, ldkm, ldkc, ldvm, ldvc, ldom, ldoc};
  return wattn_long<MET>(prec, false, a, p, b_offset, lds, 8, stream);
}

template <int MET>
static int wattn_long_bwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                          const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, const float* Om, int ldom, const float* Oc,
                          int ldoc, const float* LSE, const float* dOm, int lddom, const float* dOc, int lddoc, int B, int H, int L, int hd, float p,
                          const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQm, float* dQc, float* dKm, float* dKc, float* dVm,
                          float* dVc, int ldd, void* stream, float xscale = 0.f, int hd_live = 0) {
  WAttnArgs a = wattn_long_args(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, p, seed, site, b_offset,
                                const_cast<float*>(Om), ldom, const_cast<float*>(Oc), ldoc, const_cast<float*>(LSE), xscale, hd_live);
  a.dOm = dOm; a.lddom = lddom; a.dOc = dOc; a.lddoc = lddoc;
  a.dQm = dQm; a.dQc = dQc; a.dKm = dKm; a.dKc = dKc; a.dVm = dVm; a.dVc = dVc; a.ldd = ldd;
  const int lds[11] = {ldqm, ldqc, ldkm, ldkc, ldvm, ldvc, ldom, ldoc, lddom, lddoc, ldd};
  return wattn_long<MET>(prec, true, a, p, b_offset, lds, 11, stream);
}

extern "C" {

int adt_wattn_max_len(int hd) {
  // adt_wide_plan.h restates adt_stosa_args.cuh's footprint: the bound and the one beyond it, checked once against the kernels' own function
  static const bool same = [] {
    for (int h : {16, 32, 64})
      for (int L : {1, 63, 64, 141, 142, 255, 256})
        for (bool bwd : {false, true})
          if (wattn_valu_lds(L, h, bwd) != wattn_lds_bytes(L, h, bwd)) return false;
    return true;
  }();
  if (!same) return adt_set_error("wattn_max_len: adt_wide_plan.h and adt_stosa_args.cuh disagree on the LDS footprint");
  return adt::adt_wattn_max_len(hd);
}

int adt_wattn_long_fwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                       const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float p,
                       const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc, float* LSE,
                       void* stream) {
  return wattn_long_fwd<WM_W>(prec, Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, p, seed, site, b_offset, Om, ldom,
                              Oc, ldoc, LSE, stream);
}

int adt_wattn_long_bwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                       const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, const float* Om, int ldom, const float* Oc,
                       int ldoc, const float* LSE, const float* dOm, int lddom, const float* dOc, int lddoc, int B, int H, int L, int hd, float p,
                       const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQm, float* dQc, float* dKm, float* dKc, float* dVm,
                       float* dVc, int ldd, void* stream) {
  return wattn_long_bwd<WM_W>(prec, Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, Om, ldom, Oc, ldoc, LSE, dOm, lddom, dOc, lddoc,
                              B, H, L, hd, p, seed, site, b_offset, dQm, dQc, dKm, dKc, dVm, dVc, ldd, stream);
}

// Padded heads: the score scale is given (1 / sqrt(true head size)) and only lanes [0, hd_live) of a head are live; everything else as
// adt_wattn_long_fwd / _bwd.  The forward and the backward must be given the same scale.
int adt_wattn_long_scaled_fwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                              const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float scale,
                              int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc,
                              float* LSE, void* stream) {
  if (!(scale > 0.f) || hd_live < 1 || hd_live > hd) return adt_set_error("wattn_long_scaled_fwd: scale %g must be positive and 1 <= hd_live=%d <= hd=%d", (double)scale, hd_live, hd);
  return wattn_long_fwd<WM_W>(prec, Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, p, seed, site, b_offset, Om, ldom,
                              Oc, ldoc, LSE, stream, scale, hd_live);
}

int adt_wattn_long_scaled_bwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                              const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, const float* Om, int ldom, const float* Oc,
                              int ldoc, const float* LSE, const float* dOm, int lddom, const float* dOc, int lddoc, int B, int H, int L, int hd,
                              float scale, int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQm, float* dQc,
                              float* dKm, float* dKc, float* dVm, float* dVc, int ldd, void* stream) {
  if (!(scale > 0.f) || hd_live < 1 || hd_live > hd) return adt_set_error("wattn_long_scaled_bwd: scale %g must be positive and 1 <= hd_live=%d <= hd=%d", (double)scale, hd_live, hd);
  return wattn_long_bwd<WM_W>(prec, Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, Om, ldom, Oc, ldoc, LSE, dOm, lddom, dOc, lddoc,
                              B, H, L, hd, p, seed, site, b_offset, dQm, dQc, dKm, dKc, dVm, dVc, ldd, stream, scale, hd_live);
}

int adt_klattn_long_fwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                        const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float p,
                        const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc, float* LSE,
                        void* stream) {
  return wattn_long_fwd<WM_KL>(prec, Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, p, seed, site, b_offset, Om, ldom,
                               Oc, ldoc, LSE, stream);
}

int adt_klattn_long_bwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                        const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, const float* Om, int ldom, const float* Oc,
                        int ldoc, const float* LSE, const float* dOm, int lddom, const float* dOc, int lddoc, int B, int H, int L, int hd, float p,
                        const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQm, float* dQc, float* dKm, float* dKc, float* dVm,
                        float* dVc, int ldd, void* stream) {
  return wattn_long_bwd<WM_KL>(prec, Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, Om, ldom, Oc, ldoc, LSE, dOm, lddom, dOc, lddoc,
                               B, H, L, hd, p, seed, site, b_offset, dQm, dQc, dKm, dKc, dVm, dVc, ldd, stream);
}

// The KL attention on padded heads: the scale given, lanes [0, hd_live) live, the pad lanes (cov = 0) left out of
// 1 / ck, the log-determinants and the subtracted head size, and +0.0 in all six gradients.
int adt_klattn_long_scaled_fwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                               const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float scale,
                               int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc,
                               float* LSE, void* stream) {
  if (!(scale > 0.f) || hd_live < 1 || hd_live > hd) return adt_set_error("klattn_long_scaled_fwd: scale %g must be positive and 1 <= hd_live=%d <= hd=%d", (double)scale, hd_live, hd);
  return wattn_long_fwd<WM_KLP>(prec, Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, p, seed, site, b_offset, Om, ldom,
                               Oc, ldoc, LSE, stream, scale, hd_live);
}

int adt_klattn_long_scaled_bwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                               const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, const float* Om, int ldom, const float* Oc,
                               int ldoc, const float* LSE, const float* dOm, int lddom, const float* dOc, int lddoc, int B, int H, int L, int hd,
                               float scale, int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQm, float* dQc,
                               float* dKm, float* dKc, float* dVm, float* dVc, int ldd, void* stream) {
  if (!(scale > 0.f) || hd_live < 1 || hd_live > hd) return adt_set_error("klattn_long_scaled_bwd: scale %g must be positive and 1 <= hd_live=%d <= hd=%d", (double)scale, hd_live, hd);
  return wattn_long_bwd<WM_KLP>(prec, Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, Om, ldom, Oc, ldoc, LSE, dOm, lddom, dOc, lddoc,
                               B, H, L, hd, p, seed, site, b_offset, dQm, dQc, dKm, dKc, dVm, dVc, ldd, stream, scale, hd_live);
}

}  // extern "C"
