// C ABI (include/adt_hip.h): STOSA-ADT distance attention at head size 128, 1 <= L <= 1024, both metrics, either precision: the streamed
// kernels of adt_wattn_long.cuh instantiated at HD = 128.  A translation unit of its own: the code objects of head
// sizes 16 / 32 / 64 (adt_wattn_long.hip) and of the shorter lengths (adt_wide.hip) stay as they are.  A 256-thread workgroup is one wave per
// SIMD, so a lane may use the whole 512-entry register file; the templates fit it unchanged (tools/kernel_resources.sh adt_wattn_hd128.hip).
// Host code only enqueues work on the caller's stream.
#include "adt_host.h"

#include "adt_wattn_long.cuh"

using namespace adt;

static_assert(PREC_F32 == ADT_PREC_F32 && PREC_BF16 == ADT_PREC_BF16, "adt_wide_plan.h speaks of the ABI's prec values");

constexpr int HD128 = 128;

// adt_wattn_hd128_plan (adt_wide_plan.h) chooses the chunk, the grid and the footprint; this names the instantiation
template <int PREC, int MET>
static int launch_wattn_hd128(const AttnPlan& p, bool bwd, const WAttnArgs& a, hipStream_t s) {
  constexpr int CHF = wattn_hd128_kc(false), CHB = wattn_hd128_kc(true);
  static_assert(CHF >= 32 && CHB >= 32, "a chunk of whole tile pairs fits the LDS in both directions");
  static_assert(wattn_long_lds(HD128, CHF, false) == WattnLongLds<HD128, CHF>::fwd_bytes, "plan and kernel disagree on the LDS footprint");
  static_assert(wattn_long_lds(HD128, CHB, true) == WattnLongLds<HD128, CHB>::bwd_bytes, "plan and kernel disagree on the LDS footprint");
  static_assert(wattn_long_lds(HD128, CHF, false) <= ADT_LDS_MAX && wattn_long_lds(HD128, CHB, true) <= ADT_LDS_MAX, "both directions fit the LDS");
  static_assert(ATTN_STREAMED_NW == WM_NW, "plan and kernel disagree on the waves of a workgroup");
  const void* fn = bwd ? (const void*)k_wattn_long_bwd<PREC, HD128, MET, CHB> : (const void*)k_wattn_long_fwd<PREC, HD128, MET, CHF>;
  static AdtLdsOptIn optin[2];
  return adt_launch_lds1(fn, dim3(a.B * a.H, p.grid_y), dim3(p.waves * 64), p.lds_bytes, a, s,
                         wm_kl(MET) ? (bwd ? "klattn_hd128_bwd" : "klattn_hd128_fwd") : (bwd ? "wattn_hd128_bwd" : "wattn_hd128_fwd"), optin[bwd ? 1 : 0]);
}

// The checks of adt_wattn_long.hip's wattn_long() in its order: the plan's refusals (precision, head size, length) first, an empty shape,
// null key ids, the row strides (16-byte loads and stores along the features), the scale and the live lanes, the dropout index space; then
// the launch.  KL picks the unpadded kernel when every lane is live: its lane tests fold away at compile time.
template <bool KL>
static int wattn_hd128(int prec, bool bwd, const WAttnArgs& a, float p, uint32_t b_offset, const int* lds, int nlds, void* stream) {
  const char* what = KL ? (bwd ? "klattn_hd128_bwd" : "klattn_hd128_fwd") : (bwd ? "wattn_hd128_bwd" : "wattn_hd128_fwd");
  const AttnPlan plan = adt_wattn_hd128_plan(prec, a.hd, a.L, bwd);
  if (plan.error[0]) return adt_set_error("%s: %s", what, plan.error);
  if (a.B <= 0 || a.H <= 0) return adt_set_error("%s: empty shape", what);
  if (!a.kid) return adt_set_error("%s: key_ids is null", what);
  for (int i = 0; i < nlds; ++i)
    if (lds[i] % 4) return adt_set_error("%s: ld %% 4", what);
  if (!(a.xscale > 0.f) || a.hd_live < 1 || a.hd_live > a.hd)
    return adt_set_error("%s: scale %g must be positive and 1 <= hd_live=%d <= hd=%d", what, (double)a.xscale, a.hd_live, a.hd);
  // the dropout element index ((b_offset + b) * H + h) * L * L + i * L + j is a uint32: past 2^32 two elements would share a draw
  if (p > 0.f && ((uint64_t)b_offset + (uint64_t)a.B) * (uint64_t)a.H * (uint64_t)a.L * (uint64_t)a.L >= (1ull << 32))
    return adt_set_error("%s: dropout index space (b_offset + B) * H * L * L = (%u + %d) * %d * %d * %d reaches 2^32", what, b_offset, a.B, a.H, a.L, a.L);
  hipStream_t s = (hipStream_t)stream;
  if constexpr (KL) {
    if (a.hd_live == a.hd) return prec == ADT_PREC_F32 ? launch_wattn_hd128<PREC_F32, WM_KL>(plan, bwd, a, s) : launch_wattn_hd128<PREC_BF16, WM_KL>(plan, bwd, a, s);
    return prec == ADT_PREC_F32 ? launch_wattn_hd128<PREC_F32, WM_KLP>(plan, bwd, a, s) : launch_wattn_hd128<PREC_BF16, WM_KLP>(plan, bwd, a, s);
  } else {
    return prec == ADT_PREC_F32 ? launch_wattn_hd128<PREC_F32, WM_W>(plan, bwd, a, s) : launch_wattn_hd128<PREC_BF16, WM_W>(plan, bwd, a, s);
  }
}

static WAttnArgs wattn_hd128_args(const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                                  const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float scale,
                                  int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc,
                                  float* LSE) {
  WAttnArgs a{};
  a.Qm = Qm; a.ldqm = ldqm; a.Qc = Qc; a.ldqc = ldqc; a.Km = Km; a.ldkm = ldkm; a.Kc = Kc; a.ldkc = ldkc; a.Vm = Vm; a.ldvm = ldvm;
  a.Vc = Vc; a.ldvc = ldvc; a.kid = key_ids; a.B = B; a.H = H; a.L = L; a.hd = hd; a.scale = scale;
  a.drop = adt_make_drop(p, seed, site); a.bh_offset = b_offset * (uint32_t)H; a.Om = Om; a.ldom = ldom; a.Oc = Oc; a.ldoc = ldoc; a.LSE = LSE;
  a.xscale = scale; a.hd_live = hd_live;
  return a;
}

template <bool KL>
static int wattn_hd128_fwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                           const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float scale,
                           int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc,
                           float* LSE, void* stream) {
  const WAttnArgs a = wattn_hd128_args(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, scale, hd_live, p, seed, site,
                                       b_offset, Om, ldom, Oc, ldoc, LSE);
  const int lds[8] = {ldqm, ldqc, ldkm, ldkc, ldvm, ldvc, ldom, ldoc};
  return wattn_hd128<KL>(prec, false, a, p, b_offset, lds, 8, stream);
}

template <bool KL>
static int wattn_hd128_bwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                           const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, const float* Om, int ldom, const float* Oc,
                           int ldoc, const float* LSE, const float* dOm, int lddom, const float* dOc, int lddoc, int B, int H, int L, int hd,
                           float scale, int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQm, float* dQc,
                           float* dKm, float* dKc, float* dVm, float* dVc, int ldd, void* stream) {
  WAttnArgs a = wattn_hd128_args(Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, scale, hd_live, p, seed, site,
                                 b_offset, const_cast<float*>(Om), ldom, const_cast<float*>(Oc), ldoc, const_cast<float*>(LSE));
  a.dOm = dOm; a.lddom = lddom; a.dOc = dOc; a.lddoc = lddoc;
  a.dQm = dQm; a.dQc = dQc; a.dKm = dKm; a.dKc = dKc; a.dVm = dVm; a.dVc = dVc; a.ldd = ldd;
  const int lds[11] = {ldqm, ldqc, ldkm, ldkc, ldvm, ldvc, ldom, ldoc, lddom, lddoc, ldd};
  return wattn_hd128<KL>(prec, true, a, p, b_offset, lds, 11, stream);
}

extern "C" {

int adt_wattn_hd128_fwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                        const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float scale,
                        int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc,
                        float* LSE, void* stream) {
  return wattn_hd128_fwd<false>(prec, Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, scale, hd_live, p, seed, site,
                                b_offset, Om, ldom, Oc, ldoc, LSE, stream);
}

int adt_wattn_hd128_bwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                        const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, const float* Om, int ldom, const float* Oc,
                        int ldoc, const float* LSE, const float* dOm, int lddom, const float* dOc, int lddoc, int B, int H, int L, int hd,
                        float scale, int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQm, float* dQc,
                        float* dKm, float* dKc, float* dVm, float* dVc, int ldd, void* stream) {
  return wattn_hd128_bwd<false>(prec, Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, Om, ldom, Oc, ldoc, LSE, dOm, lddom, dOc,
                                lddoc, B, H, L, hd, scale, hd_live, p, seed, site, b_offset, dQm, dQc, dKm, dKc, dVm, dVc, ldd, stream);
}

int adt_klattn_hd128_fwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                         const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, int B, int H, int L, int hd, float scale,
                         int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* Om, int ldom, float* Oc, int ldoc,
                         float* LSE, void* stream) {
  return wattn_hd128_fwd<true>(prec, Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, B, H, L, hd, scale, hd_live, p, seed, site,
                               b_offset, Om, ldom, Oc, ldoc, LSE, stream);
}

int adt_klattn_hd128_bwd(int prec, const float* Qm, int ldqm, const float* Qc, int ldqc, const float* Km, int ldkm, const float* Kc, int ldkc,
                         const float* Vm, int ldvm, const float* Vc, int ldvc, const int32_t* key_ids, const float* Om, int ldom, const float* Oc,
                         int ldoc, const float* LSE, const float* dOm, int lddom, const float* dOc, int lddoc, int B, int H, int L, int hd,
                         float scale, int hd_live, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQm, float* dQc,
                         float* dKm, float* dKc, float* dVm, float* dVc, int ldd, void* stream) {
  return wattn_hd128_bwd<true>(prec, Qm, ldqm, Qc, ldqc, Km, ldkm, Kc, ldkc, Vm, ldvm, Vc, ldvc, key_ids, Om, ldom, Oc, ldoc, LSE, dOm, lddom, dOc,
                               lddoc, B, H, L, hd, scale, hd_live, p, seed, site, b_offset, dQm, dQc, dKm, dKc, dVm, dVc, ldd, stream);
}

}  // extern "C"
