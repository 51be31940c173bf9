// C ABI (include/adt_hip.h): masked attention at 1 <= L <= 1024 (the 1024-row instantiations of adt_attn_long.cuh), every head size, either
// precision.  A translation unit of its own, compiled beside adt_wide.hip.  Host code only enqueues work on the caller's stream.
#include "adt_attn_long_launch.h"

using namespace adt;

static_assert(PREC_F32 == ADT_PREC_F32 && PREC_BF16 == ADT_PREC_BF16, "adt_wide_plan.h speaks of the ABI's prec values");
static_assert(attn_long_lds(ADT_PREC_F32, 256, attn_streamed_kc(ADT_PREC_F32, true), true, ATTN_LONG_LMAX) <= ADT_LDS_MAX, "the tightest instantiation fits the LDS");

template <int PREC>
static int launch_attn_long_hd(const AttnPlan& p, bool bwd, int hd, const AttnGenArgs& a, hipStream_t s) {
  const char *wf = "attn_long_fwd", *wb = "attn_long_bwd";
  if (hd == 16) return launch_attn_long<PREC, 16, ATTN_LONG_LMAX>(p, bwd, a, s, wf, wb);
  if (hd == 32) return launch_attn_long<PREC, 32, ATTN_LONG_LMAX>(p, bwd, a, s, wf, wb);
  if (hd == 64) return launch_attn_long<PREC, 64, ATTN_LONG_LMAX>(p, bwd, a, s, wf, wb);
  if (hd == 128) return launch_attn_long<PREC, 128, ATTN_LONG_LMAX>(p, bwd, a, s, wf, wb);
  return launch_attn_long<PREC, 256, ATTN_LONG_LMAX>(p, bwd, a, s, wf, wb);
}

// the checks and the argument block both directions share; the plan's refusals (head size, length, LDS) come first
static int attn_long_args(AttnGenArgs& g, AttnPlan& plan, const char* what, int prec, bool bwd, const float* Q, int ldq, const float* K, int ldk,
                          const float* V, int ldv, int B, int H, int L, int hd, float scale, int causal, const int32_t* kid, float fill, float p,
                          const uint32_t* seed, uint32_t site, uint32_t b_offset) {
  if (!(scale > 0.f)) return adt_set_error("%s: scale %g must be positive", what, (double)scale);
  plan = adt_attn_long_plan(prec, hd, L, bwd, causal != 0, kid != nullptr, fill);
  if (plan.error[0]) return adt_set_error("%s", plan.error);
  if (B <= 0 || H <= 0) return adt_set_error("%s: empty shape", what);
  if ((ldq % 4) || (ldk % 4) || (ldv % 4)) return adt_set_error("%s: ld %% 4", what);
  // the dropout element index ((b_offset + b) * H + h) * L * L + q * L + key is a uint32: past 2^32 two elements would share a draw
  if (p > 0.f && ((uint64_t)b_offset + (uint64_t)B) * (uint64_t)H * (uint64_t)L * (uint64_t)L > (1ull << 32))
    return adt_set_error("%s: dropout index space (b_offset + B) * H * L * L = (%u + %d) * %d * %d * %d exceeds 2^32", what, b_offset, B, H, L, L);
  g.a.Q = Q; g.a.ldq = ldq; g.a.K = K; g.a.ldk = ldk; g.a.V = V; g.a.ldv = ldv; g.a.B = B; g.a.H = H; g.a.L = L; g.a.causal = causal;
  g.a.scale = scale; g.a.drop = adt_make_drop(p, seed, site); g.a.bh_offset = b_offset * (uint32_t)H;
  g.kid = kid; g.fill = fill;
  return 0;
}

extern "C" {

int adt_attn_masked_max_len(int hd) { return adt::adt_attn_masked_max_len(hd); }

int adt_attn_long_fwd(int prec, const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, int B, int H, int L, int hd, float scale,
                      int causal, const int32_t* key_ids, float fill, float p, const uint32_t* seed, uint32_t site, uint32_t b_offset, float* O,
                      int ldo, float* LSE, void* stream) {
  AttnGenArgs g{};
  AttnPlan plan;
  if (attn_long_args(g, plan, "attn_long_fwd", prec, false, Q, ldq, K, ldk, V, ldv, B, H, L, hd, scale, causal, key_ids, fill, p, seed, site, b_offset))
    return -1;
  g.a.O = O; g.a.ldo = ldo; g.a.LSE = LSE;
  return prec == ADT_PREC_F32 ? launch_attn_long_hd<PREC_F32>(plan, false, hd, g, (hipStream_t)stream)
                              : launch_attn_long_hd<PREC_BF16>(plan, false, hd, g, (hipStream_t)stream);
}

int adt_attn_long_bwd(int prec, const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, const float* O, int ldo, const float* LSE,
                      const float* dO, int lddo, int B, int H, int L, int hd, float scale, int causal, const int32_t* key_ids, float fill, float p,
                      const uint32_t* seed, uint32_t site, uint32_t b_offset, float* dQ, int lddq, float* dK, int lddk, float* dV, int lddv,
                      void* stream) {
  AttnGenArgs g{};
  AttnPlan plan;
  if (attn_long_args(g, plan, "attn_long_bwd", prec, true, Q, ldq, K, ldk, V, ldv, B, H, L, hd, scale, causal, key_ids, fill, p, seed, site, b_offset))
    return -1;
  if ((ldo % 4) || (lddo % 4) || (lddq % 4) || (lddk % 4) || (lddv % 4)) return adt_set_error("attn_long_bwd: ld %% 4");
  g.a.O = const_cast<float*>(O); g.a.ldo = ldo; g.a.LSE = const_cast<float*>(LSE); g.a.dO = dO; g.a.lddo = lddo;
  g.a.dQ = dQ; g.a.lddq = lddq; g.a.dK = dK; g.a.lddk = lddk; g.a.dV = dV; g.a.lddv = lddv;
  return prec == ADT_PREC_F32 ? launch_attn_long_hd<PREC_F32>(plan, true, hd, g, (hipStream_t)stream)
                              : launch_attn_long_hd<PREC_BF16>(plan, true, hd, g, (hipStream_t)stream);
}

}  // extern "C"
