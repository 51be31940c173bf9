// The one launcher of the streamed masked attention (adt_attn_long.cuh), shared by adt_attn_masked_* (adt_wide.hip, LMAX 256) and
// adt_attn_long_* (adt_attn_long.hip, LMAX 1024).  The plan (adt_wide_plan.h: attn_streamed_plan) chooses the grid and the footprint; this
// names the instantiation.  One LDS opt-in per instantiation and direction.
#pragma once
#include "adt_host.h"

#include "adt_attn_long.cuh"

template <int PREC, int HD, int LMAX>
static int launch_attn_long(const adt::AttnPlan& p, bool bwd, const adt::AttnGenArgs& a, hipStream_t s, const char* what_fwd, const char* what_bwd) {
  using namespace adt;
  constexpr int NW = ATTN_STREAMED_NW, KCF = attn_streamed_kc(PREC, false), KCB = attn_streamed_kc(PREC, true);
  static_assert(attn_long_lds(PREC, HD, KCF, false, LMAX) == AttnLongLds<PREC, HD, KCF, LMAX>::fwd_bytes, "plan and kernel disagree on the LDS footprint");
  static_assert(attn_long_lds(PREC, HD, KCB, true, LMAX) == AttnLongLds<PREC, HD, KCB, LMAX>::bwd_bytes, "plan and kernel disagree on the LDS footprint");
  const void* fn = bwd ? (const void*)k_attn_long_bwd<PREC, HD, NW, KCB, LMAX> : (const void*)k_attn_long_fwd<PREC, HD, NW, KCF, LMAX>;
  static AdtLdsOptIn optin[2];
  return adt_launch_lds1(fn, dim3(a.a.B * a.a.H, p.grid_y), dim3(p.waves * 64), p.lds_bytes, a, s, bwd ? what_bwd : what_fwd, optin[bwd ? 1 : 0]);
}
