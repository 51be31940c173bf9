// What every STOSA-ADT attention kernel shares (adt_stosa.cuh, adt_klattn.cuh, adt_wattn_mfma.cuh, adt_wattn_long.cuh): the argument block,
// the additive mask with its dead-row rule, and the whole-(b, h) kernels' LDS footprint.  No kernels here: adt_stosa.cuh's are not
// templates, so only one translation unit (adt_wide.hip) may include that header; the others take this one.
#pragma once
#include "adt_common.cuh"

namespace adt {

struct WAttnArgs {
  const float* Qm; int ldqm; const float* Qc; int ldqc;   // query mean / covariance (T x >= H*hd), cov = ELU(.)+1 already
  const float* Km; int ldkm; const float* Kc; int ldkc;
  const float* Vm; int ldvm; const float* Vc; int ldvc;
  const int* kid;            // (B*L) ids of the KEY sequence: key j is padding when kid <= 0
  int B, H, L, hd;
  float scale;               // 1/sqrt(hd) (unused: the kernels divide, like the reference)
  DropCfg drop; uint32_t bh_offset;     // idx = ((bh + bh_offset) * L + i) * L + j
  float* Om; int ldom; float* Oc; int ldoc;   // contexts (T x H*hd)
  float* LSE;                // (B*H*L)
  const float* dOm; int lddom; const float* dOc; int lddoc;
  float *dQm, *dQc, *dKm, *dKc, *dVm, *dVc; int ldd;   // gradients (T x ldd), overwritten
  // Padded heads (the adt_wattn_*_scaled_* entry points; both 0 everywhere else): xscale > 0 replaces 1 / sqrt(hd) as the score scale in
  // the forward and both backward passes alike; hd_live > 0: only lanes [0, hd_live) of a head are live, the zero pad lanes above them
  // get a +0.0 gradient (sum(cov) has gradient 1 at cov = 0, so dQc / dKc would otherwise carry sum_j dW there).
  float xscale; int hd_live;
};

constexpr float W_MASK = -4294967296.0f;   // float32(-2**32 + 1), stosa/models.py:226,230
constexpr int W_KPL = 4;                    // keys per lane: L <= 256

static inline size_t wattn_lds_bytes(int L, int hd, bool bwd) {
  // 4 resident tensors [L][hd+1], 2 row vectors [L] (+ 2 more in the backward), per-wave scratch 4 x (3*L' + 4*hd)
  const int Lp = (L + 63) / 64 * 64;
  size_t f = (size_t)4 * L * (hd + 1) + (size_t)(bwd ? 4 : 2) * Lp + (size_t)4 * (3 * Lp + 4 * hd);
  return f * sizeof(float);
}

// A query with no attendable key (the left-padded prefix) has EVERY score shifted by the mask: in fp32 x - 2^32 rounds to a
// multiple of 512, so all of them collapse to -2^32 and the row is uniform over all L keys.  -2^32 + log(L) is not
// representable, so such rows keep the reference's rounding but drop the common shift (softmax is shift-invariant and
// (x + MASK) - MASK is exact): probabilities and gradients are unchanged, the saved LSE stays accurate.
ADT_DEVICE_INLINE float w_score(float x, bool masked, bool dead_row) {
  if (dead_row) return (x + W_MASK) - W_MASK;
  return masked ? x + W_MASK : x;
}

}  // namespace adt
