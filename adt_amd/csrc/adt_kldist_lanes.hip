// C ABI (include/adt_hip.h, "grouped KL full sort on padded rows"): launch wrappers of adt_kldist_groups_lanes.cuh.  A translation unit of
// its own, so that the code objects of adt_fullrank.hip stay what they are.  Host code only enqueues work on the caller's stream.
#include "adt_host.h"

#include "adt_kldist_groups_lanes.cuh"

using namespace adt;

extern "C" {

int adt_kldist_pack_lanes(const float* Em, const float* Ec, int ld, int V, int d, int H, int hd, int hd_pad, float* img, int ldi, float* lv,
                          void* stream) {
  KlPackLanesArgs a{Em, Ec, ld, V, d, img, ldi, lv};
  if (adt_make_lanes(a.ln, H, hd, hd_pad, "kldist_pack_lanes")) return -1;
  if (d != H * hd_pad) return adt_set_error("kldist_pack_lanes: d=%d is not the padded row H * hd_pad = %d * %d", d, H, hd_pad);
  if (ld < d || ldi < 2 * d) return adt_set_error("kldist_pack_lanes: ld=%d must be >= d_pad=%d and ldi=%d >= 2 d_pad", ld, d, ldi);
  if ((ld % 4) || (ldi % 4) || !adt_aligned16(Em) || !adt_aligned16(Ec) || !adt_aligned16(img))
    return adt_set_error("kldist_pack_lanes: Em, Ec and img must be 16-byte aligned with ld %% 4 == 0 and ldi %% 4 == 0");
  if (V <= 0) return 0;
  if (!Em || !Ec || !img || !lv) return adt_set_error("kldist_pack_lanes: missing operand");
  hipLaunchKernelGGL(k_kldist_pack_lanes, dim3(adt_grid_for((size_t)V, 16, 4096)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("kldist_pack_lanes");
}

int adt_kldist_full_groups_lanes(const float* Sm, const float* Sc, int lds, const float* img, int ldi, const float* lv, int rows, int E, int V,
                                 int d, int H, int hd, int hd_pad, float* dist, int ldo, void* stream) {
  if (!Sm || !Sc || !img || !lv || !dist) return adt_set_error("kldist_full_groups_lanes: missing operand");
  Lanes ln;
  if (adt_make_lanes(ln, H, hd, hd_pad, "kldist_full_groups_lanes")) return -1;      // H * hd_pad in {64, 128, 192, 256}
  if (d != H * hd_pad) return adt_set_error("kldist_full_groups_lanes: d=%d is not the padded row H * hd_pad = %d * %d", d, H, hd_pad);
  if (E < 1) return adt_set_error("kldist_full_groups_lanes: E=%d < 1", E);
  if (rows < 0 || rows % E) return adt_set_error("kldist_full_groups_lanes: rows=%d is not a multiple of E=%d", rows, E);
  if (V < 0 || lds < d || ldi < 2 * d || ldo < V)
    return adt_set_error("kldist_full_groups_lanes: lds=%d must be >= d_pad=%d, ldi=%d >= 2 d_pad, ldo=%d >= V=%d >= 0", lds, d, ldi, ldo, V);
  if ((lds % 4) || (ldi % 4) || !adt_aligned16(Sm) || !adt_aligned16(Sc) || !adt_aligned16(img))
    return adt_set_error("kldist_full_groups_lanes: Sm, Sc and img must be 16-byte aligned with lds %% 4 == 0 and ldi %% 4 == 0");
  if ((int64_t)V + 2 * (int64_t)E + 32 > 0x7fffffff)
    return adt_set_error("kldist_full_groups_lanes: V=%d + 2 E=%d + 32 exceeds the item index range", V, E);
  if (rows == 0 || V == 0) return 0;
  const size_t smem = kldist_groups_lanes_lds_bytes(d);      // at most 33,088 B (d_pad 256)
  KlGroupsLanesArgs a{Sm, Sc, lds, img, ldi, lv, rows, E, V, d, (E + 15) / 16, (V + E - 1) / E, dist, ldo, ln};      // dist is indexed in size_t throughout
  const size_t wgs = (size_t)(rows / E) * a.nch * a.nt;
  if (wgs > 0x7fffffffu) return adt_set_error("kldist_full_groups_lanes: %zu workgroups (rows=%d, E=%d, V=%d) exceed the grid", wgs, rows, E, V);
  static AdtLdsOptIn optin;      // smem follows d: the high-water mark in optin follows it
  return adt_launch_lds1((const void*)k_kldist_full_groups_lanes, dim3((unsigned)wgs), dim3(256), smem, a, (hipStream_t)stream,
                         "kldist_full_groups_lanes", optin);
}

}  // extern "C"
