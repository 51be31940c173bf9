// C ABI (include/adt_hip.h, "full-catalogue ranking"): launch wrappers of adt_fullrank.cuh.  Host code only enqueues work on the
// caller's stream.
#include "adt_host.h"

#include "adt_fullrank.cuh"
#include "adt_fullstats.cuh"
#include "adt_wdist_pack.cuh"
#include "adt_kldist_groups.cuh"
#include "adt_klrow_pack.cuh"

using namespace adt;

// The split count and the items per split, from the shape alone.  Automatic: about two workgroups per CU (512) over the tiles of 16
// users, every split at least two chunks long, at most 64 splits.  The range per split is a whole number of chunks, and splits that
// would be empty are dropped, so S <= the request.
static int fr_plan(int B, int n_items, int splits, int* S_out, int* per_out) {
  const int tiles = (B + 15) / 16, total = n_items + 1;
  int S = splits;
  if (S <= 0) {
    S = (512 + tiles - 1) / tiles;
    const int most = total / (2 * FR_CH);
    if (S > most) S = most;
    if (S > 64) S = 64;
    if (S < 1) S = 1;
  }
  int per = ((total + S - 1) / S + FR_CH - 1) / FR_CH * FR_CH;
  S = (total + per - 1) / per;
  *S_out = S;
  *per_out = per;
  return 0;
}

static int64_t fr_ws_bytes(int B, int S, int K) { return (int64_t)B * S * (8 + 8 * (int64_t)K); }

extern "C" {

int64_t adt_full_rank_ws_bytes(int B, int n_items, int K, int splits) {
  if (B < 1 || n_items < 1 || K < 0 || K > FR_KMAX || splits < 0 || splits > 1024) return 0;
  int S, per;
  fr_plan(B, n_items, splits, &S, &per);
  return fr_ws_bytes(B, S, K);
}

// What every entry point asks of its arguments, then the plan and the argument block.  `what` names the entry point in the messages;
// seen_ptr is its CSR offsets (int32 indptr or int64 seen_off).  1: nothing to do (B <= 0), 0: *a and *smem are ready, -1: an error.
static int fr_prepare(const char* what, const float* F, int ldf, const float* E, int lde, const float* bias, int B, int d, int n_items, int first_id,
                      const int32_t* target, const void* seen_ptr, const int32_t* indices, int K, int splits, void* ws, int64_t ws_bytes, int32_t* rank,
                      int32_t* n_elig, int32_t* top_idx, float* top_val, FullRankArgs* out, size_t* smem_out) {
  if (first_id != 0 && first_id != 1) return adt_set_error("%s: first_id=%d must be 0 or 1", what, first_id);
  if (K < 0 || K > FR_KMAX) return adt_set_error("%s: K=%d outside 0..%d", what, K, FR_KMAX);
  if (d < 4 || (d % 4)) return adt_set_error("%s: d=%d must be a positive multiple of 4", what, d);
  if (lde < d || ldf < d) return adt_set_error("%s: lde=%d, ldf=%d must be >= d=%d", what, lde, ldf, d);
  if (n_items < 1) return adt_set_error("%s: n_items=%d < 1", what, n_items);
  if ((lde % 4) || (ldf % 4) || !adt_aligned16(F) || !adt_aligned16(E)) return adt_set_error("%s: F and E must be 16-byte aligned with ld %% 4 == 0", what);
  if ((seen_ptr == nullptr) != (indices == nullptr)) return adt_set_error("%s: indptr and indices go together", what);
  if (splits < 0 || splits > 1024) return adt_set_error("%s: splits=%d outside 0..1024", what, splits);
  if (B <= 0) return 1;
  if (!rank || !n_elig || (K > 0 && (!top_idx || !top_val))) return adt_set_error("%s: missing output", what);
  const size_t smem = full_rank_lds_bytes(d);
  if (smem > ADT_LDS_MAX) return adt_set_error("%s: d=%d needs %zu B of LDS (> 160 KB)", what, d, smem);
  FullRankArgs a{};
  fr_plan(B, n_items, splits, &a.S, &a.per);
  if (!ws || ws_bytes < fr_ws_bytes(B, a.S, K))
    return adt_set_error("%s: workspace of %lld B, need %lld (adt_full_rank_ws_bytes)", what, (long long)ws_bytes, (long long)fr_ws_bytes(B, a.S, K));
  a.F = F; a.ldf = ldf; a.E = E; a.lde = lde; a.bias = bias; a.B = B; a.d = d; a.n_items = n_items; a.first_id = first_id;
  a.target = target; a.indices = indices; a.K = K;
  a.ws_cnt = static_cast<int32_t*>(ws);
  a.ws_val = reinterpret_cast<float*>(a.ws_cnt + (size_t)B * a.S * 2);
  a.ws_idx = reinterpret_cast<int32_t*>(a.ws_val + (size_t)B * a.S * K);
  a.rank = rank; a.n_elig = n_elig; a.top_idx = top_idx; a.top_val = top_val;
  *out = a;
  *smem_out = smem;
  return 0;
}

int adt_full_rank_from(const float* F, int ldf, const float* E, int lde, const float* bias, int B, int d, int n_items, int first_id,
                       const int32_t* target, const int32_t* indptr, const int32_t* indices, int K, int splits, void* ws, int64_t ws_bytes,
                       int32_t* rank, int32_t* n_elig, int32_t* top_idx, float* top_val, void* stream) {
  FullRankArgs a;
  size_t smem;
  const int st = fr_prepare("full_rank", F, ldf, E, lde, bias, B, d, n_items, first_id, target, indptr, indices, K, splits, ws, ws_bytes, rank, n_elig,
                            top_idx, top_val, &a, &smem);
  if (st) return st < 0 ? -1 : 0;
  a.indptr = indptr;
  static AdtLdsOptIn optin;      // smem follows d: the high-water mark in optin follows it
  if (adt_launch_lds1((const void*)k_full_rank<false>, dim3((B + 15) / 16, a.S), dim3(FR_NTH), smem, a, (hipStream_t)stream, "full_rank", optin)) return -1;
  hipLaunchKernelGGL(k_full_rank_merge<false>, dim3((B + FR_NW - 1) / FR_NW), dim3(FR_NTH), 0, (hipStream_t)stream, a);
  return adt_check_launch("full_rank(merge)");
}

int adt_full_rank_groups(const float* F, int ldf, const float* E, int lde, const float* bias, int n_rows, int rows_per_group, int d, int n_items,
                         int first_id, const int32_t* target, const int64_t* seen_off, const int32_t* seen_items, int n_total, int row0, int K,
                         int splits, void* ws, int64_t ws_bytes, int32_t* rank, int32_t* n_elig, int32_t* top_idx, float* top_val, void* stream) {
  const int R = rows_per_group;
  if (R < 1) return adt_set_error("full_rank_groups: rows_per_group=%d < 1", R);
  if (n_rows < 0 || n_rows % R != 0) return adt_set_error("full_rank_groups: n_rows=%d is not a multiple of rows_per_group=%d", n_rows, R);
  if (row0 < 0 || (int64_t)row0 + R > (int64_t)n_total)
    return adt_set_error("full_rank_groups: rows %d .. %d + %d lie outside the %d rows of the seen lists", row0, row0, R, n_total);
  FullRankGroupArgs a;
  size_t smem;
  const int st = fr_prepare("full_rank_groups", F, ldf, E, lde, bias, n_rows, d, n_items, first_id, target, seen_off, seen_items, K, splits, ws, ws_bytes,
                            rank, n_elig, top_idx, top_val, &a, &smem);
  if (st) return st < 0 ? -1 : 0;
  a.R = R; a.row0 = row0; a.off = seen_off;
  static AdtLdsOptIn optin;      // smem follows d: the high-water mark in optin follows it
  if (adt_launch_lds1((const void*)k_full_rank<true>, dim3((n_rows + 15) / 16, a.S), dim3(FR_NTH), smem, a, (hipStream_t)stream, "full_rank_groups", optin))
    return -1;
  hipLaunchKernelGGL(k_full_rank_merge<true>, dim3((n_rows + FR_NW - 1) / FR_NW), dim3(FR_NTH), 0, (hipStream_t)stream, a);
  return adt_check_launch("full_rank_groups(merge)");
}

int adt_full_rank_stats(const int32_t* rank, const int32_t* n_elig, int n_rows, int rows_per_group, int kh, int64_t* hist, double* auc,
                        void* stream) {
  if (kh < 1 || kh > ADT_FULLSTATS_MAX_KH) return adt_set_error("full_rank_stats: kh=%d outside 1..%d", kh, ADT_FULLSTATS_MAX_KH);
  if (rows_per_group < 1) return adt_set_error("full_rank_stats: rows_per_group=%d < 1", rows_per_group);
  if (n_rows < 0 || n_rows % rows_per_group != 0)
    return adt_set_error("full_rank_stats: n_rows=%d is not a multiple of rows_per_group=%d", n_rows, rows_per_group);
  if (!rank || !n_elig || !hist || !auc) return adt_set_error("full_rank_stats: NULL rank, n_elig, hist or auc");
  if (n_rows == 0) return 0;
  FullStatsArgs a{rank, n_elig, rows_per_group, kh, hist, auc};
  hipLaunchKernelGGL(k_full_rank_stats, dim3(n_rows / rows_per_group), dim3(ADT_FULLSTATS_NTH), 0, (hipStream_t)stream, a);
  return adt_check_launch("full_rank_stats");
}

int adt_full_rank(const float* F, int ldf, const float* E, int lde, const float* bias, int B, int d, int n_items, const int32_t* target,
                  const int32_t* indptr, const int32_t* indices, int K, int splits, void* ws, int64_t ws_bytes, int32_t* rank,
                  int32_t* n_elig, int32_t* top_idx, float* top_val, void* stream) {
  return adt_full_rank_from(F, ldf, E, lde, bias, B, d, n_items, 1, target, indptr, indices, K, splits, ws, ws_bytes, rank, n_elig, top_idx,
                            top_val, stream);
}

int adt_wdist_pack(const float* M, const float* C, int ld, int rows, int d, int elu, float* img, int ldi, float* nrm, float nrm_scale,
                   void* stream) {
  if (d < 4 || (d % 4)) return adt_set_error("wdist_pack: d=%d must be a positive multiple of 4", d);
  if (ld < d || ldi < 2 * d) return adt_set_error("wdist_pack: ld=%d must be >= d=%d and ldi=%d >= 2d", ld, d, ldi);
  if ((ld % 4) || (ldi % 4) || !adt_aligned16(M) || !adt_aligned16(C) || !adt_aligned16(img))
    return adt_set_error("wdist_pack: M, C and img must be 16-byte aligned with ld %% 4 == 0 and ldi %% 4 == 0");
  if (rows <= 0) return 0;
  if (!M || !C || !img || !nrm) return adt_set_error("wdist_pack: missing operand");
  WPackArgs a{M, C, ld, rows, d, elu != 0, img, ldi, nrm, nrm_scale};
  hipLaunchKernelGGL(k_wdist_pack<false>, dim3(adt_grid_for((size_t)rows, 16, 4096)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("wdist_pack");
}

// adt_wdist_pack on padded rows (d_pad = H * hd_pad columns): the pad lanes of both halves of the image are +0.0 and stay out of the norm
int adt_wdist_pack_lanes(const float* M, const float* C, int ld, int rows, int H, int hd, int hd_pad, int elu, float* img, int ldi, float* nrm,
                         float nrm_scale, void* stream) {
  const int d = H * hd_pad;
  WPackArgs a{M, C, ld, rows, d, elu != 0, img, ldi, nrm, nrm_scale};
  if (adt_make_lanes(a.ln, H, hd, hd_pad, "wdist_pack_lanes")) return -1;
  if (ld < d || ldi < 2 * d) return adt_set_error("wdist_pack_lanes: ld=%d must be >= d_pad=%d and ldi=%d >= 2 d_pad", ld, d, ldi);
  if ((ld % 4) || (ldi % 4) || !adt_aligned16(M) || !adt_aligned16(C) || !adt_aligned16(img))
    return adt_set_error("wdist_pack_lanes: M, C and img must be 16-byte aligned with ld %% 4 == 0 and ldi %% 4 == 0");
  if (rows <= 0) return 0;
  if (!M || !C || !img || !nrm) return adt_set_error("wdist_pack_lanes: missing operand");
  hipLaunchKernelGGL(k_wdist_pack<true>, dim3(adt_grid_for((size_t)rows, 16, 4096)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("wdist_pack_lanes");
}

int adt_kldist_pack(const float* Em, const float* Ec, int ld, int V, int d, float* img, int ldi, float* lv, void* stream) {
  if (d < 4 || (d % 4)) return adt_set_error("kldist_pack: d=%d must be a positive multiple of 4", d);
  if (ld < d || ldi < 2 * d) return adt_set_error("kldist_pack: ld=%d must be >= d=%d and ldi=%d >= 2d", ld, d, ldi);
  if ((ld % 4) || (ldi % 4) || !adt_aligned16(Em) || !adt_aligned16(Ec) || !adt_aligned16(img))
    return adt_set_error("kldist_pack: Em, Ec and img must be 16-byte aligned with ld %% 4 == 0 and ldi %% 4 == 0");
  if (V <= 0) return 0;
  if (!Em || !Ec || !img || !lv) return adt_set_error("kldist_pack: missing operand");
  KlPackArgs a{Em, Ec, ld, V, d, img, ldi, lv};
  hipLaunchKernelGGL(k_kldist_pack, dim3(adt_grid_for((size_t)V, 16, 4096)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("kldist_pack");
}

int adt_klrow_pack(const float* M, const float* C, int ld, int rows, int d, int items, float* img, int ldi, float* off, void* stream) {
  if (items != 0 && items != 1) return adt_set_error("klrow_pack: items=%d must be 0 (user states) or 1 (item tables)", items);
  if (d < 4 || (d % 4)) return adt_set_error("klrow_pack: d=%d must be a positive multiple of 4", d);
  if (ld < d || ldi < 2 * d) return adt_set_error("klrow_pack: ld=%d must be >= d=%d and ldi=%d >= 2d", ld, d, ldi);
  if ((ld % 4) || (ldi % 4) || !adt_aligned16(M) || !adt_aligned16(C) || !adt_aligned16(img))
    return adt_set_error("klrow_pack: M, C and img must be 16-byte aligned with ld %% 4 == 0 and ldi %% 4 == 0");
  if (rows <= 0) return 0;
  if (!M || !C || !img || !off) return adt_set_error("klrow_pack: missing operand");
  KlRowPackArgs a{M, C, ld, rows, d, items, img, ldi, off};
  hipLaunchKernelGGL(k_klrow_pack<false>, dim3(adt_grid_for((size_t)rows, 16, 4096)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("klrow_pack");
}

// adt_klrow_pack on padded rows (d_pad = H * hd_pad columns): the pad lanes of both halves of the image are +0.0 and stay out of off[r],
// which takes the true d = H * hd
int adt_klrow_pack_lanes(const float* M, const float* C, int ld, int rows, int H, int hd, int hd_pad, int items, float* img, int ldi, float* off,
                         void* stream) {
  if (items != 0 && items != 1) return adt_set_error("klrow_pack_lanes: items=%d must be 0 (user states) or 1 (item tables)", items);
  const int d = H * hd_pad;
  KlRowPackArgs a{M, C, ld, rows, d, items, img, ldi, off};
  if (adt_make_lanes(a.ln, H, hd, hd_pad, "klrow_pack_lanes")) return -1;
  if (ld < d || ldi < 2 * d) return adt_set_error("klrow_pack_lanes: ld=%d must be >= d_pad=%d and ldi=%d >= 2 d_pad", ld, d, ldi);
  if ((ld % 4) || (ldi % 4) || !adt_aligned16(M) || !adt_aligned16(C) || !adt_aligned16(img))
    return adt_set_error("klrow_pack_lanes: M, C and img must be 16-byte aligned with ld %% 4 == 0 and ldi %% 4 == 0");
  if (rows <= 0) return 0;
  if (!M || !C || !img || !off) return adt_set_error("klrow_pack_lanes: missing operand");
  hipLaunchKernelGGL(k_klrow_pack<true>, dim3(adt_grid_for((size_t)rows, 16, 4096)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("klrow_pack_lanes");
}

int adt_kldist_full_groups(const float* Sm, const float* Sc, int lds, const float* img, int ldi, const float* lv, int rows, int E, int V, int d,
                           float* dist, int ldo, void* stream) {
  if (!Sm || !Sc || !img || !lv || !dist) return adt_set_error("kldist_full_groups: missing operand");
  if (d < 4 || (d % 4)) return adt_set_error("kldist_full_groups: d=%d must be a positive multiple of 4", d);
  if (E < 1) return adt_set_error("kldist_full_groups: E=%d < 1", E);
  if (rows < 0 || rows % E) return adt_set_error("kldist_full_groups: rows=%d is not a multiple of E=%d", rows, E);
  if (V < 0 || lds < d || ldi < 2 * d || ldo < V) return adt_set_error("kldist_full_groups: lds=%d must be >= d=%d, ldi=%d >= 2d, ldo=%d >= V=%d >= 0", lds, d, ldi, ldo, V);
  if ((lds % 4) || (ldi % 4) || !adt_aligned16(Sm) || !adt_aligned16(Sc) || !adt_aligned16(img))
    return adt_set_error("kldist_full_groups: Sm, Sc and img must be 16-byte aligned with lds %% 4 == 0 and ldi %% 4 == 0");
  if ((int64_t)V + 2 * (int64_t)E + 32 > 0x7fffffff) return adt_set_error("kldist_full_groups: V=%d + 2 E=%d + 32 exceeds the item index range", V, E);
  if (rows == 0 || V == 0) return 0;
  const size_t smem = kldist_groups_lds_bytes(d);
  if (smem > ADT_LDS_MAX) return adt_set_error("kldist_full_groups: d=%d needs %zu B of LDS (> 160 KB)", d, smem);
  KlGroupsArgs a{Sm, Sc, lds, img, ldi, lv, rows, E, V, d, (E + 15) / 16, (V + E - 1) / E, dist, ldo};      // dist is indexed in size_t throughout
  const size_t wgs = (size_t)(rows / E) * a.nch * a.nt;
  if (wgs > 0x7fffffffu) return adt_set_error("kldist_full_groups: %zu workgroups (rows=%d, E=%d, V=%d) exceed the grid", wgs, rows, E, V);
  static AdtLdsOptIn optin;      // smem follows d: the high-water mark in optin follows it
  return adt_launch_lds1((const void*)k_kldist_full_groups, dim3((unsigned)wgs), dim3(256), smem, a, (hipStream_t)stream, "kldist_full_groups", optin);
}

}  // extern "C"
