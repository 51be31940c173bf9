// C ABI (include/adt_hip.h, "STOSA-ADT batches built on the device", "full-sort scores on the device", "BERT4Rec-ADT batches masked and
// built on the device" and "SASRec-ADT evaluation candidates drawn on the device"): launch wrappers of adt_seqbatch.cuh, adt_hithist.cuh,
// adt_bertbatch.cuh and adt_evalcand.cuh, and the host-side draws.  Host code only enqueues work on the caller's stream.
#include "adt_host.h"

#include "adt_bertbatch.cuh"
#include "adt_evalcand.cuh"
#include "adt_hithist.cuh"
#include "adt_seqbatch.cuh"

using namespace adt;

extern "C" {

int adt_seqbatch_draw(uint32_t seed, uint32_t step, int row, int t, int attempt, int item_size) {
  if (item_size < 2 || row < 0 || t < 0 || attempt < 0) return 0;
  return adt_seqbatch_draw_id(seed, step, (uint32_t)row, (uint32_t)t, (uint32_t)attempt, (uint32_t)item_size);
}

int adt_seqbatch_build(const int64_t* seq_off, const int32_t* seq_items, const int64_t* set_off, const int32_t* set_items, const int32_t* users,
                       int n_users, int row0, int n_rows, int L, int cut, int item_size, uint32_t seed, uint32_t step, int32_t* inp, int32_t* dec,
                       int32_t* pos, int32_t* neg, float* inv_count, void* stream) {
  if (cut < 1 || cut > 3) return adt_set_error("seqbatch_build: cut=%d outside 1..3", cut);
  if (L < 1) return adt_set_error("seqbatch_build: L=%d < 1", L);
  if (item_size < 2) return adt_set_error("seqbatch_build: item_size=%d < 2", item_size);
  if (n_users < 0 || row0 < 0 || n_rows < 0 || (int64_t)row0 + n_rows > n_users)
    return adt_set_error("seqbatch_build: rows %d..%d+%d outside the batch of %d users", row0, row0, n_rows, n_users);
  if (!seq_off || !seq_items || !set_off || !set_items || !users) return adt_set_error("seqbatch_build: NULL input");
  const size_t work = (size_t)n_rows * (size_t)L;
  if (work > ((size_t)1 << 31)) return adt_set_error("seqbatch_build: %d rows x L=%d is more than 2^31 positions", n_rows, L);
  if (n_rows > 0 && !inp) return adt_set_error("seqbatch_build: inp is NULL");
  SeqBatchArgs a{seq_off, seq_items, set_off, set_items, users, n_users, row0, n_rows, L, cut, (uint32_t)item_size, seed, step, inp, dec, pos, neg,
                 inv_count};
  if (n_rows > 0) {
    hipLaunchKernelGGL(k_seqbatch_build, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    if (adt_check_launch("seqbatch_build")) return -1;
  }
  if (inv_count) {
    hipLaunchKernelGGL(k_seqbatch_count, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    return adt_check_launch("seqbatch_build(count)");
  }
  return 0;
}

int adt_hit_hist(const int32_t* top_idx, int ld, int n_rows, int K, const int32_t* answers, int rows_per_group, int64_t* hist,
                 int32_t* hit_pos, void* stream) {
  if (K < 1 || K > ADT_HITHIST_MAX_K) return adt_set_error("hit_hist: K=%d outside 1..%d", K, ADT_HITHIST_MAX_K);
  if (ld < K) return adt_set_error("hit_hist: ld=%d < K=%d", ld, K);
  if (rows_per_group < 1) return adt_set_error("hit_hist: rows_per_group=%d < 1", rows_per_group);
  if (n_rows < 0 || n_rows % rows_per_group != 0)
    return adt_set_error("hit_hist: n_rows=%d is not a multiple of rows_per_group=%d", n_rows, rows_per_group);
  if (n_rows == 0) return 0;      // nothing to count: the pointers are not looked at (an empty tensor has none)
  if (!top_idx || !answers || !hist) return adt_set_error("hit_hist: NULL top_idx, answers or hist");
  // 16 rows of a group per block (4 per wave) up to 256 blocks per group; beyond that the waves stride over the group's rows
  const int groups = n_rows / rows_per_group;
  int chunks = (rows_per_group + 4 * ADT_HITHIST_WAVES - 1) / (4 * ADT_HITHIST_WAVES);
  chunks = chunks > 256 ? 256 : chunks;
  const int64_t blocks = (int64_t)groups * chunks;      // <= n_rows
  HitHistArgs a{top_idx, ld, K, rows_per_group, chunks, answers, (unsigned long long*)hist, hit_pos};
  hipLaunchKernelGGL(k_hit_hist, dim3((unsigned)blocks), dim3(64 * ADT_HITHIST_WAVES), 0, (hipStream_t)stream, a);
  return adt_check_launch("hit_hist");
}

// what both evalcand entry points ask of the table's scalars (the table itself may be in device memory: `total` is the caller's word)
static int evalcand_check_table(const char* what, const void* cum, int n_ids, int64_t total) {
  if (!cum) return adt_set_error("%s: cum is NULL", what);
  if (n_ids < 1) return adt_set_error("%s: n_ids=%d < 1", what, n_ids);
  if (total < 1 || total >= ((int64_t)1 << 32)) return adt_set_error("%s: total=%lld outside 1 .. 2^32 - 1", what, (long long)total);
  return 0;
}

int adt_evalcand_stream(const int64_t* cum, int n_ids, uint32_t seed, uint32_t salt, int row, int n0, int n, int32_t* out) {
  if (evalcand_check_table("evalcand_stream", cum, n_ids, cum && n_ids >= 1 ? cum[n_ids] : 0)) return -1;
  if (row < 0 || n0 < 0 || n < 0 || (int64_t)n0 + n > (int64_t)INT32_MAX)
    return adt_set_error("evalcand_stream: row=%d, positions %d..%d+%d", row, n0, n0, n);
  if (n > 0 && !out) return adt_set_error("evalcand_stream: out is NULL");
  const uint32_t key = adt_evalcand_key(seed, salt, (uint32_t)row);
  for (int i = 0; i < n; ++i) out[i] = adt_evalcand_item_key(key, (uint32_t)(n0 + i), cum, n_ids, (uint32_t)cum[n_ids]);
  return 0;
}

int adt_evalcand_draw(const int64_t* cum, int n_ids, int64_t total, const int64_t* seen_off, const int32_t* seen_items, const int32_t* targets,
                      int n_total, int row0, int n_rows, int S, uint32_t seed, uint32_t salt, int32_t* cand, int ldc, int32_t* filled,
                      void* stream) {
  if (evalcand_check_table("evalcand_draw", cum, n_ids, total)) return -1;
  if (S < 1 || S > ADT_EVALCAND_MAX_S) return adt_set_error("evalcand_draw: S=%d outside 1..%d", S, ADT_EVALCAND_MAX_S);
  if (!seen_off || !seen_items || !targets) return adt_set_error("evalcand_draw: NULL seen_off, seen_items or targets");
  if (n_total < 0 || row0 < 0 || n_rows < 0 || (int64_t)row0 + n_rows > n_total)
    return adt_set_error("evalcand_draw: rows %d..%d+%d outside the list of %d users", row0, row0, n_rows, n_total);
  if (ldc < 1 + S) return adt_set_error("evalcand_draw: ldc=%d < 1 + S=%d", ldc, 1 + S);
  if (n_rows == 0) return 0;
  if (!cand) return adt_set_error("evalcand_draw: cand is NULL");
  EvalCandArgs a{cum, n_ids, (uint32_t)total, seen_off, seen_items, targets, row0, n_rows, S, seed, salt, cand, ldc, filled};
  hipLaunchKernelGGL(k_evalcand_draw, dim3((unsigned)n_rows), dim3(64), 0, (hipStream_t)stream, a);
  return adt_check_launch("evalcand_draw");
}

int adt_bertbatch_token(uint32_t seed, uint32_t salt, int example, int pos, uint32_t thr_mask, int itemnum, int item, int* masked) {
  bool m = false;
  int tok = item;
  if (itemnum >= 1 && example >= 0 && pos >= 0)
    tok = adt_bertbatch_rule(seed, salt, (uint32_t)example, (uint32_t)pos, thr_mask, (uint32_t)itemnum, item, &m);
  if (masked) *masked = m ? 1 : 0;
  return tok;
}

int adt_bertbatch_build(const int64_t* seq_off, const int32_t* seq_items, const int64_t* win_start, const int32_t* win_len,
                        const int32_t* examples, int n_examples, int row0, int n_rows, int L, int n_windows, int dupe, int n_users, int itemnum,
                        uint32_t seed, uint32_t salt, uint32_t thr_mask, int32_t* src, int32_t* dec, int32_t* labels, int32_t* rows,
                        int32_t* labels_c, int32_t* M, float* inv_count, int32_t* work, void* stream) {
  if (L < 1) return adt_set_error("bertbatch_build: L=%d < 1", L);
  if (itemnum < 1) return adt_set_error("bertbatch_build: itemnum=%d < 1", itemnum);
  if (dupe < 1 || n_windows < 0 || n_users < 0 || (int64_t)n_windows * dupe + n_users > (int64_t)INT32_MAX)
    return adt_set_error("bertbatch_build: %d windows x %d copies + %d users is not a count of examples below 2^31", n_windows, dupe, n_users);
  if (n_examples < 0 || row0 < 0 || n_rows < 0 || (int64_t)row0 + n_rows > n_examples)
    return adt_set_error("bertbatch_build: rows %d..%d+%d outside the batch of %d examples", row0, row0, n_rows, n_examples);
  if ((size_t)n_examples * (size_t)L >= ((size_t)1 << 31))
    return adt_set_error("bertbatch_build: %d examples x L=%d is 2^31 positions or more", n_examples, L);
  if (!seq_off || !seq_items || !win_start || !win_len || (n_examples > 0 && !examples)) return adt_set_error("bertbatch_build: NULL input");
  if (!M || !work) return adt_set_error("bertbatch_build: M or work is NULL");
  if (n_rows > 0 && (!src || !dec || !rows || !labels_c)) return adt_set_error("bertbatch_build: src, dec, rows or labels_c is NULL");
  BertBatchArgs a{seq_off, seq_items, win_start, win_len, examples, n_examples, row0, n_rows, L, n_windows, dupe, n_users, (uint32_t)itemnum,
                  seed, salt, thr_mask, src, dec, labels, rows, labels_c, M, inv_count, (uint32_t*)work};
  if (n_examples > 0) {
    hipLaunchKernelGGL(k_bertbatch_count, dim3((unsigned)((n_examples + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    if (adt_check_launch("bertbatch_build(count)")) return -1;
  }
  hipLaunchKernelGGL(k_bertbatch_scan, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
  if (adt_check_launch("bertbatch_build(scan)")) return -1;
  if (n_rows > 0) {
    hipLaunchKernelGGL(k_bertbatch_rows, dim3((unsigned)n_rows), dim3(256), 0, (hipStream_t)stream, a);
    return adt_check_launch("bertbatch_build(rows)");
  }
  return 0;
}

int adt_bertbatch_eval(const int64_t* seq_off, const int32_t* seq_items, const int32_t* users, int n_rows, int n_users, int L, int itemnum,
                       int32_t* seq, void* stream) {
  if (L < 1) return adt_set_error("bertbatch_eval: L=%d < 1", L);
  if (itemnum < 1) return adt_set_error("bertbatch_eval: itemnum=%d < 1", itemnum);
  if (n_rows < 0 || n_users < 0) return adt_set_error("bertbatch_eval: n_rows=%d, n_users=%d", n_rows, n_users);
  if (n_rows == 0) return 0;
  if (!seq_off || !seq_items || !users || !seq) return adt_set_error("bertbatch_eval: NULL pointer");
  const size_t work = (size_t)n_rows * (size_t)L;
  if (work > ((size_t)1 << 31)) return adt_set_error("bertbatch_eval: %d rows x L=%d is more than 2^31 positions", n_rows, L);
  BertEvalArgs a{seq_off, seq_items, users, n_rows, n_users, L, (uint32_t)itemnum, seq};
  hipLaunchKernelGGL(k_bertbatch_eval, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return adt_check_launch("bertbatch_eval");
}

}  // extern "C"
