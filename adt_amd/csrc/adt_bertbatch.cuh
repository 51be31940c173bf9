// BERT4Rec-ADT batches masked and built on the device (include/adt_hip.h: adt_bertbatch_build / adt_bertbatch_eval / adt_bertbatch_token;
// the counterpart of adt_amd/bert4rec/datasets.py:BertTrainDataset + BertModel.stage).  Resident: the training sequences as CSR over the
// U users with a non-empty sequence, and the table of the W sliding windows (offset into seq_items, length 1..L).  Examples are numbered,
// not stored: with D = dupe_factor, example e < W * D is random copy e % D of window e / D, and example W * D + u is the mask-last
// example of user u (its last min(n, L) items).  An id outside 0 .. W * D + U - 1 gives an all-padding row (the caller checks ids on the
// host; the kernels never index with one).
//
// Masking rule (adt_bertbatch_rule, one inline function for the kernels and the host replay).  The decision at window position j of example
// e is a pure function of (seed, salt, e, j) -- not of the step or of the batch row, so a shard draws what the whole batch would:
//   key = adt_seqbatch_key(seed, salt, e, j); h_k = adt_hash32(key ^ k), k = 0, 1, 2 (three independent draws)
//   masked iff h_0 < thr_mask; a masked position becomes [MASK] = itemnum + 1 when h_1 < floor(0.8 * 2^32), the uniform item
//   1 + (h_2 * itemnum >> 32) when h_1 < floor(0.9 * 2^32), and stays the item otherwise; its label is the item.
// dec equals src except that its last position is always [MASK].  A mask-last example draws nothing: src = dec = the items with the last
// replaced by [MASK], and the only label is the last item.
//
// Ordered compaction, integers only, no atomics:
//   1. k_bertbatch_count: one wave per GLOBAL row counts the row's labels (ballot + popcount; only h_0 is needed).
//   2. k_bertbatch_scan: one workgroup turns the n_examples counts into exclusive prefix sums in place (prefix[n_examples] = the total),
//      and writes M = prefix[row0 + n_rows] - prefix[row0] and inv_count = (float)(1.0 / (double)max(total, 1)).
//   3. k_bertbatch_rows: one workgroup per local row writes src / dec / labels and compacts inside the row -- a ballot prefix within a
//      wave, the wave offsets through LDS -- at prefix[row0 + r] - prefix[row0], so rows / labels_c are in ascending flat order.  The
//      workgroup of row r also zeroes the entries r * L .. (r + 1) * L - 1 of rows / labels_c that lie at or beyond M.
// Every loop is bounded by a kernel argument.  Consecutive lanes read and write consecutive ints.
#pragma once
#include "adt_seqbatch.cuh"

#define ADT_BERTBATCH_THR_MASK_TOKEN 0xCCCCCCCCu      // floor(0.8 * 2^32)
#define ADT_BERTBATCH_THR_RANDOM 0xE6666666u          // floor(0.9 * 2^32)

__host__ __device__ __forceinline__ bool adt_bertbatch_masked(uint32_t key, uint32_t thr_mask) { return adt_hash32(key) < thr_mask; }

// the token at window position j of random example e whose item is `item`; *masked says whether the position carries a label
__host__ __device__ __forceinline__ int32_t adt_bertbatch_rule(uint32_t seed, uint32_t salt, uint32_t e, uint32_t j, uint32_t thr_mask,
                                                               uint32_t itemnum, int32_t item, bool* masked) {
  const uint32_t key = adt_seqbatch_key(seed, salt, e, j);
  *masked = adt_bertbatch_masked(key, thr_mask);
  if (!*masked) return item;
  const uint32_t h1 = adt_hash32(key ^ 1u);
  if (h1 < ADT_BERTBATCH_THR_MASK_TOKEN) return (int32_t)(itemnum + 1u);
  if (h1 < ADT_BERTBATCH_THR_RANDOM) return (int32_t)(1u + (uint32_t)(((uint64_t)adt_hash32(key ^ 2u) * (uint64_t)itemnum) >> 32));
  return item;
}

namespace adt {

struct BertBatchArgs {
  const int64_t* seq_off; const int32_t* seq_items;      // the training sequences, CSR over the U users
  const int64_t* win_start; const int32_t* win_len;      // the W windows: offset into seq_items, length 1..L
  const int32_t* examples;                               // the GLOBAL batch, n_examples example ids
  int n_examples, row0, n_rows, L, n_windows, dupe, n_users;
  uint32_t itemnum, seed, salt, thr_mask;
  int32_t* src; int32_t* dec; int32_t* labels;           // (n_rows, L); labels may be null
  int32_t* rows; int32_t* labels_c;                      // capacity n_rows * L
  int32_t* M; float* inv_count;                          // inv_count may be null
  uint32_t* prefix;                                      // n_examples + 1: the row counts, then their exclusive prefix sums
};

struct BertExample {
  const int32_t* items;      // the window
  int len;                   // 0 .. L
  bool random;               // false: the mask-last example
};

ADT_DEVICE_INLINE BertExample bb_example(const BertBatchArgs& a, int e) {
  BertExample x{a.seq_items, 0, false};
  const int64_t n_random = (int64_t)a.n_windows * (int64_t)a.dupe;
  if (e < 0 || (int64_t)e >= n_random + (int64_t)a.n_users) return x;
  if ((int64_t)e < n_random) {
    const int w = e / a.dupe;
    const int len = a.win_len[w];
    x.items = a.seq_items + a.win_start[w];
    x.len = len < 0 ? 0 : (len > a.L ? a.L : len);
    x.random = true;
  } else {
    const int u = (int)((int64_t)e - n_random);
    const int64_t s1 = a.seq_off[u + 1];
    const int64_t n = s1 - a.seq_off[u];
    x.len = n < 0 ? 0 : (n > (int64_t)a.L ? a.L : (int)n);
    x.items = a.seq_items + (s1 - x.len);
  }
  return x;
}

static __global__ __launch_bounds__(256) void k_bertbatch_count(BertBatchArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);      // wave-uniform
  if (row >= a.n_examples) return;
  const int e = a.examples[row];
  const BertExample x = bb_example(a, e);
  int c = 0;
  if (!x.random) {
    c = x.len > 0 ? 1 : 0;
  } else {
    for (int j0 = 0; j0 < x.len; j0 += 64) {
      const int j = j0 + lane;
      const bool m = j < x.len && adt_bertbatch_masked(adt_seqbatch_key(a.seed, a.salt, (uint32_t)e, (uint32_t)j), a.thr_mask);
      c += __popcll(__ballot(m));
    }
  }
  if (lane == 0) a.prefix[row] = (uint32_t)c;
}

// One workgroup.  Thread t owns the contiguous chunk t * per .. (t + 1) * per - 1 of the counts: it sums the chunk, the 256 sums are
// scanned (a shuffle scan inside each wave, the four wave totals through LDS), and the thread walks its chunk again writing prefixes.
static __global__ __launch_bounds__(256) void k_bertbatch_scan(BertBatchArgs a) {
  __shared__ uint32_t wave_total[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n_examples;
  const int per = (n + 255) / 256;
  const int64_t b64 = (int64_t)tid * per;
  const int beg = b64 < (int64_t)n ? (int)b64 : n, end = b64 + per < (int64_t)n ? (int)(b64 + per) : n;
  uint32_t sum = 0;
  for (int i = beg; i < end; ++i) sum += a.prefix[i];
  uint32_t incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wave_total[wave] = incl;
  __syncthreads();
  uint32_t base = incl - sum;
  for (int w = 0; w < wave; ++w) base += wave_total[w];
  for (int i = beg; i < end; ++i) {
    const uint32_t c = a.prefix[i];
    a.prefix[i] = base;
    base += c;
  }
  if (tid == 255) a.prefix[n] = base;      // the last chunk ends at n (or is empty, and base is the total all the same)
  __syncthreads();                         // the prefixes written above are visible to the workgroup
  if (tid == 0) {
    const uint32_t total = a.prefix[n];
    *a.M = (int32_t)(a.prefix[a.row0 + a.n_rows] - a.prefix[a.row0]);
    if (a.inv_count) *a.inv_count = (float)(1.0 / (double)(total > 0u ? total : 1u));
  }
}

static __global__ __launch_bounds__(256) void k_bertbatch_rows(BertBatchArgs a) {
  __shared__ int wave_count[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.x;              // < n_rows
  const int row = a.row0 + r;            // < n_examples (checked by the launcher)
  const int e = a.examples[row];
  const BertExample x = bb_example(a, e);
  const int L = a.L, pad = L - x.len;
  const int32_t mask_token = (int32_t)(a.itemnum + 1u);
  const uint32_t first = a.prefix[a.row0];
  const int M = (int)(a.prefix[a.row0 + a.n_rows] - first);
  int at = (int)(a.prefix[row] - first);       // where this row's compacted entries begin
  const size_t out0 = (size_t)r * (size_t)L;
  for (int t0 = 0; t0 < L; t0 += 256) {
    const int t = t0 + tid;
    int32_t tok = 0, lab = 0;
    if (t < L && t >= pad) {
      const int j = t - pad;
      const int32_t item = x.items[j];
      tok = item;
      if (x.random) {
        bool masked;
        tok = adt_bertbatch_rule(a.seed, a.salt, (uint32_t)e, (uint32_t)j, a.thr_mask, a.itemnum, item, &masked);
        lab = masked ? item : 0;
      } else if (t == L - 1) {
        tok = mask_token;
        lab = item;
      }
    }
    if (t < L) {
      a.src[out0 + t] = tok;
      a.dec[out0 + t] = (t == L - 1 && x.len > 0) ? mask_token : tok;
      if (a.labels) a.labels[out0 + t] = lab;
      const int i = (int)out0 + t;           // < n_rows * L < 2^31 (checked by the launcher)
      if (i >= M) {                          // beyond the compacted entries of ALL rows: this row's share of the zero tail
        a.rows[i] = 0;
        a.labels_c[i] = 0;
      }
    }
    const unsigned long long b = __ballot(lab != 0);
    if (lane == 0) wave_count[wave] = __popcll(b);
    __syncthreads();
    int before = __popcll(b & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = wave_count[w];
      before += w < wave ? c : 0;
      all += c;
    }
    if (lab != 0) {
      a.rows[at + before] = (int32_t)(out0 + t);
      a.labels_c[at + before] = lab;
    }
    at += all;
    __syncthreads();                         // wave_count is rewritten by the next chunk
  }
}

// BertEvalDataset.sequence: the last L - 1 training items followed by [MASK], left-padded; one thread per (row, position)
struct BertEvalArgs {
  const int64_t* seq_off; const int32_t* seq_items; const int32_t* users;
  int n_rows, n_users, L;
  uint32_t itemnum;
  int32_t* seq;
};

static __global__ __launch_bounds__(256) void k_bertbatch_eval(BertEvalArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)a.n_rows * (size_t)a.L) return;
  const int r = (int)(i / (size_t)a.L), t = (int)(i - (size_t)r * (size_t)a.L);
  int32_t v = 0;
  if (t == a.L - 1) {
    v = (int32_t)(a.itemnum + 1u);
  } else {
    const int u = a.users[r];
    if (u >= 0 && u < a.n_users) {         // a user outside the CSR has no history
      const int64_t s1 = a.seq_off[u + 1];
      const int64_t n = s1 - a.seq_off[u];
      const int64_t back = (int64_t)(a.L - 1 - t);      // 1 .. L - 1 items from the end
      if (back <= n) v = a.seq_items[s1 - back];
    }
  }
  a.seq[i] = v;
}

}  // namespace adt
