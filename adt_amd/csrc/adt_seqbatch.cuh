// STOSA-ADT batches built on the device (include/adt_hip.h: adt_seqbatch_build / adt_seqbatch_draw; the counterpart of
// adt_amd/stosa/datasets.py:DisenDataset.batch).  The user sequences and every user's sorted item set live in HBM as two CSRs; one thread
// per (row, position) cuts the train / valid / test view and draws the negative, so consecutive lanes read and write consecutive ints.
//
// Views of a sequence s of length n (cut = 3 train, 2 valid, 1 test; Python slicing, so an empty result is all padding):
//   inp = s[:-cut], pos = s[1:-(cut - 1)] (s[1:] for cut 1), dec = s[:-(cut + 1)]; each keeps its last L entries, left-padded with 0.
// inp and pos have m = max(n - cut, 0) entries and dec has max(m - 1, 0), so with j = m - L + t position t of a row holds
//   inp[t] = s[j], pos[t] = s[j + 1] where j >= 0, dec[t] = s[j - 1] where j >= 1, and 0 elsewhere.
//
// Negatives.  Where pos is 0, neg is 0.  Elsewhere neg is uniform over [1, item_size - 1] minus the user's set, by rejection: attempt a of
// position t of GLOBAL row `row` proposes adt_seqbatch_draw_id(seed, step, row, t, a, item_size), a pure function of its arguments (so
// what a rank draws does not depend on how the batch is sharded, and the host can replay it), and the first proposal outside the set
// wins.  Membership is a binary search of the sorted set.
//
// Termination.  At most ADT_SEQBATCH_MAX_REJECTS = 32 proposals are rejected (attempts 0 .. 31).  After the 32nd, the kernel walks upward
// from that last proposal, cyclically inside [1, item_size - 1] (item_size - 1 is followed by 1), and takes the first id outside the set;
// the walk visits each id once, so it is at most item_size - 1 steps.  When the set covers every id of [1, item_size - 1] the negative
// is 0.  Every loop is bounded by a kernel argument or by the length of a set; none depends on the ids themselves.
#pragma once
#include "adt_common.cuh"

#define ADT_SEQBATCH_MAX_REJECTS 32

// the part of a draw that all attempts of one (row, position) share: a chain of bijections, so changing any one argument changes the key
__host__ __device__ __forceinline__ uint32_t adt_seqbatch_key(uint32_t seed, uint32_t step, uint32_t row, uint32_t t) {
  uint32_t h = adt_hash32(seed ^ 0x9E3779B9u);
  h = adt_hash32(h ^ step);
  h = adt_hash32(h ^ row);
  return adt_hash32(h ^ t);
}
// multiply-high of the 32-bit hash onto [1, item_size - 1]: bias at most (item_size - 1) / 2^32
__host__ __device__ __forceinline__ int32_t adt_seqbatch_draw_key(uint32_t key, uint32_t attempt, uint32_t item_size) {
  const uint32_t h = adt_hash32(key ^ attempt);
  return (int32_t)(1u + (uint32_t)(((uint64_t)h * (uint64_t)(item_size - 1u)) >> 32));
}
__host__ __device__ __forceinline__ int32_t adt_seqbatch_draw_id(uint32_t seed, uint32_t step, uint32_t row, uint32_t t, uint32_t attempt,
                                                                 uint32_t item_size) {
  return adt_seqbatch_draw_key(adt_seqbatch_key(seed, step, row, t), attempt, item_size);
}

namespace adt {

struct SeqBatchArgs {
  const int64_t* seq_off; const int32_t* seq_items;      // the sequences, CSR over the users
  const int64_t* set_off; const int32_t* set_items;      // every user's sorted, de-duplicated items (held-out ones included)
  const int32_t* users;                                  // the GLOBAL batch, n_users entries
  int n_users, row0, n_rows, L, cut;
  uint32_t item_size, seed, step;
  int32_t* inp; int32_t* dec; int32_t* pos; int32_t* neg;      // (n_rows, L); dec / pos / neg may be null
  float* inv_count;
};

// at most ceil(log2(n + 1)) rounds
ADT_DEVICE_INLINE bool sb_member(const int32_t* set, int n, int32_t id) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (set[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && set[lo] == id;
}

static __global__ __launch_bounds__(256) void k_seqbatch_build(SeqBatchArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)a.n_rows * (size_t)a.L) return;
  const int r = (int)(i / (size_t)a.L), t = (int)(i - (size_t)r * (size_t)a.L);
  const int row = a.row0 + r;      // < n_users (checked by the launcher)
  const int u = a.users[row];
  const int64_t s0 = a.seq_off[u];
  const int n = (int)(a.seq_off[u + 1] - s0);
  const int m = n > a.cut ? n - a.cut : 0;
  const int j = m - a.L + t;       // <= m - 1, so j + 1 <= n - cut < n
  const int32_t* s = a.seq_items + s0;
  const int32_t vp = j >= 0 ? s[j + 1] : 0;
  a.inp[i] = j >= 0 ? s[j] : 0;
  if (a.dec) a.dec[i] = j >= 1 ? s[j - 1] : 0;
  if (a.pos) a.pos[i] = vp;
  if (!a.neg) return;
  int32_t vn = 0;
  if (vp != 0) {
    const int64_t q0 = a.set_off[u];
    const int ns = (int)(a.set_off[u + 1] - q0);
    const int32_t* set = a.set_items + q0;
    const uint32_t key = adt_seqbatch_key(a.seed, a.step, (uint32_t)row, (uint32_t)t);
    bool found = false;
    for (uint32_t att = 0; att < ADT_SEQBATCH_MAX_REJECTS; ++att) {
      vn = adt_seqbatch_draw_key(key, att, a.item_size);
      if (!sb_member(set, ns, vn)) { found = true; break; }
    }
    if (!found) {                  // the guard: first free id upward from the last proposal, cyclically; 0 when there is none
      const int32_t top = (int32_t)a.item_size - 1;
      int32_t c = vn;
      vn = 0;
      for (int32_t k = 0; k < top; ++k) {
        c = c == top ? 1 : c + 1;
        if (!sb_member(set, ns, c)) { vn = c; break; }
      }
    }
  }
  a.neg[i] = vn;
}

// 1 / max(number of non-zero pos entries of the WHOLE batch, 1): item ids are >= 1, so a row has min(max(n - cut, 0), L) of them.
// One wave; an integer sum (no float atomics), the quotient taken in double and rounded once, as the host computes it.
static __global__ __launch_bounds__(64) void k_seqbatch_count(SeqBatchArgs a) {
  unsigned long long c = 0;
  for (int i = threadIdx.x; i < a.n_users; i += 64) {
    const int u = a.users[i];
    const int n = (int)(a.seq_off[u + 1] - a.seq_off[u]);
    const int m = n > a.cut ? n - a.cut : 0;
    c += (unsigned long long)(m < a.L ? m : a.L);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (threadIdx.x == 0) *a.inv_count = (float)(1.0 / (double)(c > 0 ? c : 1ull));
}

}  // namespace adt
