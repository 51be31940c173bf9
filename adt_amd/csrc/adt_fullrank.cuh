// Full-catalogue ranking and top-K selection for the dot-product backbones (SASRec-ADT, BERT4Rec-ADT): exact fp32 scores
// s[b][j] = F[b] . E[j] (+ bias[j]) of every eligible item (ids first_id .. n_items, first_id = 1 or 0), the rank of one target item per user and the K best items, without a
// (B, V) logit matrix in HBM.  DESIGN.md section 12.
//
//   k_full_rank        grid (tiles of 16 user rows, S item splits), 4 waves.  The workgroup keeps its 16 feature rows in LDS and streams
//                      its item range through LDS in chunks of 128 items x 64 columns (register prefetch of the next piece while the
//                      current one is multiplied); wave w owns item tiles 2w, 2w+1 of the chunk (two independent accumulators) and, in
//                      the epilogue, user rows 4w .. 4w+3: it counts the eligible items that beat the target and offers every eligible
//                      score to the row's running top-K list, which lives in registers (entries `lane` and `lane + 64` of 128).
//   k_full_rank_merge  one wave per user row: sums the S counts and merges the S partial lists in split order.
//
// The target's score comes from the SAME tile code: a first pass multiplies the feature tile with the 16 gathered target rows and keeps
// the diagonal, so a table row equal to the target's row ties with it bit for bit: every score is one fmaf chain over the columns in
// the same fixed order (MFMA j of a 32-column block contracts columns j, 8 + j, 16 + j, 24 + j), whatever the item's place in a tile.
// No atomics touch a result: counts are ballots, a top-K list is the K best of a SET under the total order (score descending, id
// ascending), so neither the chunking nor S can change an output bit.
//
// The group-aware form (k_full_rank<true>, k_full_rank_merge<true>) ranks P stacked candidates of the same R
// users in one launch: feature row r belongs to user row0 + r % R of a resident CSR with int64 offsets, whose target and seen list it
// reads.  The seen bitmap and the target are per row already, so a 16-row tile may straddle a group boundary; only the three reads
// that name the user change.  It is a template flag: the <false> instantiations compile to the code the plain kernels had.
#pragma once
#include "adt_common.cuh"
#include <type_traits>

namespace adt {

constexpr int FR_NW = 4, FR_NTH = FR_NW * 64;
constexpr int FR_CH = 128;            // items per chunk: two 16-item tiles per wave
constexpr int FR_KC = 64;             // columns per piece
constexpr int FR_ERS = FR_KC + 4;     // row stride of the item image (adt_common.cuh: K + 4)
constexpr int FR_SRS = FR_CH + 4;     // row stride of the score tile: rows 4g + r of the accumulator layout land 16 banks apart
constexpr int FR_SC = 4096;           // items per seen bitmap (16 rows x 128 words); a longer split range rebuilds it per 4,096 items
constexpr int FR_BMW = FR_SC / 32;
constexpr int FR_KMAX = 128;
constexpr int FR_LD4 = FR_CH * FR_KC / 4 / FR_NTH;      // float4 loads per thread and piece (8)

struct FullRankArgs {
  const float* F; int ldf; const float* E; int lde; const float* bias;
  int B, d, n_items;
  int first_id;                        // the smallest id that competes: 1, or 0 where the padding row is a candidate (STOSA-ADT's full sort)
  const int32_t* target; const int32_t* indptr; const int32_t* indices;
  int K, S, per;                      // per: items per split, a multiple of FR_CH
  int32_t* ws_cnt; float* ws_val; int32_t* ws_idx;      // (B, S, 2) {rank count, eligible count}, (B, S, K), (B, S, K)
  int32_t* rank; int32_t* n_elig; int32_t* top_idx; float* top_val;
};

// the group-aware form's argument block: rows per group, the first CSR row, the CSR's int64 offsets (indptr is unused, indices its items)
struct FullRankGroupArgs : FullRankArgs { int R, row0; const int64_t* off; };
template <bool GROUPS> using FrArgs = std::conditional_t<GROUPS, FullRankGroupArgs, FullRankArgs>;

static inline size_t full_rank_lds_bytes(int d) {
  const int d32 = (d + 31) & ~31;
  return ((size_t)16 * (d32 + 4) + (size_t)FR_CH * FR_ERS + (size_t)16 * FR_SRS + (size_t)16 * FR_BMW + 32) * 4;
}

// (v, i) ranks ahead of (bv, bi): the higher score, ties to the smaller id (adt_wide.cuh: topk_less, mirrored)
ADT_DEVICE_INLINE bool fr_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && (unsigned)i < (unsigned)bi); }

ADT_DEVICE_INLINE float fr_readlane(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }

// One user's running list: 128 entries sorted best first, entry p on lane p & 63 (v0 / i0 for p < 64, v1 / i1 above); empty entries
// are (-inf, -1), which every real candidate beats.  (tv, ti) is entry K - 1, wave-uniform: what a candidate has to beat.
struct FrList { float v0, v1; int i0, i1; float tv; int ti; };

ADT_DEVICE_INLINE void fr_list_init(FrList& L) {
  L.v0 = L.v1 = L.tv = -__builtin_inff();
  L.i0 = L.i1 = L.ti = -1;
}

ADT_DEVICE_INLINE void fr_insert(FrList& L, float cv, int ci, int K, int lane) {
  const bool b0 = fr_better(L.v0, L.i0, cv, ci), b1 = fr_better(L.v1, L.i1, cv, ci);      // the entries that stay ahead: a prefix
  const int pos = __popcll(__ballot(b0)) + __popcll(__ballot(b1));
  const float uv0 = __shfl_up(L.v0, 1, 64), uv1 = __shfl_up(L.v1, 1, 64), wv = fr_readlane(L.v0, 63);
  const int ui0 = __shfl_up(L.i0, 1, 64), ui1 = __shfl_up(L.i1, 1, 64), wi = __builtin_amdgcn_readlane(L.i0, 63);
  if (!b0) {
    L.v0 = lane == pos ? cv : uv0;
    L.i0 = lane == pos ? ci : ui0;
  }
  if (!b1) {
    L.v1 = lane + 64 == pos ? cv : (lane == 0 ? wv : uv1);
    L.i1 = lane + 64 == pos ? ci : (lane == 0 ? wi : ui1);
  }
  const int kl = (K - 1) & 63;
  L.tv = K > 64 ? fr_readlane(L.v1, kl) : fr_readlane(L.v0, kl);
  L.ti = K > 64 ? __builtin_amdgcn_readlane(L.i1, kl) : __builtin_amdgcn_readlane(L.i0, kl);
}

// every lane offers (v, id) where cond holds; those that beat entry K - 1 are inserted, lowest lane first
ADT_DEVICE_INLINE void fr_offer(FrList& L, float v, int id, bool cond, int K, int lane) {
  cond = cond && fr_better(v, id, L.tv, L.ti);
  unsigned long long m = __ballot(cond);
  while (m) {
    const int l = __builtin_ctzll(m);
    fr_insert(L, fr_readlane(v, l), __builtin_amdgcn_readlane(id, l), K, lane);
    cond = cond && lane != l && fr_better(v, id, L.tv, L.ti);
    m = __ballot(cond);
  }
}

struct FrCtx {
  float* Fi; float* Ei; float* Sc; uint32_t* bm; float* tsc; int* tgt;
  int frs, d32, b0, tid, lane, w;
};

// one 128 x 64 piece of the item table into registers; GATHER: slot c < 16 is the target row of user c
template <bool GATHER>
ADT_DEVICE_INLINE void fr_load_piece(const FullRankArgs& a, const FrCtx& x, float4 (&regs)[FR_LD4], int base, int hi, int k0) {
  adt_static_for<FR_LD4>([&](auto I) {
    constexpr int i = decltype(I)::value;
    const int idx = x.tid + FR_NTH * i, slot = idx >> 4, k = k0 + (idx & 15) * 4;
    int item;
    if constexpr (GATHER) item = slot < 16 ? x.tgt[slot] : 0;
    else item = base + slot < hi ? base + slot : 0;
    regs[i] = k < a.d ? *reinterpret_cast<const float4*>(a.E + (size_t)item * a.lde + k) : make_float4(0.f, 0.f, 0.f, 0.f);
  });
}

// The items [lo, hi) in chunks of FR_CH (GATHER: the one chunk of target rows).  cnt / ne / L: the four user rows this wave owns.
template <bool GATHER>
ADT_DEVICE_INLINE void fr_run(const FullRankArgs& a, const FrCtx& x, int lo, int hi, int sc_lo, int (&cnt)[4], int (&ne)[4], FrList (&L)[4]) {
  const int nk = (x.d32 + FR_KC - 1) / FR_KC;
  const int nchunks = GATHER ? 1 : (hi - lo + FR_CH - 1) / FR_CH, nsteps = nchunks * nk;
  const int c = x.lane & 15, g = x.lane >> 4;
  float4 regs[FR_LD4];
  fr_load_piece<GATHER>(a, x, regs, lo, hi, 0);
  f32x4 acc[2];
  for (int step = 0; step < nsteps; ++step) {
    const int ic = step / nk, kc = step - ic * nk, base = lo + ic * FR_CH, k0 = kc * FR_KC;
    adt_static_for<FR_LD4>([&](auto I) {
      constexpr int i = decltype(I)::value;
      const int idx = x.tid + FR_NTH * i;
      *reinterpret_cast<float4*>(x.Ei + (idx >> 4) * FR_ERS + (idx & 15) * 4) = regs[i];
    });
    __syncthreads();
    if (step + 1 < nsteps) {
      const int ic1 = (step + 1) / nk;
      fr_load_piece<GATHER>(a, x, regs, lo + ic1 * FR_CH, hi, (step + 1 - ic1 * nk) * FR_KC);
    }
    if (kc == 0) acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kn = (x.d32 - k0 < FR_KC ? x.d32 - k0 : FR_KC) / 32;
    for (int kk = 0; kk < kn; ++kk) {
      const Frag8 fa = frag_contig(x.Fi + c * x.frs + k0 + kk * 32 + 8 * g);
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[t] = mma16<PREC_F32>(acc[t], fa, frag_contig(x.Ei + ((2 * x.w + t) * 16 + c) * FR_ERS + kk * 32 + 8 * g));
    }
    if (kc == nk - 1) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int slot = (2 * x.w + t) * 16 + c;
        float bv = 0.f;
        if (a.bias) {
          int item;
          if constexpr (GATHER) item = slot < 16 ? x.tgt[slot] : 0;
          else item = base + slot < hi ? base + slot : 0;
          bv = a.bias[item];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) x.Sc[(4 * g + r) * FR_SRS + slot] = a.bias ? acc[t][r] + bv : acc[t][r];
      }
      __syncthreads();
      if constexpr (GATHER) {
        if (x.tid < 16) x.tsc[x.tid] = x.Sc[x.tid * FR_SRS + x.tid];
      } else {
        adt_static_for<4>([&](auto R) {
          constexpr int rr = decltype(R)::value;
          const int row = 4 * x.w + rr;
          const bool live = x.b0 + row < a.B;
          const int t = x.tgt[row] ? x.tgt[row] : -1;      // no target: no id is set aside (id 0 competes when first_id = 0)
          const float ts = x.tsc[row];
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            const int slot = x.lane + 64 * half, id = base + slot;
            const float v = x.Sc[row * FR_SRS + slot];
            bool elig = live && id >= a.first_id && id < hi;
            if (elig) elig = ((x.bm[row * FR_BMW + ((id - sc_lo) >> 5)] >> ((id - sc_lo) & 31)) & 1u) == 0u;
            const bool other = elig && id != t;
            ne[rr] += __popcll(__ballot(other));
            cnt[rr] += __popcll(__ballot(other && v > ts));
            if (a.K > 0) fr_offer(L[rr], v, id, elig, a.K, x.lane);
          }
        });
      }
    }
    __syncthreads();
  }
}

template <bool GROUPS>
__global__ __launch_bounds__(FR_NTH) void k_full_rank(FrArgs<GROUPS> a) {
  extern __shared__ __attribute__((aligned(16))) float fr_lds[];
  FrCtx x;
  x.tid = threadIdx.x; x.lane = x.tid & 63; x.w = x.tid >> 6;
  x.d32 = (a.d + 31) & ~31; x.frs = x.d32 + 4;
  x.b0 = blockIdx.x * 16;
  x.Fi = fr_lds;
  x.Ei = x.Fi + 16 * x.frs;
  x.Sc = x.Ei + FR_CH * FR_ERS;
  x.bm = reinterpret_cast<uint32_t*>(x.Sc + 16 * FR_SRS);
  x.tsc = reinterpret_cast<float*>(x.bm + 16 * FR_BMW);
  x.tgt = reinterpret_cast<int*>(x.tsc + 16);
  const int s = blockIdx.y, lo = s * a.per, hi = lo + a.per < a.n_items + 1 ? lo + a.per : a.n_items + 1;

  // the 16 feature rows, zero beyond d and beyond B; the targets (0 = none)
  const int q = x.d32 / 4;
  for (int idx = x.tid; idx < 16 * q; idx += FR_NTH) {
    const int row = idx / q, c4 = (idx - row * q) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (x.b0 + row < a.B && c4 < a.d) v = *reinterpret_cast<const float4*>(a.F + (size_t)(x.b0 + row) * a.ldf + c4);
    *reinterpret_cast<float4*>(x.Fi + row * x.frs + c4) = v;
  }
  // the row of target / the seen CSR that feature row b reads: b itself, or user row0 + b % R
  const auto user = [&](int b) {
    if constexpr (GROUPS) return a.row0 + b % a.R;
    else return b;
  };
  if (x.tid < 16) {
    int t = (a.target && x.b0 + x.tid < a.B) ? a.target[user(x.b0 + x.tid)] : 0;
    if (t < 1 || t > a.n_items) t = 0;
    x.tgt[x.tid] = t;
    x.tsc[x.tid] = 0.f;
  }
  __syncthreads();

  int cnt[4] = {0, 0, 0, 0}, ne[4] = {0, 0, 0, 0};
  FrList L[4];
  adt_static_for<4>([&](auto R) { fr_list_init(L[decltype(R)::value]); });

  if (a.target) fr_run<true>(a, x, 0, 0, 0, cnt, ne, L);      // target scores through the tile code

  for (int sc_lo = lo; sc_lo < hi; sc_lo += FR_SC) {
    const int sc_hi = sc_lo + FR_SC < hi ? sc_lo + FR_SC : hi;
    // seen bitmap of items [sc_lo, sc_hi): out-of-range ids and duplicates fall away, the target stays eligible
    for (int i = x.tid; i < 16 * FR_BMW; i += FR_NTH) x.bm[i] = 0u;
    __syncthreads();
    using Off = std::conditional_t<GROUPS, int64_t, int>;      // the offsets' own type: int64 in the resident CSR
    const Off* off;
    if constexpr (GROUPS) off = a.off; else off = a.indptr;
    if (off) {
      for (int row = x.w; row < 16; row += FR_NW) {
        const int b = x.b0 + row;
        if (b >= a.B) break;
        const int u = user(b), t = x.tgt[row] ? x.tgt[row] : -1;
        const Off j1 = off[u + 1];
        for (Off j = off[u] + x.lane; j < j1; j += 64) {
          const int id = a.indices[j];
          if (id >= a.first_id && id >= sc_lo && id < sc_hi && id != t) atomicOr(&x.bm[row * FR_BMW + ((id - sc_lo) >> 5)], 1u << ((id - sc_lo) & 31));
        }
      }
      __syncthreads();
    }
    fr_run<false>(a, x, sc_lo, sc_hi, sc_lo, cnt, ne, L);
  }

  adt_static_for<4>([&](auto R) {
    constexpr int rr = decltype(R)::value;
    const int b = x.b0 + 4 * x.w + rr;
    if (b < a.B) {
      const size_t o = (size_t)b * a.S + s;
      if (x.lane == 0) { a.ws_cnt[o * 2] = cnt[rr]; a.ws_cnt[o * 2 + 1] = ne[rr]; }
      if (x.lane < a.K) { a.ws_val[o * a.K + x.lane] = L[rr].v0; a.ws_idx[o * a.K + x.lane] = L[rr].i0; }
      if (x.lane + 64 < a.K) { a.ws_val[o * a.K + x.lane + 64] = L[rr].v1; a.ws_idx[o * a.K + x.lane + 64] = L[rr].i1; }
    }
  });
}

template <bool GROUPS>
__global__ __launch_bounds__(FR_NTH) void k_full_rank_merge(FrArgs<GROUPS> a) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * FR_NW + (threadIdx.x >> 6);
  if (b >= a.B) return;
  int cnt = 0, ne = 0;
  for (int s = lane; s < a.S; s += 64) {
    cnt += a.ws_cnt[((size_t)b * a.S + s) * 2];
    ne += a.ws_cnt[((size_t)b * a.S + s) * 2 + 1];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    ne += __shfl_xor(ne, o, 64);
  }
  if (lane == 0) {
    int u = b;
    if constexpr (GROUPS) u = a.row0 + b % a.R;
    const int t = a.target ? a.target[u] : 0;
    a.rank[b] = (t >= 1 && t <= a.n_items) ? cnt : -1;
    a.n_elig[b] = ne;
  }
  if (a.K <= 0) return;
  FrList L;
  fr_list_init(L);
  for (int s = 0; s < a.S; ++s) {
    const size_t o = ((size_t)b * a.S + s) * a.K;
    for (int p0 = 0; p0 < a.K; p0 += 64) {
      const int p = p0 + lane;
      const bool ok = p < a.K;
      const float v = ok ? a.ws_val[o + p] : 0.f;
      const int id = ok ? a.ws_idx[o + p] : -1;
      fr_offer(L, v, id, id >= 0, a.K, lane);
    }
  }
  if (lane < a.K) { a.top_val[(size_t)b * a.K + lane] = L.v0; a.top_idx[(size_t)b * a.K + lane] = L.i0; }
  if (lane + 64 < a.K) { a.top_val[(size_t)b * a.K + lane + 64] = L.v1; a.top_idx[(size_t)b * a.K + lane + 64] = L.i1; }
}

}  // namespace adt
