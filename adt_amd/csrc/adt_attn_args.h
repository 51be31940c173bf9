// Argument block of the attention kernels (adt_attn.cuh, adt_attn_bf16.cuh, adt_seqattn.cuh); shared with the host executor.
#pragma once
#include "adt_common.cuh"

namespace adt {

struct AttnArgs {
  const float* Q; int ldq;
  const float* K; int ldk;
  const float* V; int ldv;
  float* O; int ldo;          // forward: output; backward: forward output (input)
  float* LSE;                 // (B*H*L) log-sum-exp of the scaled, masked scores
  int B, H, L;
  int causal;
  float scale;                // 1/sqrt(HD)
  DropCfg drop;               // idx = ((bh + bh_offset) * L + q) * L + key
  uint32_t bh_offset;
  const float* dO; int lddo;  // backward
  float* dQ; int lddq;
  float* dK; int lddk;
  float* dV; int lddv;
  uint32_t* mask;             // optional (B*H*L x 8 words): dropout keep bits written by the bf16 forward, read by its backward
  unsigned long long* stamps; // timing experiments only (ADT_SEQ_STAMPS): s_memtime per wave of workgroup 0
  int in_bf16;                // backward, adt_seqattn.cuh only: Q, K, V, O point at bf16 rows and ldq / ldk / ldv / ldo count bf16 elements
  int out_bf16;               // backward, adt_seqattn.cuh only: dQ, dK, dV are written as bf16 rows in the saved-row order (adt_tt.cuh: tt_store_bf16), lddq /
                              // lddk / lddv count bf16 elements -- for a consumer that only builds bf16 MFMA operands from them (k_seqtt_mid_bwd): the same
                              // values it would have rounded itself, half the bytes
  const void* do_bf16; const float* do_delta;
                              // backward, adt_seqattn.cuh with in_bf16 only: do_bf16 != nullptr: the out-projection reverse in front (k_seqtt_post_bwd<DEC>,
                              // BwdChainArgs::do_bf16) handed dO over as bf16 rows of dO * drop.scale in the saved-row order (64 elements per row) and
                              // delta[h] = rowsum(dO . O) of head h at do_delta[row * 4 + h]: dO and O are not read
  const int* pad_pre;         // backward, k_seqtt_xattn_mid_bwd only: pad prefix of every QUERY sequence (adt_seq_args.h; nullptr: none): the handed-over
                              // dO rows and delta of a query tile wholly inside it are exact zeros (the producer masks its gradient) and are not requested
};

}  // namespace adt
