// Argument blocks of the logits / BCE pass and of the id-ring prefetch (adt_misc.cuh: logits_bce_body, ring_prefetch_body); shared with
// the host executor, which hands them from one call of a step to the next as plain arguments.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace adt {

struct LogitsBceArgs {
  const float* F; const float* E; const int* pos; const int* neg; const float* norms; int T;
  float* pos_logits; float* neg_logits; float* dpos; float* dneg; float* loss;      // loss: 2 x 64 sub-slots (pos term, neg term)
  float* dF; float* rep; int nrep; size_t rep_stride;
  int neg_only;              // the item rows of the NEGATIVE ids only: the positive ones are added by k_embed_bwd3 with the embedding rows they share
};

struct RingPrefetchArgs {
  const int32_t* ring; size_t slot_ints; int nslots; size_t n_ints; uint32_t* state; uint32_t* consumed; int32_t* staging;
  int part, nparts;      // this launch copies 16-byte words [part, part + 1) * n / nparts of the slot; the LAST part marks the batch staged and releases the
                         // slot (the parts run in stream order).  0, 0 = the whole slot.  819 KB over PCIe took 34-39 us inside the 24 us loss launch:
                         // half there, half inside the 20 us embedding scatter is hidden in both.
};

}  // namespace adt
