// The `phase` word of adt_sasrec_backward* (include/adt_hip.h: ADT_PHASE_*) decoded once, by name.  Plain C++: no HIP, no library state, so
// the accept / reject table is tested by a host program (tests/test_backward_plan_cpu.py).
#pragma once
#include "../../include/adt_hip.h"

struct BwdPlan {
  int phase;               // 0 everything, 1 logits + decoder stack, 2 last LayerNorm + encoder stack + tables
  bool prep_zeroed;        // adt_sasrec_step_begin* of this step zeroed the item-table and parameter-gradient replicas
  bool defer_fold;         // (one-phase only) adt_sasrec_fold_clip_adam / adt_sasrec_fold_grads does the last fold
  bool bce_here;           // the forward was adt_sasrec_forward_loss on the deferred path: logits + BCE seed are formed by the backward
  bool bce_fwd;            // ... and launched that kernel itself (ADT_TRAIN_BCE_SIDE): only its join is left
  bool seeds_virtual;      // that forward does not materialise the reconstruction seeds k_seqtt_attn_pre_bwd can form itself
};

// nullptr and *out filled, or the error message.  deferred: bce_deferred(cfg), the forward's predicate for the deferred path.
inline const char* adt_bwd_plan(int phase_word, bool deferred, BwdPlan* out) {
  BwdPlan p;
  p.phase = phase_word & ADT_PHASE_MASK;
  p.prep_zeroed = (phase_word & ADT_PHASE_PREZEROED) != 0;
  p.defer_fold = (phase_word & ADT_PHASE_DEFER_FOLD) != 0 && p.phase == 0;
  p.bce_here = (phase_word & ADT_PHASE_BCE_HERE) != 0;
  p.bce_fwd = (phase_word & ADT_PHASE_BCE_FWD) != 0;
  p.seeds_virtual = p.bce_here || p.bce_fwd || (phase_word & ADT_PHASE_SEEDS_VIRTUAL) != 0;
  if (p.phase == 3) return "backward: phase 3 (0 everything, 1 decoder half, 2 encoder half)";
  if ((p.bce_here || p.bce_fwd) && !deferred) return "backward: phase bit 4 / 5 without the deferred-BCE forward (adt_sasrec_bce_deferred)";
  if (p.bce_fwd && (p.bce_here || !p.prep_zeroed || p.phase == 2)) return "backward: phase bit 5 goes with bit 2, without bit 4, in phase 0 or 1";
  *out = p;
  return nullptr;
}
