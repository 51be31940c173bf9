"""CPU: which kernels a flagship SASRec-ADT step launches and which shapes the per-sequence launchers cover, as adt_amd/csrc/adt_step_plan.h decides
it.  A stand-alone host program (plain g++, no HIP) prints one line per case; the expected lines are restated here from the predicates that
adt_sasrec.hip and adt_seq.hip applied before the plan header existed (commit a96fd0e: "sasrec.hip:N" / "seq.hip:N" below are its line numbers), each
group citing its rule.  Built and run a second time with -fsanitize=address,undefined."""
import itertools
import os
import subprocess

import pytest

from adt_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F32, BF16 = 0, 1
LDS_MAX = 160 * 1024
MAXLEN, ROW_STRIDE = 224, 72
IS_MAXV1 = 16000      # adt_itemgrad.cuh: adt_item_sort_supported(rows) = 2 <= rows <= IS_MAXV1

# SeqSwitches, in the order of its fields, with the defaults adt_env_on / adt_env_int gave each site
SWITCHES = ("seq seq_lean seq_tt seq_bwd seq_attn_bwd seq_post_bwd seq_partials xattn_fused seq_ablate seq_ablate_set seq_split attn_split side_stream "
            "side_stream_dp item_sort lnl_fused fold_parts fwd_fused embed3 bce_merged").split()
DEFAULT = dict(seq=1, seq_lean=1, seq_tt=1, seq_bwd=1, seq_attn_bwd=1, seq_post_bwd=1, seq_partials=1, xattn_fused=1, seq_ablate=0, seq_ablate_set=0,
               seq_split=0, attn_split=1, side_stream=7, side_stream_dp=0, item_sort=0, lnl_fused=1, fold_parts=1, fwd_fused=1, embed3=1, bce_merged=1)
GATING = SWITCHES[:8]      # the eight that gate one another
ON_OFF = GATING + ["attn_split", "lnl_fused", "fold_parts", "fwd_fused", "embed3", "bce_merged"]


def arm(**kw):
    assert set(kw) <= set(SWITCHES), kw
    return dict(DEFAULT, **kw)


ARMS = [arm()] + [arm(**{k: 0}) for k in ON_OFF] + [arm(item_sort=1), arm(side_stream_dp=1), arm(seq_split=1), arm(seq_split=2)]
ARMS += [arm(side_stream=v) for v in range(8)] + [arm(seq_ablate=0, seq_ablate_set=1), arm(seq_ablate=1, seq_ablate_set=1), arm(side_stream=15)]
N_NAMED = len(ARMS)
ARMS += [arm(**dict(zip(GATING, bits))) for bits in itertools.product((0, 1), repeat=8)]

# (prec, d, H, L, layers, B, rows): every shape under the default switches, a flagship subset under every arm
FULL = ((F32, BF16), (64, 128), (1, 2, 4, 8), (1, 4, 6, 128, 200, 202, 224, 225), (1, 2, 3, 4, 5, 16, 17), (1, 16, 32, 64, 128, 129, 256), (2, 3417, 16000, 16001))
SOME = ((F32, BF16), (64,), (1, 2, 4), (4, 200, 202, 224), (2, 3, 5), (128, 256), (3417, 16001))
EDGE = [(BF16, 64, 3, 200, 2, 128, 3417), (BF16, 64, 0, 200, 2, 128, 3417), (BF16, 64, -2, 200, 2, 128, 3417), (BF16, 64, 128, 200, 2, 128, 3417),
        (BF16, 64, 2, 200, 0, 128, 3417), (BF16, 64, 2, 0, 2, 128, 3417), (BF16, 64, 2, 200, 2, 0, 3417), (BF16, 64, 2, 200, 2, 128, 1), (7, 64, 2, 200, 2, 128, 3417)]
BWD_ARMS = [ARMS.index(arm(**kw)) for kw in ({}, {"fold_parts": 0}, {"embed3": 0}, {"fwd_fused": 0}, {"seq_lean": 0}, {"item_sort": 1}, {"side_stream_dp": 1},
                                             {"side_stream": 0})]
BWD_LAYERS = (2, 3)

# hand-made argument shapes for the launchers' rules: a covered base, one fact changed at a time.
# attention (L H B causal in_bf16 out_bf16 ldq ldk ldv ldo lddo dropout keep_bits), chain (L H B T wimg saved_bf16 grad_bf16 parts4 nsplit ablate drec), hd, handover
ATT0 = dict(L=200, H=2, B=128, causal=1, in_bf16=1, out_bf16=1, ldq=64, ldk=128, ldv=128, ldo=64, lddo=64, dropout=1, keep_bits=1)
CH0 = dict(L=200, H=2, B=128, T=25600, wimg=1, saved_bf16=1, grad_bf16=1, parts4=1, nsplit=1, ablate=0, drec=0)
HAND = [({}, {}, 32, 1)]
HAND += [({k: v}, {}, 32, 1) for k, v in (("causal", 0), ("in_bf16", 0), ("out_bf16", 0), ("ldq", 68), ("ldk", 132), ("ldv", 132), ("ldo", 68), ("ldq", 66), ("lddo", 66),
                                          ("keep_bits", 0), ("dropout", 0), ("B", 64), ("L", 128), ("H", 4), ("H", 1))]
HAND += [({"in_bf16": 0, "ld" + t: 68}, {}, 32, 1) for t in "qkvo"] + [({"in_bf16": 0, "ldq": 66}, {}, 32, 1), ({"dropout": 0, "keep_bits": 0}, {}, 32, 1)]
HAND += [({}, {k: v}, 32, 1) for k, v in (("wimg", 0), ("saved_bf16", 0), ("grad_bf16", 0), ("parts4", 0), ("nsplit", 2), ("ablate", 1), ("T", 25599), ("L", 204),
                                          ("drec", 1), ("H", 4), ("B", 127))]
HAND += [({}, {}, hd, 1) for hd in (16, 64, 8, 48)] + [({}, {}, 32, 0), ({"H": 4}, {"H": 4, "drec": 1}, 16, 1), ({"H": 1}, {"H": 1, "drec": 1}, 64, 1), ({"H": 4}, {"H": 4, "drec": 1}, 32, 1)]
HAND += [({"L": L, "H": H}, {"L": L, "T": 128 * L}, 64 // H, 1) for H in (1, 2, 4) for L in (4, 128, 132, 192, 196, 224, 228)]
HAND += [({"L": 202}, {"L": 202, "T": 128 * 202}, 32, 1), ({"L": 225}, {"L": 225, "T": 128 * 225}, 32, 1)]


# ---- the rules, as the two files applied them ----------------------------------------------------------------------------------------------
def sab_lds(L, H):      # adt_seqattn.cuh: sab_lds_bytes
    R = (L + 31) // 32 * 32
    return 4 * R * ROW_STRIDE * 2 + H * R * 8 * 4 + 2 * H * R * 4


def xm_lds(L, H):      # adt_seqxattn_tt.cuh: xm_rows, xm_lds_bytes
    R = 128 if (L + 31) // 32 <= 4 else MAXLEN
    return 4 * R * ROW_STRIDE * 2 + H * R * 8 * 4 + 2 * H * R * 4 + 256 * 4


def head_ok(hd):
    return hd in (16, 32, 64)


def expect_plan(sw, prec, d, H, L, nl, B, rows):
    hd = d // H if H >= 1 and d % H == 0 else 0
    # check_cfg, sasrec.hip:215-223
    if d != 64:
        err = "sasrec: hidden=%d unsupported in this build (64)" % d
    elif H < 1 or d % H:
        err = "sasrec: bad num_heads"
    elif not head_ok(hd):
        err = "sasrec: head_dim=%d unsupported (16/32/64)" % hd
    elif L > 224:
        err = "sasrec: maxlen=%d > 224 unsupported" % L
    elif nl < 1 or nl > 16:
        err = "sasrec: num_layers"
    else:
        err = ""
    # adt_seq_supported, seq.hip:32-35 (SQ_LP = 224)
    use_seq = bool(sw["seq"] and prec == BF16 and d == 64 and L <= 224 and head_ok(hd))
    # adt_seq_lean, seq.hip:40-44 (SB_R = 224)
    lean = bool(sw["seq_lean"] and sw["seq_tt"] and sw["seq_bwd"] and sw["seq_attn_bwd"] and not sw["seq_ablate_set"] and use_seq and L % 4 == 0 and L <= 224
                and sab_lds(L, 64 // hd) <= LDS_MAX)
    # adt_seq_partials, seq.hip:311-314 ; Bwd::parts, sasrec.hip:636 with WS::part_stride, sasrec.hip:127
    parts_area = prec == BF16 and d == 64
    parts = bool(parts_area and sw["seq_partials"] and sw["seq_post_bwd"] and lean)
    # fold_sums_partials, sasrec.hip:318-321
    fold_parts = bool(sw["fold_parts"] and parts_area and nl <= 2 and sw["seq_partials"] and sw["seq_post_bwd"] and lean)
    # WS::isort_n, sasrec.hip:129 ; item_det, sasrec.hip:204-207
    sort_area = d == 64 and 2 <= rows <= IS_MAXV1
    det = bool(sw["item_sort"] and sort_area)
    # embed3_on, sasrec.hip:476-479 ; Bwd::lnl_fused, sasrec.hip:640 ; bce_deferred, sasrec.hip:469-473 ; bce_merged, sasrec.hip:481-484
    embed3_on = bool(sw["embed3"] and not det and d == 64)
    lnl_fused = bool(parts and use_seq and sw["lnl_fused"])
    bce_deferred = bool(sw["fwd_fused"] and d == 64 and nl <= 4 and lean)
    # seq_split, sasrec.hip:40-46 ; attn_split, sasrec.hip:278-281
    if sw["seq_split"] > 0:
        split = sw["seq_split"]
    else:
        split = 1
        while split < 8 and B * split * 2 <= 256:
            split *= 2
    attn_split = 2 if sw["attn_split"] and split >= 2 else 1
    # side_sites, sasrec.hip:152-155 ; ADT_SIDE_STREAM_DP, sasrec.hip:644 ; loss_seed_impl, sasrec.hip:1239
    return dict(err=err, use_seq=use_seq, lean=lean, parts=parts, fold_parts=fold_parts, parts_area=parts_area, sort_area=sort_area, det=det, embed3_on=embed3_on,
                lnl_fused=lnl_fused, bce_deferred=bce_deferred, bce_merged=bool(sw["bce_merged"]), seq_split=split, attn_split=attn_split,
                side_sites=sw["side_stream"] & 7, side_dp=bool(sw["side_stream_dp"]), loss_one_launch=nl <= 4)


PLAN_FIELDS = ("use_seq lean parts fold_parts parts_area sort_area det embed3_on lnl_fused bce_deferred bce_merged seq_split attn_split side_sites side_dp "
               "loss_one_launch").split()


def cover_attn_bwd(sw, hd, a):      # adt_launch_seq_attn_bwd, seq.hip:120-132
    if not sw["seq_attn_bwd"] or not a["causal"] or a["H"] * hd != 64 or a["L"] > 224:
        return False
    if any(a[k] % 4 for k in ("ldq", "ldk", "ldv", "ldo")) or (a["in_bf16"] and any(a[k] % 8 for k in ("ldq", "ldk", "ldv", "ldo"))):
        return False
    return sab_lds(a["L"], a["H"]) <= LDS_MAX and head_ok(hd)


def cover_attn_pre_bwd(sw, hd, c):      # adt_launch_seq_attn_pre_bwd, seq.hip:157-165
    return bool(sw["seq_bwd"] and c["wimg"] and c["L"] <= 224 and c["L"] % 4 == 0 and c["H"] * hd == 64 and head_ok(hd))


def cover_mid_bwd(sw, hd, c):      # seq_post_ok, seq.hip:169-172 ; adt_launch_seq_mid_bwd, seq.hip:186-187
    return bool(sw["seq_post_bwd"] and c["wimg"] and c["L"] <= 224 and c["T"] == c["B"] * c["L"] and head_ok(hd))


def cover_post_bwd(sw, hd, enc, c):      # adt_launch_seq_post_bwd, seq.hip:174-176
    return cover_mid_bwd(sw, hd, c) and not (enc and c["drec"] and c["H"] * hd != 64)


def cover_xattn_mid(sw, hd, a, c, handover):      # adt_seq_xattn_mid_covered, seq.hip:204-217
    if not sw["xattn_fused"] or not cover_mid_bwd(sw, hd, c):
        return False
    if not (a["in_bf16"] and a["out_bf16"] and c["saved_bf16"] and c["grad_bf16"] and c["parts4"]) or c["nsplit"] > 1 or c["ablate"]:
        return False
    if not a["causal"] or a["H"] * hd != 64 or a["L"] % 4 or a["L"] > 224 or a["L"] != c["L"] or a["B"] != c["B"]:
        return False
    if (a["dropout"] and not a["keep_bits"]) or any(a[k] % 8 for k in ("ldq", "ldk", "ldv", "ldo")) or a["lddo"] % 4 or not handover:
        return False
    return xm_lds(a["L"], a["H"]) <= LDS_MAX


COVER_FIELDS = "attn_lean attn_cross attn_self pre post_enc post_dec mid xattn".split()


def expect_cover(sw, p, prec, d, H, L, B):
    """The argument blocks the executor builds for that step (the program's step_chain / step_attn), through the launchers' rules."""
    hd = d // H if H >= 1 and d % H == 0 else 0

    def chain(drec):      # Bwd::BA, Bwd::PART, dec_mid_seq_args, enc_post_bwd: sasrec.hip:599-606, :738-745, :946-951
        return dict(L=L, H=H if drec else 0, B=B, T=B * L, wimg=prec == BF16, saved_bf16=p["lean"], grad_bf16=p["lean"] and p["parts"], parts4=p["parts"],
                    nsplit=p["seq_split"], ablate=0, drec=drec)

    def attn(in_bf16, out_bf16, ldq, ldk):      # dec_cross_attn_bwd, dec_cross_attn_lean_args, attn_block_bwd: sasrec.hip:719-726, :751-757, :829
        return dict(L=L, H=H, B=B, causal=1, in_bf16=in_bf16, out_bf16=out_bf16, ldq=ldq, ldk=ldk, ldv=ldk, ldo=d, lddo=d, dropout=1, keep_bits=1)
    pre = dict(chain(False), H=H)
    lean_at = attn(1, p["parts"], d, 2 * d)
    return dict(attn_lean=cover_attn_bwd(sw, hd, lean_at), attn_cross=cover_attn_bwd(sw, hd, attn(0, 0, d, 2 * d)), attn_self=cover_attn_bwd(sw, hd, attn(0, 0, 3 * d, 3 * d)),
                pre=cover_attn_pre_bwd(sw, hd, pre), post_enc=cover_post_bwd(sw, hd, True, chain(1 < H <= 4)), post_dec=cover_post_bwd(sw, hd, False, chain(False)),
                mid=cover_mid_bwd(sw, hd, chain(False)), xattn=cover_xattn_mid(sw, hd, dict(lean_at, out_bf16=1), chain(False), True))


def expect_bwd(word, p):
    """adt_bwd_plan (tests/test_backward_plan_cpu.py) and what bwd_init made of it: sasrec.hip:637, :639, :645 with side_stream, sasrec.hip:159."""
    phase = word & _lib.PHASE_MASK
    here, fwd = bool(word & _lib.PHASE_BCE_HERE), bool(word & _lib.PHASE_BCE_FWD)
    if phase == 3 or ((here or fwd) and not p["bce_deferred"]) or (fwd and (here or not word & _lib.PHASE_PREZEROED or phase == 2)):
        return None
    defer_fold = bool(word & _lib.PHASE_DEFER_FOLD) and phase == 0
    virt = here or fwd or bool(word & _lib.PHASE_SEEDS_VIRTUAL)
    return (defer_fold and p["fold_parts"], virt and p["embed3_on"], p["side_sites"] != 0 and (phase == 0 or p["side_dp"]))


# ---- the program ------------------------------------------------------------------------------------------------------------------------------
MAIN = r"""
#include <stdio.h>
#include "adt_step_plan.h"
static const int ARMS[][%(nsw)d] = {%(arms)s};
static const int BWD_ARMS[] = {%(bwd_arms)s};
static const int HAND[][26] = {%(hand)s};
static const int EDGE[][7] = {%(edge)s};
%(lists)s
// the footprints the library takes from the device headers (adt_seqattn.cuh: sab_lds_bytes ; adt_seqxattn_tt.cuh: xm_rows, xm_lds_bytes)
static size_t sab_lds(int L, int H) { const size_t R = (size_t)((L + 31) / 32 * 32); return 4 * R * 72 * 2 + (size_t)H * R * 8 * 4 + 2 * (size_t)H * R * 4; }
static size_t xm_lds(int L, int H) { const size_t R = (L + 31) / 32 <= 4 ? 128 : 224; return 4 * R * 72 * 2 + (size_t)H * R * 8 * 4 + 2 * (size_t)H * R * 4 + 256 * 4; }
static StepFacts facts(int prec, int L, int d, int H, int nl, int B, int rows) {
  return StepFacts{prec, L, d, H, nl, B, rows, rows >= 2 && rows <= %(maxv1)d, H > 0 ? sab_lds(L, H) : 0};
}
static SeqSwitches switches(const int* v) {
  SeqSwitches s;
  s.seq = v[0]; s.seq_lean = v[1]; s.seq_tt = v[2]; s.seq_bwd = v[3]; s.seq_attn_bwd = v[4]; s.seq_post_bwd = v[5]; s.seq_partials = v[6]; s.xattn_fused = v[7];
  s.seq_ablate = v[8]; s.seq_ablate_set = v[9]; s.seq_split = v[10]; s.attn_split = v[11]; s.side_stream = v[12]; s.side_stream_dp = v[13]; s.item_sort = v[14];
  s.lnl_fused = v[15]; s.fold_parts = v[16]; s.fwd_fused = v[17]; s.embed3 = v[18]; s.bce_merged = v[19];
  return s;
}
// the argument blocks adt_sasrec.hip builds for a step: Bwd::BA + Bwd::PART (drec: the encoder post chain with the head classifier) ...
static SeqChainFacts step_chain(const StepFacts& f, const StepPlan& p, bool drec) {
  SeqChainFacts c{};
  c.L = f.L; c.H = drec ? f.H : 0; c.B = f.B; c.T = f.B * f.L; c.wimg = f.prec == ADT_PREC_BF16; c.saved_bf16 = p.lean; c.grad_bf16 = p.lean && p.parts;
  c.parts4 = p.parts; c.nsplit = p.seq_split; c.ablate = 0; c.drec = drec;
  return c;
}
// ... and the attention backward's (dec_cross_attn_bwd, dec_cross_attn_lean_args, attn_block_bwd)
static SeqAttnFacts step_attn(const StepFacts& f, bool in_bf16, bool out_bf16, int ldq, int ldk) {
  return {f.L, f.H, f.B, true, in_bf16, out_bf16, ldq, ldk, ldk, f.d, f.d, true, true, sab_lds(f.L, f.H), xm_lds(f.L, f.H)};
}
static void step_line(int a, const StepFacts& f) {
  const SeqSwitches sw = switches(ARMS[a]);
  const StepPlan p = adt_step_plan(f, sw);
  const int hd = (f.H >= 1 && f.d %% f.H == 0) ? f.d / f.H : 0;
  SeqChainFacts pre = step_chain(f, p, false);
  pre.H = f.H;
  const SeqAttnFacts lean_at = step_attn(f, true, p.parts, f.d, 2 * f.d);
  SeqAttnFacts fused_at = lean_at;
  fused_at.out_bf16 = true;
  printf("S %%d %%d %%d %%d %%d %%d %%d %%d : %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d : %%d %%d %%d %%d %%d %%d %%d %%d : %%s\n", a, f.prec, f.d, f.H, f.L,
         f.num_layers, f.B, f.rows, (int)p.use_seq, (int)p.lean, (int)p.parts, (int)p.fold_parts, (int)p.parts_area, (int)p.sort_area, (int)p.det,
         (int)p.embed3_on, (int)p.lnl_fused, (int)p.bce_deferred, (int)p.bce_merged, p.seq_split, p.attn_split, p.side_sites, (int)p.side_dp, (int)p.loss_one_launch,
         (int)adt_covers_attn_bwd(sw, hd, lean_at), (int)adt_covers_attn_bwd(sw, hd, step_attn(f, false, false, f.d, 2 * f.d)),
         (int)adt_covers_attn_bwd(sw, hd, step_attn(f, false, false, 3 * f.d, 3 * f.d)), (int)adt_covers_attn_pre_bwd(sw, hd, pre),
         (int)adt_covers_post_bwd(sw, hd, true, step_chain(f, p, f.H > 1 && f.H <= 4)), (int)adt_covers_post_bwd(sw, hd, false, step_chain(f, p, false)),
         (int)adt_covers_mid_bwd(sw, hd, step_chain(f, p, false)), (int)adt_covers_xattn_mid(sw, hd, fused_at, step_chain(f, p, false), true), p.cfg_error);
}
int main() {
  for (int ip = 0; ip < n_FULL0; ++ip) for (int id = 0; id < n_FULL1; ++id) for (int ih = 0; ih < n_FULL2; ++ih) for (int il = 0; il < n_FULL3; ++il)
    for (int in = 0; in < n_FULL4; ++in) for (int ib = 0; ib < n_FULL5; ++ib) for (int ir = 0; ir < n_FULL6; ++ir)
      step_line(0, facts(FULL0[ip], FULL3[il], FULL1[id], FULL2[ih], FULL4[in], FULL5[ib], FULL6[ir]));
  for (int i = 0; i < %(nedge)d; ++i)
    step_line(0, facts(EDGE[i][0], EDGE[i][3], EDGE[i][1], EDGE[i][2], EDGE[i][4], EDGE[i][5], EDGE[i][6]));
  for (int a = 0; a < %(narms)d; ++a)
    for (int ip = 0; ip < n_SOME0; ++ip) for (int id = 0; id < n_SOME1; ++id) for (int ih = 0; ih < n_SOME2; ++ih) for (int il = 0; il < n_SOME3; ++il)
      for (int in = 0; in < n_SOME4; ++in) for (int ib = 0; ib < n_SOME5; ++ib) for (int ir = 0; ir < n_SOME6; ++ir)
        step_line(a, facts(SOME0[ip], SOME3[il], SOME1[id], SOME2[ih], SOME4[in], SOME5[ib], SOME6[ir]));
  for (int ia = 0; ia < %(nbwd_arms)d; ++ia)
    for (int in = 0; in < n_BWDL; ++in) {
      const StepPlan p = adt_step_plan(facts(ADT_PREC_BF16, 200, 64, 2, BWDL[in], 128, 3417), switches(ARMS[BWD_ARMS[ia]]));
      for (int word = 0; word < 128; ++word) {
        BwdPlan b;
        if (adt_bwd_plan(word, p.bce_deferred, &b)) { printf("B %%d %%d %%d reject\n", BWD_ARMS[ia], BWDL[in], word); continue; }
        const BwdCallPlan c = adt_bwd_call_plan(p, b);
        printf("B %%d %%d %%d %%d %%d %%d\n", BWD_ARMS[ia], BWDL[in], word, (int)c.late_parts, (int)c.embed3, (int)c.side);
      }
    }
  for (int i = 0; i < %(nhand)d; ++i) {
    const int* v = HAND[i];
    const SeqAttnFacts a{v[0], v[1], v[2], v[3] != 0, v[4] != 0, v[5] != 0, v[6], v[7], v[8], v[9], v[10], v[11] != 0, v[12] != 0, sab_lds(v[0], v[1]), xm_lds(v[0], v[1])};
    const SeqChainFacts c{v[13], v[14], v[15], v[16], v[17] != 0, v[18] != 0, v[19] != 0, v[20] != 0, v[21], v[22], v[23] != 0};
    const SeqSwitches sw;
    printf("C %%d %%d %%d %%d %%d %%d %%d %%d\n", i, (int)adt_covers_attn_bwd(sw, v[24], a), (int)adt_covers_attn_pre_bwd(sw, v[24], c), (int)adt_covers_mid_bwd(sw, v[24], c),
           (int)adt_covers_post_bwd(sw, v[24], true, c), (int)adt_covers_post_bwd(sw, v[24], false, c), (int)adt_covers_xattn_mid(sw, v[24], a, c, v[25] != 0),
           (int)adt_seq_fwd_tt(sw, c.wimg, c.L));
  }
  for (int L = 1; L <= 256; ++L)
    for (int H = 1; H <= 4; H *= 2) printf("L %%d %%d %%zu %%zu\n", L, H, sab_lds(L, H), xm_lds(L, H));
  return 0;
}
"""
ATT_KEYS = "L H B causal in_bf16 out_bf16 ldq ldk ldv ldo lddo dropout keep_bits".split()
CH_KEYS = "L H B T wimg saved_bf16 grad_bf16 parts4 nsplit ablate drec".split()


def c_rows(rows):
    return ", ".join("{" + ", ".join(str(int(v)) for v in r) + "}" for r in rows)


def main_source():
    lists = []
    for name, lst in [("FULL%d" % i, v) for i, v in enumerate(FULL)] + [("SOME%d" % i, v) for i, v in enumerate(SOME)] + [("BWDL", BWD_LAYERS)]:
        lists.append("static const int %s[] = {%s}; static const int n_%s = %d;" % (name, ", ".join(map(str, lst)), name, len(lst)))
    hand = [[dict(ATT0, **a)[k] for k in ATT_KEYS] + [dict(CH0, **c)[k] for k in CH_KEYS] + [hd, ho] for a, c, hd, ho in HAND]
    return MAIN % dict(nsw=len(SWITCHES), arms=c_rows([[a[k] for k in SWITCHES] for a in ARMS]), bwd_arms=", ".join(map(str, BWD_ARMS)), hand=c_rows(hand),
                       lists="\n".join(lists), edge=c_rows(EDGE), nedge=len(EDGE), maxv1=IS_MAXV1, narms=len(ARMS), nbwd_arms=len(BWD_ARMS), nhand=len(HAND))


def step_cases():
    for c in itertools.product(*FULL):
        yield (0,) + c
    for c in EDGE:
        yield (0,) + c
    for a in range(len(ARMS)):
        for c in itertools.product(*SOME):
            yield (a,) + c


@pytest.fixture(scope="module", params=[[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]], ids=["plain", "asan-ubsan"])
def table(request, tmp_path_factory):
    """The program's output lines by tag: {"S": [...], "B": [...], "C": [...], "L": [...]}."""
    tmp = tmp_path_factory.mktemp("step_plan")
    src, exe = tmp / "step_plan_main.cpp", tmp / "step_plan_main"
    src.write_text(main_source())
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "adt_amd", "csrc")] +
                          request.param + ["-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
    lines = {}
    for line in out.stdout.splitlines():
        lines.setdefault(line[0], []).append(line)
    return lines


@pytest.fixture(scope="module")
def expected_steps():
    """(case, plan, coverage) per step line, computed once for both builds."""
    rows = []
    for case in step_cases():
        a, prec, d, H, L, nl, B, rows_ = case
        p = expect_plan(ARMS[a], prec, d, H, L, nl, B, rows_)
        rows.append((case, p, expect_cover(ARMS[a], p, prec, d, H, L, B)))
    return rows


def test_header_is_plain_cpp():
    """No HIP and no environment in the header: nothing from ROCm on the include path of the builds above, and no such word in the text."""
    text = open(os.path.join(REPO, "adt_amd", "csrc", "adt_step_plan.h")).read()
    for word in ("hip/", "__global__", "__device__", "getenv", "adt_env_"):
        assert word not in text, word


def test_switch_struct_defaults_and_design_table():
    """SeqSwitches declares every switch with the default this file assumes, and DESIGN.md's table of the flagship switches lists the same names,
    defaults and descriptions as the struct's field comments."""
    import re
    text = open(os.path.join(REPO, "adt_amd", "csrc", "adt_step_plan.h")).read()
    fields = re.findall(r"^  (?:bool|int) (\w+) = (\w+);\s*// (ADT_\w+)?\s*(.*)$", text[text.index("struct SeqSwitches"):text.index("};", text.index("struct SeqSwitches"))], re.M)
    assert [f[0] for f in fields] == SWITCHES
    assert {f[0]: {"true": 1, "false": 0}[f[1]] if f[1] in ("true", "false") else int(f[1]) for f in fields} == DEFAULT
    rows = re.findall(r"^\| `(ADT_\w+)` \| (\w+) \| (.*) \|$", open(os.path.join(REPO, "DESIGN.md")).read(), re.M)
    want = [(f[2], {"true": "on", "false": "off"}.get(f[1], f[1]), f[3].strip()) for f in fields if f[2]]
    assert rows == want, [(a, b) for a, b in zip(rows, want) if a != b][:3]
    assert [r[0] for r in rows] == ["ADT_" + k.upper() for k in SWITCHES if k != "seq_ablate_set"]


def test_arm_list():
    assert len(ARMS) == N_NAMED + 256 and ARMS[0] == DEFAULT and ARMS[-1] == DEFAULT
    assert [sorted(k for k in SWITCHES if a[k] != DEFAULT[k]) for a in ARMS[1:1 + len(ON_OFF)]] == [[k] for k in ON_OFF]
    assert ARMS[BWD_ARMS[5]]["item_sort"] == 1 and ARMS[BWD_ARMS[6]]["side_stream_dp"] == 1 and ARMS[BWD_ARMS[7]]["side_stream"] == 0
    assert {a["side_stream"] for a in ARMS} >= set(range(8)) and {a["seq_split"] for a in ARMS} == {0, 1, 2}
    assert any(a["seq_ablate_set"] and a["seq_ablate"] == 0 for a in ARMS)


def test_step_table(table, expected_steps):
    assert len(table["S"]) == len(expected_steps)
    want = []
    for case, p, cov in expected_steps:
        want.append("S %s : %s : %s : %s" % (" ".join(map(str, case)), " ".join(str(int(p[k])) for k in PLAN_FIELDS), " ".join(str(int(cov[k])) for k in COVER_FIELDS),
                                             p["err"]))
    assert table["S"] == want, [(a, b) for a, b in zip(table["S"], want) if a != b][:5]


def test_every_field_takes_every_value(expected_steps):
    seen = {}
    for _, p, cov in expected_steps:
        for k in PLAN_FIELDS:
            seen.setdefault(k, set()).add(int(p[k]))
        for k in COVER_FIELDS:
            seen.setdefault(k, set()).add(int(cov[k]))
        seen.setdefault("err", set()).add(p["err"].split("=")[0].split(" >")[0])
    for k in PLAN_FIELDS + COVER_FIELDS:
        if k not in ("seq_split", "attn_split", "side_sites"):
            assert seen[k] == {0, 1}, (k, seen[k])
    assert seen["seq_split"] == {1, 2, 4, 8} and seen["attn_split"] == {1, 2} and seen["side_sites"] == set(range(8))
    assert seen["err"] == {"", "sasrec: hidden", "sasrec: bad num_heads", "sasrec: head_dim", "sasrec: maxlen", "sasrec: num_layers"}, seen["err"]


def test_the_flagship_row_and_the_known_edges(expected_steps):
    by = {case: (p, cov) for case, p, cov in expected_steps}
    p, cov = by[(0, BF16, 64, 2, 200, 2, 256, 3417)]      # the benchmarked shape, library defaults
    assert [int(p[k]) for k in PLAN_FIELDS] == [1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 7, 0, 1] and not p["err"] and all(cov.values())
    assert [by[(0, BF16, 64, 2, 200, 2, B, 3417)][0]["seq_split"] for B in (1, 16, 32, 64, 128, 129, 256)] == [8, 8, 8, 4, 2, 1, 1]
    assert not by[(0, BF16, 64, 2, 200, 2, 128, 3417)][1]["xattn"]      # two workgroups per sequence: the two launches
    assert by[(0, BF16, 64, 2, 200, 3, 128, 3417)][0]["fold_parts"] is False and by[(0, BF16, 64, 2, 200, 5, 128, 3417)][0]["bce_deferred"] is False
    four = by[(0, BF16, 64, 4, 200, 2, 128, 3417)]      # four 16-wide heads: k_seq_attn_bwd's images fit up to L = 192, the fused launch's up to 128
    assert not four[0]["lean"] and four[0]["use_seq"] and not four[1]["attn_lean"] and by[(0, BF16, 64, 4, 128, 2, 256, 3417)][1]["xattn"]
    assert by[(0, BF16, 64, 2, 202, 2, 128, 3417)][0]["lean"] is False and by[(0, BF16, 64, 2, 202, 2, 128, 3417)][0]["use_seq"]
    assert by[(0, F32, 64, 2, 200, 2, 128, 3417)][0]["use_seq"] is False and by[(0, BF16, 64, 2, 200, 2, 128, 16001)][0]["sort_area"] is False
    assert by[(0, BF16, 64, 8, 200, 2, 128, 3417)][0]["err"] == "sasrec: head_dim=8 unsupported (16/32/64)"
    assert {by[(0,) + c][0]["err"] for c in EDGE[:4]} == {"sasrec: bad num_heads"} and by[(0,) + EDGE[4]][0]["err"] == "sasrec: num_layers"
    assert [by[(0,) + c][0]["err"] for c in EDGE[5:]] == [""] * 4 and not by[(0,) + EDGE[7]][0]["sort_area"] and not by[(0,) + EDGE[8]][0]["use_seq"]
    assert by[(0, BF16, 64, 2, 225, 2, 128, 3417)][0]["err"] == "sasrec: maxlen=225 > 224 unsupported"
    ablate0 = next(i for i, a in enumerate(ARMS) if a["seq_ablate_set"] and a["seq_ablate"] == 0)
    assert by[(ablate0, BF16, 64, 2, 200, 2, 128, 3417)][0]["lean"] is False and by[(ablate0, BF16, 64, 2, 200, 2, 128, 3417)][0]["use_seq"]


def test_chosen_paths_are_covered(expected_steps):
    """What the three defensive errors of the executor stand for: wherever the plan chooses the lean forward or the partial-gradient path, every
    per-sequence launcher the backward then depends on covers the argument blocks it gets."""
    n_lean = n_parts = 0
    for case, p, cov in expected_steps:
        if p["lean"]:      # dec_cross_attn_bwd -> adt_attn_bwd_saved_bf16 ; attn_block_bwd -> adt_launch_seq_attn_pre_bwd
            n_lean += 1
            assert p["use_seq"] and cov["attn_lean"] and cov["pre"], case
        if p["parts"]:      # dec_post_bwd, enc_post_bwd, dec_mid_bwd (NO_FALLBACK)
            n_parts += 1
            assert p["lean"] and cov["post_enc"] and cov["post_dec"] and cov["mid"], case
        if p["fold_parts"] or p["lnl_fused"]:
            assert p["parts"], case
        if p["bce_deferred"]:
            assert p["lean"] and p["loss_one_launch"], case
    assert n_lean > n_parts > 1000


def test_backward_call_table(table):
    want, seen = [], set()
    for a in BWD_ARMS:
        for nl in BWD_LAYERS:
            p = expect_plan(ARMS[a], BF16, 64, 2, 200, nl, 128, 3417)
            for word in range(128):
                e = expect_bwd(word, p)
                want.append("B %d %d %d reject" % (a, nl, word) if e is None else "B %d %d %d %d %d %d" % ((a, nl, word) + tuple(int(v) for v in e)))
                seen.add(e)
    assert table["B"] == want, [(a, b) for a, b in zip(table["B"], want) if a != b][:5]
    assert None in seen and all({bool(v[i]) for v in seen if v is not None} == {False, True} for i in range(3))
    rows = {tuple(int(x) for x in line.split()[1:4]): line.split()[4:] for line in table["B"]}
    # the single-GPU step (bits 2, 3, 5: 44), the data-parallel halves (1 | 4 | 32, 2 | 64), and the two-phase side stream only by its switch
    assert rows[(0, 2, 44)] == ["1", "1", "1"] and rows[(0, 3, 44)] == ["0", "1", "1"] and rows[(0, 2, 37)] == ["0", "1", "0"] and rows[(0, 2, 66)] == ["0", "1", "0"]
    assert rows[(BWD_ARMS[6], 2, 37)] == ["0", "1", "1"] and rows[(BWD_ARMS[7], 2, 44)] == ["1", "1", "0"] and rows[(BWD_ARMS[5], 2, 44)] == ["1", "0", "1"]
    assert rows[(BWD_ARMS[3], 2, 44)] == ["reject"] and rows[(BWD_ARMS[3], 2, 12)] == ["1", "0", "1"]


def test_launcher_rules_by_hand(table):
    want = []
    for i, (da, dc, hd, ho) in enumerate(HAND):
        a, c = dict(ATT0, **da), dict(CH0, **dc)
        v = (cover_attn_bwd(DEFAULT, hd, a), cover_attn_pre_bwd(DEFAULT, hd, c), cover_mid_bwd(DEFAULT, hd, c), cover_post_bwd(DEFAULT, hd, True, c),
             cover_post_bwd(DEFAULT, hd, False, c), cover_xattn_mid(DEFAULT, hd, a, c, ho), bool(c["wimg"] and c["L"] % 4 == 0))
        want.append("C %d %s" % (i, " ".join(str(int(x)) for x in v)))
    assert table["C"] == want, [(a, b) for a, b in zip(table["C"], want) if a != b][:5]
    cols = list(zip(*[line.split()[2:] for line in table["C"]]))
    assert all(set(col) == {"0", "1"} for col in cols), [set(col) for col in cols]
    assert table["C"][0] == "C 0 1 1 1 1 1 1 1"
    # one changed fact each: the rule that reads it, and only that launcher's
    got = {(tuple(sorted(da.items())), tuple(sorted(dc.items())), hd, ho): line.split()[2:] for (da, dc, hd, ho), line in zip(HAND, table["C"])}
    assert got[((("ldq", 68),), (), 32, 1)] == ["0", "1", "1", "1", "1", "0", "1"] and got[((("in_bf16", 0), ("ldq", 68)), (), 32, 1)][0] == "1"
    assert got[((("in_bf16", 0), ("ldq", 66)), (), 32, 1)][0] == "0" and got[((("lddo", 66),), (), 32, 1)] == ["1", "1", "1", "1", "1", "0", "1"]
    assert got[((("keep_bits", 0),), (), 32, 1)][5] == "0" and got[((("dropout", 0), ("keep_bits", 0)), (), 32, 1)][5] == "1"
    assert got[((), (("nsplit", 2),), 32, 1)] == ["1", "1", "1", "1", "1", "0", "1"] and got[((), (), 32, 0)] == ["1", "1", "1", "1", "1", "0", "1"]
    assert got[((), (("T", 25599),), 32, 1)] == ["1", "1", "0", "0", "0", "0", "1"] and got[((), (("wimg", 0),), 32, 1)] == ["1", "0", "0", "0", "0", "0", "0"]
    assert got[((("H", 4),), (("H", 4), ("drec", 1)), 32, 1)][3:5] == ["0", "1"]      # the classifier reverse needs H hd = 64


def test_lds_footprints(table):
    """The program's and this file's restatement of the two device-header footprints agree; the library itself passes the device functions' values
    in as facts (StepFacts::sab_lds, SeqAttnFacts::sab_lds / xm_lds)."""
    want = ["L %d %d %d %d" % (L, H, sab_lds(L, H), xm_lds(L, H)) for L in range(1, 257) for H in (1, 2, 4)]
    assert table["L"] == want
    # adt_seqxattn_tt.cuh's header: 147,968 B at L > 128 with two heads, 84,992 B at L <= 128 ; four heads fit up to L = 128 only
    assert xm_lds(200, 2) == 147968 and xm_lds(128, 2) == 84992 and xm_lds(128, 4) <= LDS_MAX < xm_lds(129, 4)
    assert sab_lds(192, 4) <= LDS_MAX < sab_lds(193, 4) and sab_lds(224, 2) <= LDS_MAX
