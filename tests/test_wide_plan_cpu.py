"""CPU: which kernel a call of the wide C ABI gets (adt_dense_fwd, adt_dense_bwd, adt_attn_masked_*) as adt_amd/csrc/adt_wide_plan.h decides it.
A stand-alone host program (plain g++, no HIP) prints one line per case; the expected lines are restated here from the rules the launchers of
adt_wide.hip applied before the plan header existed, each group citing its rule.  Built and run a second time with -fsanitize=address,undefined."""
import math
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GBM, GBK, GTH = 128, 32, 256
DWP_TS, DWP_NTH, DWP_IMG = 32, 512, 32 * 256 * 2
DW64_ROWS, DW64_NTH, DW64_PART = 128, 256, 4096 + 64
ROWS_NW, ROWS_PC = 8, 256
DW_BN, DW_BK, DW_TS, DW_NTH, DW_LDS = 256, 128, 64, 512, 2 * (8 * 256 * 8 + 8 * 128 * 8) * 2
LDS_MAX = 160 * 1024
WS = 64 << 20
F32, BF16 = 0, 1

FACT_FIELDS = ("prec T K N has_bias has_u has_r has_r2 has_mask has_drop has_act has_dx has_dw beta "
               "x_ok w_ok g_ok bias_ok u_ok r_ok r2_ok dx_ok rows_on stage256_on ws_bytes").split()


def facts(T, K, N, **kw):
    """bf16, every operand aligned, both switches on, the 64 MiB workspace registered; the optional operands absent."""
    f = dict.fromkeys(FACT_FIELDS, 0)
    f.update(prec=BF16, T=T, K=K, N=N, x_ok=1, w_ok=1, g_ok=1, bias_ok=1, u_ok=1, r_ok=1, r2_ok=1, dx_ok=1, rows_on=1, stage256_on=1, ws_bytes=WS)
    assert set(kw) <= set(FACT_FIELDS), kw
    f.update(kw)
    return f


def ceil(a, b):
    return (a + b - 1) // b


def rnd(a, b):
    return ceil(a, b) * b


def xcd_grid(n_outer, n_inner):      # adt_gemm.cuh: XCD-aware 1-D launch
    return n_outer * n_inner if n_outer < 16 else ceil(n_outer, 8) * 8 * n_inner


def gemm_lds(prec, bn):      # adt_gemm.cuh: GemmLds (fp32 rows of 36 floats, bf16 rows of 40) and gemm_lds_bytes
    return (GBM + bn) * (40 * 2 if prec != F32 else 36 * 4)


def rows_grid(T, cols, contraction):
    """rows_launch and its callers: panel of <= 256 columns (a multiple of 16), LDS = panel x (contraction + 8) bf16 + panel floats, one workgroup
    per CU and panel group, twice that at <= 64 KB, never more row groups than 16-row tiles / 8 waves."""
    pc = ROWS_PC if cols >= ROWS_PC else rnd(cols, 16)
    n_panels = ceil(cols, pc)
    lds = pc * (contraction + 8) * 2 + pc * 4
    nrg = 256 // n_panels
    if lds <= 64 * 1024:
        nrg *= 2
    nrg = max(min(nrg, ceil(ceil(T, 16), ROWS_NW)), 1)
    return pc, n_panels, nrg, lds


def present_ok(f, *names):
    return all(not f["has_" + n] or f[n + "_ok"] for n in names)


def expect_fwd(f):
    """launch_dense_fwd: k_dense_fwd256 ahead of the row-streaming kernel ahead of the tiled one.
    (arm, grid_x, grid_y, block, lds, chunk, epi, pc, n_panels, row_groups, kb, ch, bn, nt_m, nt_n)"""
    T, K, N, bf16 = f["T"], f["K"], f["N"], f["prec"] != F32
    if (bf16 and f["rows_on"] and K == 256 and N % 256 == 0 and N <= 1024 and f["x_ok"] and f["w_ok"] and f["g_ok"] and present_ok(f, "u", "r", "r2")
            and f["stage256_on"]):
        nwg = min(ceil(T, DWP_TS), 512 // (N // 256) if N > 256 else 256)
        chunk = rnd(ceil(T, nwg), DWP_TS)
        epi = (1 if f["has_r"] or f["has_r2"] or f["has_mask"] else 0) | (2 if f["has_drop"] else 0) | (4 if f["has_act"] or f["has_u"] else 0)
        return ("F256", ceil(T, chunk), N // 256, DWP_NTH, 0, chunk, epi, 0, 0, 0, 0, 0, 0, 0, 0)
    # rows_fwd_ok
    if bf16 and f["rows_on"] and K in (64, 128, 256) and N % 4 == 0 and f["g_ok"] and present_ok(f, "bias", "u", "r", "r2"):
        pc, n_panels, nrg, lds = rows_grid(T, N, K)
        return ("FROWS", nrg * n_panels, 1, ROWS_NW * 64, lds, 0, 0, pc, n_panels, nrg, K // 32, 4 if f["has_r2"] else 8, 0, 0, 0)
    bn, nt_n, nt_m = (128, ceil(N, 128), ceil(T, GBM)) if N > 64 else (64, 1, ceil(T, GBM))
    return ("FTILED", xcd_grid(nt_m, nt_n), 1, GTH, gemm_lds(f["prec"], bn), 0, 0, 0, 0, 0, 0, 0, bn, nt_m, nt_n)


def expect_dx(f):
    """launch_dense_bwd, dX: k_dense_dx256 ahead of the row-streaming pieces (rows_dx_ok, launch_dense_dx_rows) ahead of the tiled kernel with its
    split of N.  (arm, grid_x, grid_y, block, lds, nb, chunk, n_pieces, pc, n_panels, has_u, pieces, bn, gx, gy, splits, n_chunk, zero_fill)"""
    T, K, N, bf16 = f["T"], f["K"], f["N"], f["prec"] != F32
    act_ok = not f["has_act"] or f["u_ok"]
    if not f["has_dx"]:
        return ("DXNONE", 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, "-", 0, 0, 0, 0, 0, 0)
    if bf16 and f["rows_on"] and N % 256 == 0 and N <= 768 and K == 256 and f["w_ok"] and f["g_ok"] and act_ok and f["stage256_on"]:
        chunk = rnd(ceil(T, min(ceil(T, DWP_TS), 256)), DWP_TS)
        return ("DX256", ceil(T, chunk), K // 256, DWP_NTH, DWP_IMG * (N // 256), N // 256, chunk, 0, 0, 0, 0, "-", 0, 0, 0, 0, 0, 0)
    if bf16 and f["rows_on"] and N % 64 == 0 and N <= 1024 and K % 4 == 0 and f["dx_ok"] and f["g_ok"] and act_ok:
        pieces, n0 = [], 0
        while n0 < N:      # with an activation: contraction chunks of 128 instead of 256
            chunk = 256 if (N - n0 >= 256 and not f["has_act"]) else (128 if N - n0 >= 128 else 64)
            pc, n_panels, nrg, lds = rows_grid(T, K, chunk)
            pieces.append("%d:%d:%d:%d:%d:%d" % (n0, chunk, 1 if n0 > 0 or f["beta"] else 0, chunk // 32, nrg, lds))
            n0 += chunk
        return ("DXROWS", 0, 0, ROWS_NW * 64, 0, 0, 0, len(pieces), pc, n_panels, f["has_act"], ",".join(pieces), 0, 0, 0, 0, 0, 0)
    gx, gy = (ceil(K, 128) if K > 64 else 1), ceil(T, GBM)
    splits, n_chunk, zero = 1, 0, 0
    if N >= 4096 and gx * gy < 1024:
        splits = min(ceil(2048, gx * gy), 32)
        n_chunk = rnd(ceil(N, splits), GBK)
        splits = ceil(N, n_chunk)
        zero = int(splits > 1 and not f["beta"])
    bn = 128 if K > 64 else 64
    return ("DXTILED", xcd_grid(gy, gx * splits), 1, GTH, gemm_lds(f["prec"], bn), 0, 0, 0, 0, 0, 0, "-", bn, gx, gy, splits, n_chunk, zero)


def expect_dw(f):
    """launch_dense_bwd, dW: k_dense_dw256 + reduce ahead of k_dense_dw_rows ahead of k_dense_dw64 ahead of the tiled kernel with its three measured
    work-group targets.  (arm, grid_x, grid_y, block, lds, chunk, nwg, blocks, kblocks, per, reduce_groups, ws_used, partials, splits, n_blocks,
    k_blocks, bn, gx, gy)"""
    T, K, N, bf16, ws = f["T"], f["K"], f["N"], f["prec"] != F32, f["ws_bytes"]
    rows = bf16 and f["rows_on"] and f["x_ok"] and f["g_ok"]
    if not f["has_dw"]:
        return ("DWNONE",) + (0,) * 18
    if rows and N % 256 == 0 and K % 256 == 0 and (N // 256) * (K // 256) <= 4:
        blocks = (N // 256) * (K // 256)
        nwg = min(ceil(T, DWP_TS), 256 // blocks)
        need = nwg * blocks * 262144
        if need <= ws:
            chunk = rnd(ceil(T, nwg), DWP_TS)
            nwg = ceil(T, chunk)
            per = 32 if nwg >= 128 else 16
            return ("DW256", nwg, blocks, DWP_NTH, 0, chunk, nwg, blocks, K // 256, per, ceil(nwg, per), need, 0, 0, 0, 0, 0, 0, 0)
    if rows and ceil(N, DW_BN) * ceil(K, DW_BK) >= 4 and N % 4 == 0 and K % 4 == 0 and (not f["has_act"] or f["u_ok"]):
        n_blocks, k_blocks = ceil(N, DW_BN), ceil(K, DW_BK)
        tiles = n_blocks * k_blocks
        chunk = max(rnd(ceil(T, 1 if tiles >= 256 else 256 // tiles), DW_TS), DW_TS)
        splits = ceil(T, chunk)
        return ("DWROWS", xcd_grid(splits, tiles), 1, DW_NTH, DW_LDS, chunk, 0, 0, 0, 0, 0, 0, 0, splits, n_blocks, k_blocks, 0, 0, 0)
    if rows and N % 64 == 0 and K % 64 == 0 and (N // 64) * (K // 64) <= 4:
        chunk = max(rnd(ceil(T, 256), DW64_ROWS), DW64_ROWS)
        nwg, blocks = ceil(T, chunk), (N // 64) * (K // 64)
        need = nwg * blocks * DW64_PART * 4
        part = int(need <= ws)
        return ("DW64", nwg, blocks, DW64_NTH, 0, chunk, nwg, blocks, K // 64, 0, 0, need if part else 0, part, 0, 0, 0, 0, 0, 0)
    bn = 128 if K > 64 else 64
    gx, gy = ceil(K, bn), ceil(N, GBM)
    tiles = gx * gy
    target = 512 if tiles <= 4 else (2048 if tiles <= 12 else 1024)
    chunk = max(rnd(ceil(T, ceil(target, tiles)), GBK), GBK)
    splits = ceil(T, chunk)
    return ("DWTILED", xcd_grid(splits, tiles), 1, GTH, gemm_lds(f["prec"], bn), chunk, 0, 0, 0, 0, 0, 0, 0, splits, 0, 0, bn, gx, gy)


def esz(prec):
    return 4 if prec == F32 else 2


def lds_resident(prec, hd, maxkt, bwd):      # adt_attn_gen.cuh: AttnGenLds
    lp = maxkt * 16
    img = lp * (hd + 8) + hd * (lp + 8)
    return 2 * img * esz(prec) + 2 * lp * 4 + 2 * lp * 4 if bwd else img * esz(prec) + 2 * lp * 4


def lds_chunked(prec, hd, maxkt, nch):      # adt_attn_gen.cuh: AttnChunkLds
    lp = maxkt * 16
    lpc = lp // nch
    return 2 * (lpc * (hd + 8) + hd * (lpc + 8)) * esz(prec) + 2 * lp * 4 + 2 * lp * 4


def lds_streamed(prec, hd, kc, bwd):      # adt_attn_long.cuh: AttnLongLds at 256 rows (LSE + delta in the backward, 256 validity bytes + 32)
    img = kc * (hd + 8) + hd * (kc + 8)
    return 2 * img * esz(prec) + 2 * 256 * 4 + 256 + 32 if bwd else img * esz(prec) + 256 + 32


def expect_attn(prec, hd, L, bwd, causal, kid, fill):
    """dispatch_attn_gen, dispatch_attn_gen_l, launch_attn_gen_128, launch_attn_gen, launch_attn_gen_bwd_chunked, launch_attn_stream.
    An error text, or (family, maxkt, nch, kc, waves, csk, grid_y, lds)."""
    bf16 = prec != F32

    def resident(maxkt, csk=0):
        lds = lds_resident(prec, hd, maxkt, bwd)
        if lds > LDS_MAX:
            return "masked attention: L=%d hd=%d prec=%d needs %d B of LDS (> 160 KB)" % (L, hd, prec, lds)
        waves = (16 if bf16 and hd <= 64 else 8) if bwd else (16 if bf16 else 8)
        return ("RESIDENT", maxkt, 1, 0, waves, csk, 1, lds)

    def chunked(maxkt, nch):
        lds = lds_chunked(prec, hd, maxkt, nch)
        if lds > LDS_MAX:
            return "masked attention bwd: L=%d hd=%d prec=%d needs %d B of LDS (> 160 KB)" % (L, hd, prec, lds)
        return ("CHUNKED", maxkt, nch, 0, 8, 0, 1, lds)

    def streamed(maxkt, nch):
        kc = 32 if bwd or not bf16 else 64
        lds = lds_streamed(prec, hd, kc, bwd)
        if lds > LDS_MAX:
            return "masked attention: hd=%d prec=%d needs %d B of LDS (> 160 KB)" % (hd, prec, lds)
        return ("STREAMED", maxkt, nch, kc, 4, 0, ceil(ceil(L, 16), 4), lds)

    if hd in (16, 32, 64):
        if L <= 64:
            return resident(4)
        if L <= 128:
            return resident(8)
        if L <= 224:
            if not bf16 and hd == 64 and bwd:
                return chunked(16, 2)
            return resident(14)
        return "masked attention: L=%d > 224 unsupported" % L
    if hd == 128:
        if L > 256:
            return "masked attention: L=%d > 256 unsupported at head_dim 128" % L
        maxkt, nch = (4, 1) if L <= 64 else (16, 2)
        if not bf16 and (lds_chunked(prec, hd, maxkt, nch) if bwd else lds_resident(prec, hd, maxkt, False)) > LDS_MAX:
            return streamed(maxkt, nch)
        if not bwd:
            res = resident(maxkt, int(bool(causal) and not kid and fill <= -1e9))
            return res if isinstance(res, str) else res[:2] + (nch,) + res[3:]
        return chunked(maxkt, nch)
    if hd == 256:
        if 1 <= L <= 256:
            return streamed(0, 1)
        return "masked attention: L=%d outside 1..256 at head_dim 256" % L
    return "masked attention: head_dim=%d unsupported (16/32/64/128/256)" % hd


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
FWD = [facts(100, 256, 256), facts(100, 256, 1024), facts(51200, 256, 256), facts(51200, 256, 1024), facts(51200, 256, 512)]
FWD += [facts(700, 256, 768, has_r=e & 1, has_drop=(e >> 1) & 1, has_act=(e >> 2) & 1) for e in range(8)]      # every epilogue
FWD += [facts(700, 256, 256, has_mask=1), facts(700, 256, 256, has_r2=1), facts(700, 256, 256, has_u=1)]
FWD += [facts(700, 256, 256, stage256_on=0), facts(700, 256, 256, rows_on=0), facts(700, 256, 1280), facts(700, 256, 200)]
FWD += [facts(100, 256, 100), facts(700, 64, 320), facts(700, 128, 320), facts(700, 128, 320, has_r=1, has_r2=1), facts(51200, 64, 64), facts(48, 64, 256)]
FWD += [facts(700, 96, 64), facts(700, 96, 65), facts(700, 96, 320), facts(5000, 96, 50), facts(700, 128, 102)]
FWD += [facts(700, K, N, prec=F32) for K, N in ((256, 256), (64, 64), (128, 320), (96, 100))]
FWD += [facts(700, 256, 256, g_ok=0), facts(700, 64, 64, g_ok=0), facts(700, 256, 256, has_r=1, r_ok=0), facts(700, 256, 256, has_u=1, u_ok=0),
        facts(700, 64, 64, has_bias=1, bias_ok=0), facts(700, 256, 256, has_bias=1, bias_ok=0), facts(700, 256, 256, r_ok=0, r2_ok=0, u_ok=0, bias_ok=0)]

BWD = [facts(1000, 256, N, has_dx=1, has_dw=1) for N in (256, 512, 768, 1024)]
BWD += [facts(1000, 256, N, has_dx=1, has_act=1, has_u=1, beta=b) for N in (448, 768, 1024) for b in (0, 1)]
BWD += [facts(1000, 256, 448, has_dx=1, beta=b) for b in (0, 1)]
BWD += [facts(1000, 256, 100, has_dx=1), facts(128, 64, 4096, has_dx=1), facts(128, 64, 4096, has_dx=1, beta=1), facts(300, 256, 8292, has_dx=1),
        facts(51200, 256, 4196, has_dx=1), facts(1000, 256, 256, has_dx=1, stage256_on=0), facts(1000, 256, 256, has_dx=1, rows_on=0),
        facts(1000, 256, 512, has_dx=1, has_act=1, has_u=1, u_ok=0), facts(1000, 256, 1024, has_dx=1, dx_ok=0), facts(1000, 256, 256, has_dx=1, prec=F32),
        facts(1000, 64, 64, has_dx=1, prec=F32), facts(1000, 1024, 256, has_dx=1), facts(1000, 50, 64, has_dx=1)]
DW_WS = ((256, 256), (768, 256), (1024, 256), (256, 512))
BWD += [facts(T, K, N, has_dw=1, ws_bytes=ws) for (N, K) in DW_WS for T in (1000, 4100, 51200) for ws in (WS, 0)]
BWD += [facts(51200, 256, 256, has_dw=1, ws_bytes=256 * 262144 - 1), facts(51200, 256, 256, has_dw=1, ws_bytes=256 * 262144)]
BWD += [facts(T, K, N, has_dw=1, ws_bytes=ws) for (N, K) in ((64, 64), (128, 128), (256, 64), (64, 256)) for T in (4100, 51200) for ws in (WS, 0)]
BWD += [facts(51200, 64, 64, has_dw=1, ws_bytes=200 * DW64_PART * 4 - 1), facts(51200, 64, 64, has_dw=1, ws_bytes=200 * DW64_PART * 4)]
BWD += [facts(1000, 96, 100, has_dw=1), facts(51200, 128, 128, has_dw=1, rows_on=0), facts(51200, 256, 768, has_dw=1, rows_on=0),
        facts(51200, 256, 1024, has_dw=1, rows_on=0), facts(51200, 64, 64, has_dw=1, prec=F32), facts(10, 64, 64, has_dw=1, rows_on=0),
        facts(1000, 1024, 1024, has_dw=1), facts(1000, 1024, 1024, has_dw=1, ws_bytes=0), facts(1000, 256, 768, has_dw=1, has_act=1, has_u=1, u_ok=0, ws_bytes=0),
        facts(1000, 256, 256, has_dw=1, x_ok=0), facts(1000, 128, 1024, has_dw=1), facts(1000, 512, 128, has_dw=1)]

ATTN = [(prec, hd, L, bwd, 0, 0, -1e9) for prec in (F32, BF16) for hd in (16, 32, 64) for L in (64, 65, 128, 129, 200, 224, 225) for bwd in (0, 1)]
ATTN += [(prec, 128, L, bwd, causal, kid, fill) for prec in (F32, BF16) for L in (64, 200, 256, 257) for bwd in (0, 1)
         for causal, kid, fill in ((1, 0, -1e9), (1, 1, -1e9), (0, 0, -1e9), (1, 0, -1e4), (1, 0, -math.inf))]
ATTN += [(prec, 256, L, bwd, 1, 0, -1e9) for prec in (F32, BF16) for L in (0, 1, 100, 256, 257) for bwd in (0, 1)]
ATTN += [(BF16, 48, 50, 0, 0, 0, -1e9), (F32, 8, 50, 1, 0, 0, -1e9), (BF16, 16, 0, 0, 0, 0, -1e9), (7, 64, 200, 1, 0, 0, -1e9)]

QUERY = sorted({(f["prec"], f["T"], f["K"], f["N"]) for f in BWD} | {(BF16, 0, 64, 64), (BF16, 1000, 1024, 1024)})

MAIN = r"""
#include <math.h>
#include <stdio.h>
#include "adt_wide_plan.h"
using namespace adt;
static const long long DENSE[][%(nfacts)d] = {%(dense)s};
static const double ATTN[][7] = {%(attn)s};
static const int QUERY[][4] = {%(query)s};
static DenseFacts facts_of(const long long* v) {
  DenseFacts f{};
  f.prec = (int)v[0]; f.T = (int)v[1]; f.K = (int)v[2]; f.N = (int)v[3];
  f.has_bias = v[4]; f.has_u = v[5]; f.has_r = v[6]; f.has_r2 = v[7]; f.has_mask = v[8]; f.has_drop = v[9]; f.has_act = v[10]; f.has_dx = v[11];
  f.has_dw = v[12]; f.beta = v[13]; f.x_ok = v[14]; f.w_ok = v[15]; f.g_ok = v[16]; f.bias_ok = v[17]; f.u_ok = v[18]; f.r_ok = v[19]; f.r2_ok = v[20];
  f.dx_ok = v[21]; f.rows_on = v[22]; f.stage256_on = v[23]; f.ws_bytes = v[24];
  return f;
}
int main() {
  static const char* const FA[] = {"F256", "FROWS", "FTILED"};
  static const char* const DX[] = {"DXNONE", "DX256", "DXROWS", "DXTILED"};
  static const char* const DW[] = {"DWNONE", "DW256", "DWROWS", "DW64", "DWTILED"};
  static const char* const AF[] = {"RESIDENT", "CHUNKED", "STREAMED"};
  for (int i = 0; i < %(nfwd)d; ++i) {
    const DenseFwdPlan p = adt_dense_fwd_plan(facts_of(DENSE[i]));
    printf("F %%d %%s %%d %%d %%d %%zu %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d\n", i, FA[p.arm], p.grid_x, p.grid_y, p.block, p.lds_bytes, p.chunk, p.epi, p.pc, p.n_panels,
           p.row_groups, p.kb, p.ch, p.bn, p.nt_m, p.nt_n);
  }
  for (int i = %(nfwd)d; i < %(ndense)d; ++i) {
    const DenseFacts f = facts_of(DENSE[i]);
    const DenseBwdPlan p = adt_dense_bwd_plan(f);
    printf("X %%d %%s %%d %%d %%d %%zu %%d %%d %%d %%d %%d %%d ", i, DX[p.dx], p.dx_grid_x, p.dx_grid_y, p.dx_block, p.dx_lds_bytes, p.nb, p.dx_chunk, p.n_pieces, p.pc,
           p.n_panels, (int)p.has_u);
    for (int j = 0; j < p.n_pieces; ++j)
      printf("%%s%%d:%%d:%%d:%%d:%%d:%%zu", j ? "," : "", p.piece[j].n0, p.piece[j].chunk, p.piece[j].beta, p.piece[j].kb, p.piece[j].row_groups, p.piece[j].lds_bytes);
    printf("%%s %%d %%d %%d %%d %%d %%d\n", p.n_pieces ? "" : "-", p.dx_bn, p.gx, p.gy, p.dx_splits, p.n_chunk, (int)p.dx_zero_fill);
    printf("W %%d %%s %%d %%d %%d %%zu %%d %%d %%d %%d %%d %%d %%lld %%d %%d %%d %%d %%d %%d %%d\n", i, DW[p.dw], p.dw_grid_x, p.dw_grid_y, p.dw_block, p.dw_lds_bytes, p.dw_chunk,
           p.nwg, p.blocks, p.kblocks, p.per, p.reduce_groups, (long long)p.ws_used, (int)p.partials, p.dw_splits, p.n_blocks, p.k_blocks, p.dw_bn, p.dw_gx, p.dw_gy);
  }
  for (int i = 0; i < %(nattn)d; ++i) {
    const double* c = ATTN[i];
    const AttnPlan p = adt_attn_masked_plan((int)c[0], (int)c[1], (int)c[2], c[3] != 0, c[4] != 0, c[5] != 0, (float)c[6]);
    if (p.error[0]) printf("A %%d error %%s\n", i, p.error);
    else printf("A %%d %%s %%d %%d %%d %%d %%d %%d %%zu\n", i, AF[p.family], p.maxkt, p.nch, p.kc, p.waves, (int)p.csk, p.grid_y, p.lds_bytes);
  }
  for (int i = 0; i < %(nquery)d; ++i) printf("Q %%d %%lld\n", i, (long long)adt_dense_bwd_ws_need(QUERY[i][0], QUERY[i][1], QUERY[i][2], QUERY[i][3]));
  return 0;
}
"""


def c_double(v):
    return "-INFINITY" if v == -math.inf else repr(float(v))


def main_source():
    dense = ", ".join("{" + ", ".join("%dLL" % f[k] for k in FACT_FIELDS) + "}" for f in FWD + BWD)
    attn = ", ".join("{" + ", ".join(c_double(v) for v in c) + "}" for c in ATTN)
    query = ", ".join("{%d, %d, %d, %d}" % q for q in QUERY)
    return MAIN % dict(nfacts=len(FACT_FIELDS), dense=dense, attn=attn, query=query, nfwd=len(FWD), ndense=len(FWD) + len(BWD), nattn=len(ATTN),
                       nquery=len(QUERY))


def fmt(tag, i, fields):
    return " ".join([tag, str(i)] + [str(int(v)) if isinstance(v, bool) else str(v) for v in fields])


@pytest.fixture(scope="module", params=[[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]], ids=["plain", "asan-ubsan"])
def table(request, tmp_path_factory):
    """The program's output lines by tag: {"F": [...], "X": [...], "W": [...], "A": [...], "Q": [...]}."""
    tmp = tmp_path_factory.mktemp("wide_plan")
    src, exe = tmp / "wide_plan_main.cpp", tmp / "wide_plan_main"
    src.write_text(main_source())
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "adt_amd", "csrc")] +
                          request.param + ["-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60,
                         env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
    lines = {}
    for line in out.stdout.splitlines():
        lines.setdefault(line[0], []).append(line)
    return lines


def test_header_is_plain_cpp():
    """No HIP in the header: nothing from ROCm on the include path of the builds above, and no device word in the text."""
    text = open(os.path.join(REPO, "adt_amd", "csrc", "adt_wide_plan.h")).read()
    for word in ("hip/", "__global__", "__device__", "getenv"):
        assert word not in text, word


def test_dense_fwd_table(table):
    want = [fmt("F", i, expect_fwd(f)) for i, f in enumerate(FWD)]
    assert table["F"] == want, [(a, b) for a, b in zip(table["F"], want) if a != b][:5]
    rows = [line.split() for line in table["F"]]
    assert {r[2] for r in rows} == {"F256", "FROWS", "FTILED"}
    # the rows of the issue's table, as literals
    assert rows[0][2:8] == ["F256", "4", "1", "512", "0", "32"]
    assert rows[1][2:5] == ["F256", "4", "4"] and int(rows[3][3]) <= 128 < int(rows[2][3]) <= 256      # work-group cap 512 / 4 = 128 at N = 1024, 256 at N = 256
    assert [r[8] for r in rows[5:13]] == [str(e) for e in range(8)] and all(r[2] == "F256" for r in rows[5:16])
    assert [r[8] for r in rows[13:16]] == ["1", "1", "4"]      # row mask, second residual, saved pre-activation
    assert [r[2] for r in rows[16:20]] == ["FROWS", "FTILED", "FROWS", "FROWS"]      # ADT_STAGE256 off, rows off, N = 1280, N = 200
    assert rows[20][2:11] == ["FROWS", "1", "1", "512", "59584", "0", "0", "112", "1"]      # below the 64 KB doubling threshold
    assert [r[10] for r in rows[21:24]] == ["2", "2", "2"] and [r[13] for r in rows[21:24]] == ["8", "8", "4"]      # two panels; R2: CH = 4
    assert [(r[2], r[14]) for r in rows[26:31]] == [("FTILED", "64"), ("FTILED", "128"), ("FTILED", "128"), ("FTILED", "64"), ("FTILED", "128")]
    assert all(r[2] == "FTILED" for r in rows[31:35])      # fp32
    assert [r[2] for r in rows[35:42]] == ["FTILED", "FTILED", "FTILED", "FTILED", "FTILED", "F256", "F256"]      # misaligned Y, R, U, bias (rows only); absent ones are not read
    for f, r in zip(FWD, rows):
        v = [int(x) for x in r[3:]]
        assert v[3] <= LDS_MAX
        if r[2] == "F256":
            assert v[4] * v[0] >= f["T"] and v[4] % DWP_TS == 0 and v[1] * 256 == f["N"]
        elif r[2] == "FROWS":
            assert v[6] * v[7] >= f["N"] and v[0] == v[7] * v[8] and v[6] % 16 == 0
        else:
            assert v[12] * GBM >= f["T"] and v[13] * v[11] >= f["N"] and v[0] >= v[12] * v[13]


def test_dense_bwd_dx_table(table):
    want = [fmt("X", len(FWD) + i, expect_dx(f)) for i, f in enumerate(BWD)]
    assert table["X"] == want, [(a, b) for a, b in zip(table["X"], want) if a != b][:5]
    rows = [line.split() for line in table["X"]]
    assert {r[2] for r in rows} == {"DXNONE", "DX256", "DXROWS", "DXTILED"}
    assert [(r[2], r[7]) for r in rows[:4]] == [("DX256", "1"), ("DX256", "2"), ("DX256", "3"), ("DXROWS", "0")]      # N = 256 .. 1024 at K = 256

    def pieces(r):
        return [tuple(int(v) for v in p.split(":")) for p in r[13].split(",")]
    assert [p[:3] for p in pieces(rows[4])] == [(0, 128, 0), (128, 128, 1), (256, 128, 1), (384, 64, 1)]      # N = 448 with an activation
    assert [p[:3] for p in pieces(rows[10])] == [(0, 256, 0), (256, 128, 1), (384, 64, 1)] and pieces(rows[11])[0][2] == 1      # ... without; beta
    assert rows[12][2] == "DXTILED" and rows[12][17] == "1"      # N = 100
    for r, zero in ((rows[13], "1"), (rows[14], "0")):      # (128, 64, 4096): zero-fill iff beta is 0
        assert r[2] == "DXTILED" and int(r[17]) > 1 and int(r[18]) % GBK == 0 and r[19] == zero
    for f, r in zip(BWD, rows):
        assert int(r[6]) <= LDS_MAX
        if r[2] == "DX256":
            assert int(r[8]) * int(r[3]) >= f["T"] and int(r[8]) % DWP_TS == 0
        elif r[2] == "DXROWS":
            ps = pieces(r)
            assert len(ps) == int(r[9]) and ps[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(ps, ps[1:])) and ps[-1][0] + ps[-1][1] == f["N"]
            assert all(p[2] == 1 for p in ps[1:]) and all(p[5] <= LDS_MAX and p[1] == 32 * p[3] for p in ps) and int(r[10]) * int(r[11]) >= f["K"]
        elif r[2] == "DXTILED":
            assert int(r[16]) * GBM >= f["T"] and int(r[3]) >= int(r[15]) * int(r[16]) * int(r[17])
            assert int(r[17]) == 1 or int(r[17]) * int(r[18]) >= f["N"]


def test_dense_bwd_dw_table(table):
    want = [fmt("W", len(FWD) + i, expect_dw(f)) for i, f in enumerate(BWD)]
    assert table["W"] == want, [(a, b) for a, b in zip(table["W"], want) if a != b][:5]
    rows = [line.split() for line in table["W"]]
    assert {r[2] for r in rows} == {"DWNONE", "DW256", "DWROWS", "DW64", "DWTILED"}
    by = {(f["N"], f["K"], f["T"], f["ws_bytes"]): r for f, r in zip(BWD, rows) if f["has_dw"] and not f["has_dx"] and f["rows_on"] and f["prec"] == BF16 and f["x_ok"]
          and not f["has_act"]}
    for (N, K) in DW_WS:
        for T in (1000, 4100, 51200):
            r = by[(N, K, T, WS)]
            assert r[2] == "DW256" and (r[11] == "32") == (int(r[8]) >= 128), r      # per is 32 iff nwg >= 128
            assert by[(N, K, T, 0)][2] == ("DWROWS" if ceil(N, 256) * ceil(K, 128) >= 4 else "DWTILED")
    for (N, K) in ((64, 64), (128, 128)):
        assert by[(N, K, 51200, WS)][2] == "DW64" and by[(N, K, 51200, WS)][14] == "1" and by[(N, K, 51200, 0)][2:] == by[(N, K, 51200, WS)][2:13] + ["0", "0"] + ["0"] * 6
    assert by[(64, 64, 51200, 200 * DW64_PART * 4)][14] == "1" and by[(64, 64, 51200, 200 * DW64_PART * 4 - 1)][14] == "0"      # 200 workgroups x one block
    assert by[(256, 256, 51200, 256 * 262144)][2] == "DW256" and by[(256, 256, 51200, 256 * 262144 - 1)][2] == "DWTILED"
    assert by[(100, 96, 1000, WS)][2] == "DWTILED"
    tiers = {}
    for f, r in zip(BWD, rows):
        v = [int(x) for x in r[3:]]
        assert v[3] <= LDS_MAX and v[10] <= f["ws_bytes"]
        if r[2] in ("DW256", "DW64"):
            assert v[4] * v[0] >= f["T"] and v[4] % (DWP_TS if r[2] == "DW256" else DW64_ROWS) == 0
        elif r[2] == "DWROWS":
            assert v[4] * v[12] >= f["T"] and v[4] % DW_TS == 0 and v[13] * DW_BN >= f["N"] and v[14] * DW_BK >= f["K"] and v[0] >= v[12] * v[13] * v[14]
        elif r[2] == "DWTILED":
            assert v[4] * v[12] >= f["T"] and v[4] % GBK == 0 and v[0] >= v[12] * v[16] * v[17]
            tiers[1 if v[16] * v[17] <= 4 else (2 if v[16] * v[17] <= 12 else 3)] = r
    assert set(tiers) == {1, 2, 3}      # 512, 2048 and 1024 work-groups aimed at


def test_dense_ws_query_matches_the_dw_half(table):
    """adt_dense_bwd_ws_bytes: what the dW half reports for the shape with aligned operands, the rows kernels on and any workspace."""
    got = {q: int(line.split()[2]) for q, line in zip(QUERY, table["Q"])}
    for q in QUERY:
        want = 0 if q[1] <= 0 else expect_dw(facts(q[1], q[2], q[3], prec=q[0], has_dw=1, ws_bytes=1 << 62))[11]
        assert got[q] == want, (q, got[q], want)
    assert got[(BF16, 1000, 256, 256)] == 32 * 262144 and got[(BF16, 51200, 64, 64)] == 200 * DW64_PART * 4
    assert got[(BF16, 1000, 1024, 1024)] == 0 and got[(BF16, 1000, 96, 100)] == 0 and got[(F32, 51200, 64, 64)] == 0 and got[(BF16, 0, 64, 64)] == 0


def test_attn_masked_table(table):
    want = []
    for i, c in enumerate(ATTN):
        e = expect_attn(F32 if c[0] == F32 else BF16, *c[1:])
        want.append("A %d error %s" % (i, e) if isinstance(e, str) else fmt("A", i, e))
    assert table["A"] == want, [(a, b) for a, b in zip(table["A"], want) if a != b][:5]
    got = {c: line.split(None, 2)[2] for c, line in zip(ATTN, table["A"])}
    assert {v.split()[0] for v in got.values()} == {"RESIDENT", "CHUNKED", "STREAMED", "error"}
    assert got[(F32, 64, 200, 1, 0, 0, -1e9)].split()[:3] == ["CHUNKED", "16", "2"]
    assert got[(BF16, 64, 200, 1, 0, 0, -1e9)].split()[:5] == ["RESIDENT", "14", "1", "0", "16"] and got[(BF16, 64, 200, 0, 0, 0, -1e9)].split()[4] == "16"
    for L in (64, 200):
        assert got[(BF16, 128, L, 0, 1, 0, -1e9)].split()[4:6] == ["16", "1"] and got[(BF16, 128, L, 1, 1, 0, -1e9)].split()[0:5:4] == ["CHUNKED", "8"]
        for causal, kid, fill in ((1, 1, -1e9), (0, 0, -1e9), (1, 0, -1e4)):
            assert got[(BF16, 128, L, 0, causal, kid, fill)].split()[0:6:5] == ["RESIDENT", "0"]
        assert got[(BF16, 128, L, 0, 1, 0, -math.inf)].split()[5] == "1"
    assert all(got[(F32, 128, 200, bwd, 1, 0, -1e9)].split()[0] == "STREAMED" for bwd in (0, 1))
    assert got[(F32, 128, 64, 0, 1, 0, -1e9)].split()[:3] == ["RESIDENT", "4", "1"] and got[(F32, 128, 64, 1, 1, 0, -1e9)].split()[:3] == ["CHUNKED", "4", "1"]
    assert got[(BF16, 128, 257, 0, 1, 0, -1e9)] == "error masked attention: L=257 > 256 unsupported at head_dim 128"
    for L in (1, 256):
        assert got[(BF16, 256, L, 0, 1, 0, -1e9)].split()[0:7:6] == ["STREAMED", str(ceil(ceil(L, 16), 4))]
    assert got[(BF16, 256, 0, 0, 1, 0, -1e9)] == "error masked attention: L=0 outside 1..256 at head_dim 256"
    assert got[(F32, 256, 257, 1, 1, 0, -1e9)] == "error masked attention: L=257 outside 1..256 at head_dim 256"
    assert got[(BF16, 48, 50, 0, 0, 0, -1e9)] == "error masked attention: head_dim=48 unsupported (16/32/64/128/256)"
    assert got[(BF16, 64, 225, 0, 0, 0, -1e9)] == "error masked attention: L=225 > 224 unsupported"
    assert all(int(v.split()[7]) <= LDS_MAX for v in got.values() if not v.startswith("error"))
