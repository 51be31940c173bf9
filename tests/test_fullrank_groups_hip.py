"""GPU: the group-aware full-catalogue ranking (adt_full_rank_groups, adt_amd/csrc/adt_fullrank.cuh) against P separate adt_full_rank
calls on the sliced, int32 re-based CSR -- bit for bit --, its split invariance, strided rows and refusals, and the additive statistics
kernel (adt_full_rank_stats, adt_amd/csrc/adt_fullstats.cuh) against numpy.  DESIGN.md section 31.

The resident CSR has 40 rows.  Rows 0..5 and 7..12 carry the edges, so that every (row0, R) window of the sweep meets them: an empty
row, a row that lists its own target, a row with id 0, ids above n_items and a duplicate, a row that lists the whole catalogue
(n_elig == 0 and rank == 0 whatever the scores), a row without a target, and a row whose target's table row exists twice (an exact
tie that is not counted)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from adt_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_TOTAL = 40
SRC, DST = 5, 9             # table row DST is a copy of row SRC
EDGE = {0: "empty", 1: "own", 2: "odd", 3: "all", 4: "none", 5: "tie"}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def resident(V):
    """(target int32 (40,), seen_off int64 (41,), seen_items int32) on the host."""
    r = np.random.RandomState(V)
    target = r.randint(1, V + 1, N_TOTAL).astype(np.int32)
    rows = []
    for u in range(N_TOTAL):
        kind = EDGE.get(u if u < 7 else u - 7) if u < 13 else None
        ids = list(r.randint(1, V + 1, r.randint(1, 40)))
        if kind == "empty":
            ids = []
        elif kind == "own":
            ids = [int(target[u])] + ids
        elif kind == "odd":
            ids = [0, V + 1, V + 7, 3, 3] + ids + [0]
        elif kind == "all":
            ids = list(range(0, V + 1))
        elif kind == "none":
            target[u] = 0
        elif kind == "tie":
            target[u] = SRC
            ids = [i for i in ids if i not in (SRC, DST)]
        rows.append(ids)
    off = np.zeros(N_TOTAL + 1, np.int64)
    np.cumsum([len(x) for x in rows], out=off[1:])
    return target, off, np.asarray([i for x in rows for i in x], np.int32)


@functools.lru_cache(maxsize=None)
def operands(V, d, n_rows):
    g = torch.Generator().manual_seed(1000 * V + 10 * d + n_rows)
    F = torch.randn(n_rows, d, generator=g)
    E = torch.randn(V + 1, d, generator=g)
    bias = torch.randn(V + 1, generator=g)
    E[DST] = E[SRC]
    bias[DST] = bias[SRC]
    return F.to(DEV), E.to(DEV), bias.to(DEV)


def separate_calls(F, ldf, E, bias, V, R, P, row0, k, first_id, splits=0):
    """P ops.full_rank calls on the P row blocks with the sliced CSR, its offsets re-based to int32: the reference of the issue."""
    target, off, items = resident(V)
    ip = (off[row0:row0 + R + 1] - off[row0]).astype(np.int32)
    ix = items[off[row0]:off[row0 + R]]
    tgt, ip, ix = dev(target[row0:row0 + R]), dev(ip), dev(ix)
    outs = [ops.full_rank(F[p * R:(p + 1) * R], ldf, E, V, tgt, bias, ip, ix, k, splits, first_id) for p in range(P)]
    return [torch.cat([o[i] for o in outs]) if outs[0][i] is not None else None for i in range(4)]


def grouped(F, ldf, E, bias, V, R, P, row0, k, first_id, splits=0):
    target, off, items = resident(V)
    return ops.full_rank_groups(F, ldf, E, V, dev(target), dev(off), dev(items), P * R, R, row0=row0, bias=bias, k=k, splits=splits, first_id=first_id)


def assert_same(got, want, what):
    for name, a, b in zip(("rank", "n_elig", "top_idx", "top_val"), got, want):
        assert (a is None) == (b is None), (what, name)
        if a is not None:      # bit for bit: the float scores compare as their int32 images
            a, b = (x.view(torch.int32) if x.dtype == torch.float32 else x for x in (a, b))
            assert torch.equal(a, b), (what, name)


# ---- 1. groups equal separate calls -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,d", [(120, 64), (120, 52), (4200, 64), (4200, 52)])
@pytest.mark.parametrize("R,P", [(R, P) for R in (5, 16, 17, 33) for P in (1, 3)])
def test_groups_equal_separate_calls(V, d, R, P):
    F, E, bias = operands(V, d, P * R)
    target, off, items = resident(V)
    for row0 in (0, 7):
        for k in (0, 10):
            for first_id in (0, 1):
                got = grouped(F, d, E, bias, V, R, P, row0, k, first_id)
                assert_same(got, separate_calls(F, d, E, bias, V, R, P, row0, k, first_id), (row0, k, first_id))
                rank, nel = got[0].cpu().numpy().reshape(P, R), got[1].cpu().numpy().reshape(P, R)
                u = 3               # rows 3 / 10 of the CSR: the seen list is the whole catalogue
                assert (nel[:, u] == 0).all() and (rank[:, u] == 0).all()
                none = target[row0:row0 + R] == 0      # rows 4 / 11: no target, rank -1
                assert none[4] and ((rank == -1) == none[None]).all()
                if k:                                                     # nothing eligible but the target: the list is the target, then the tail
                    top = got[2].cpu().numpy().reshape(P, R, k)
                    assert (top[:, u, 0] == target[row0 + u]).all() and (top[:, u, 1:] == -1).all()
    if P == 1:      # one group from row 0 is adt_full_rank_from itself, on the int64 offsets
        assert_same(grouped(F, d, E, bias, V, R, 1, 0, 10, 1),
                    ops.full_rank(F, d, E, V, dev(target[:R]), bias, dev(off[:R + 1].astype(np.int32)), dev(items[:off[R]]), 10), "P=1")


def test_the_planted_tie_is_not_counted():
    """Row 5's target is item SRC and item DST has the same table row and bias: DST scores exactly alike and is unseen, so it is eligible,
    counted in n_elig and NOT in the rank.  Checked against float64 scores with DST taken out."""
    V, d, R, P = 120, 64, 17, 3
    F, E, bias = operands(V, d, P * R)
    target, off, items = resident(V)
    rank, nel, _, _ = grouped(F, d, E, bias, V, R, P, 0, 0, 1)
    S = F.double().cpu().numpy() @ E.double().cpu().numpy().T + bias.double().cpu().numpy()
    seen = set(items[off[5]:off[6]].tolist())
    assert DST not in seen and SRC not in seen
    for p in range(P):
        s = S[p * R + 5]
        others = [j for j in range(1, V + 1) if j not in seen and j not in (SRC, DST)]
        gaps = np.abs(s[others] - s[SRC])
        assert gaps.min() > 1e-3                       # no near tie among the rest: float64 decides them as fp32 does
        assert int(rank[p * R + 5]) == int((s[others] > s[SRC]).sum())
        assert int(nel[p * R + 5]) == len(others) + 1


# ---- 2. split invariance ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [120, 4200])
def test_split_invariance(V):
    d, R, P, row0 = 64, 17, 3, 7                       # tiles straddle both group boundaries
    F, E, bias = operands(V, d, P * R)
    base = grouped(F, d, E, bias, V, R, P, row0, 10, 1, splits=0)
    for splits in (2, 7):
        assert_same(grouped(F, d, E, bias, V, R, P, row0, 10, 1, splits=splits), base, splits)


# ---- 3. strided rows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 52])
def test_strided_rows_equal_contiguous_rows(d):
    V, R, P, L = 120, 17, 3, 6
    F, E, bias = operands(V, d, P * R)
    buf = torch.full((P * R * L, d), float("nan"), device=DEV)
    buf[L - 1::L] = F                                  # the last position of every sequence; NaN everywhere else
    got = grouped(buf[L - 1:], L * d, E, bias, V, R, P, 7, 10, 1)
    assert_same(got, grouped(F, d, E, bias, V, R, P, 7, 10, 1), d)
    assert not torch.isnan(got[3][got[2] >= 0]).any()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def raw_groups(F, ldf, E, V, target, off, items, n_rows, R, n_total, row0, k=0, splits=0, first_id=1, rank=True):
    """The C entry point itself, with every argument as given."""
    lib = _lib.load()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    ws = torch.zeros(1 << 20, device=DEV, dtype=torch.uint8)
    out_r = torch.full((max(n_rows, 1),), -7, device=DEV, dtype=torch.int32)
    out_n = torch.full((max(n_rows, 1),), -7, device=DEV, dtype=torch.int32)
    ti = torch.zeros(max(n_rows, 1) * max(k, 1), device=DEV, dtype=torch.int32)
    tv = torch.zeros(max(n_rows, 1) * max(k, 1), device=DEV, dtype=torch.float32)
    rc = lib.adt_full_rank_groups(p(F), ldf, p(E), E.stride(0), None, n_rows, R, E.shape[1], V, first_id, p(target), p(off), p(items), n_total, row0, k,
                                  splits, p(ws), ws.numel(), p(out_r) if rank else None, p(out_n), p(ti), p(tv), None)
    torch.cuda.synchronize()
    assert (out_r == -7).all() and (out_n == -7).all()      # refused before any launch: nothing was written
    return rc, lib.adt_last_error().decode()


def test_refusals():
    V, d, R = 120, 64, 5
    F, E, bias = operands(V, d, 3 * R)
    target, off, items = (dev(x) for x in resident(V))
    ok = dict(F=F, ldf=d, E=E, V=V, target=target, off=off, items=items, n_rows=3 * R, R=R, n_total=N_TOTAL, row0=0)
    E50 = torch.zeros(V + 1, 50, device=DEV)
    bad = [(dict(R=0), "rows_per_group"), (dict(R=-1), "rows_per_group"), (dict(n_rows=3 * R + 1), "multiple"), (dict(row0=-1), "outside"),
           (dict(row0=N_TOTAL - R + 1), "outside"), (dict(n_total=R - 1), "outside"), (dict(off=None), "go together"),
           (dict(items=None), "go together"),
           # everything adt_full_rank_from refuses
           (dict(first_id=2), "first_id"), (dict(k=129), "K="), (dict(k=-1), "K="), (dict(E=E50, ldf=52), "multiple of 4"), (dict(ldf=60), "ldf"),
           (dict(V=0), "n_items"), (dict(ldf=66), "aligned"), (dict(F=F.view(-1)[1:]), "aligned"), (dict(splits=1025), "splits"),
           (dict(splits=-1), "splits"), (dict(rank=False), "missing output")]
    for change, word in bad:
        rc, msg = raw_groups(**dict(ok, **change))
        assert rc != 0 and word in msg and msg.startswith("full_rank_groups:"), (change, msg)
    rc, _ = raw_groups(**dict(ok, n_rows=0))                 # no rows: nothing to do, and no error
    assert rc == 0
    # the Python entry point raises for the same calls
    t, o, i = target, off, items
    for args, kw in (((F, d, E, V, t, o, i, 3 * R, 0), {}), ((F, d, E, V, t, o, i, 3 * R + 1, R), {}), ((F, d, E, V, t, o, i, 3 * R, R), dict(row0=-1)),
                     ((F, d, E, V, t, o, i, 3 * R, R), dict(row0=N_TOTAL - R + 1)), ((F, d, E, V, t, None, i, 3 * R, R), {}),
                     ((F, d, E, V, t, o, i, 3 * R, R), dict(k=129)), ((F, d, E, V, t, o, i, 3 * R, R), dict(first_id=2)),
                     ((F, d, E, V, t, o, i, 3 * R, R), dict(splits=1025)), ((F, d, E, V, t.long(), o, i, 3 * R, R), {}),
                     ((F, d, E, V, t, o.int(), i, 3 * R, R), {}), ((F, d, E, V, t, o, i, 3 * R, R), dict(bias=bias[:V]))):
        with pytest.raises(_lib.AdtError):
            ops.full_rank_groups(*args, **kw)
    with pytest.raises(_lib.AdtError, match="rank and n_elig"):
        ops.full_rank_stats(t.long(), t, 1, 10)
    z = torch.zeros(10, device=DEV, dtype=torch.int32)
    for kw in (dict(rows_per_group=0, kh=10), dict(rows_per_group=3, kh=10), dict(rows_per_group=5, kh=0), dict(rows_per_group=5, kh=1025),
               dict(rows_per_group=5, kh=10, hist=torch.zeros(2, 10, device=DEV, dtype=torch.int64)),
               dict(rows_per_group=5, kh=10, auc=torch.zeros(2, device=DEV, dtype=torch.float32))):
        with pytest.raises(_lib.AdtError):
            ops.full_rank_stats(z, z, **kw)
    lib = _lib.load()
    h, a = torch.zeros(2, 11, device=DEV, dtype=torch.int64), torch.zeros(2, device=DEV, dtype=torch.float64)
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    for rk, ne, n, rpg, kh, hh, aa in ((None, z, 10, 5, 10, h, a), (z, None, 10, 5, 10, h, a), (z, z, 10, 5, 10, None, a), (z, z, 10, 5, 10, h, None),
                                       (z, z, 10, 0, 10, h, a), (z, z, 10, 3, 10, h, a), (z, z, 10, 5, 0, h, a), (z, z, 10, 5, 1025, h, a)):
        assert lib.adt_full_rank_stats(p(rk), p(ne), n, rpg, kh, p(hh), p(aa), None) != 0
        assert lib.adt_last_error().decode().startswith("full_rank_stats:")
    torch.cuda.synchronize()
    assert int(h.sum()) == 0 and float(a.sum()) == 0.0


# ---- 5. adt_full_rank_stats against numpy -----------------------------------------------------------------------------------------------
def np_stats(rank, nel, groups, kh):
    rank, nel = rank.reshape(groups, -1).astype(np.int64), nel.reshape(groups, -1).astype(np.int64)
    hist = np.zeros((groups, kh + 1), np.int64)
    auc = np.zeros(groups, np.float64)
    for g in range(groups):
        ok = rank[g] >= 0
        hist[g] = np.bincount(np.minimum(rank[g][ok], kh), minlength=kh + 1)
        auc[g] = ((nel[g][ok] - rank[g][ok]) / np.maximum(nel[g][ok], 1)).sum()      # the term of sasrec.utils.full_rank_stats
    return hist, auc


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("rpg", [1, 21, 5500])
@pytest.mark.parametrize("kh", [1, 10, 128])
def test_full_rank_stats_equals_numpy(groups, rpg, kh):
    r = np.random.RandomState(100 * groups + rpg + kh)
    N = groups * rpg
    rank = np.where(r.rand(N) < 0.5, r.randint(0, 12, N), r.randint(0, 5001, N)).astype(np.int32)      # half below the usual k, half up to 5000
    nel = (rank + r.randint(0, 3000, N)).astype(np.int32)
    if N > 1:
        rank[r.rand(N) < 0.1] = -1                     # rows without a target count nowhere
        zero = r.rand(N) < 0.1                         # nothing eligible: rank 0, the term is 0 / 1
        rank[zero & (rank >= 0)] = 0
        nel[zero] = 0
    rk, ne = dev(rank), dev(nel)
    want_h, want_a = np_stats(rank, nel, groups, kh)
    hist, auc = ops.full_rank_stats(rk, ne, rpg, kh)
    assert hist.shape == (groups, kh + 1) and hist.dtype == torch.int64 and auc.shape == (groups,) and auc.dtype == torch.float64
    assert np.array_equal(hist.cpu().numpy(), want_h)
    got_a = auc.cpu().numpy()
    print(got_a, want_a)
    assert (np.abs(got_a - want_a) <= rpg * 2.0 ** -52 * np.abs(want_a)).all()
    again = ops.full_rank_stats(rk, ne, rpg, kh)       # a fixed order of addition: the same bits
    assert torch.equal(again[0], hist) and torch.equal(again[1].view(torch.int64), auc.view(torch.int64))
    h2, a2 = ops.full_rank_stats(rk, ne, rpg, kh, hist=hist, auc=auc)      # a second call into the same tensors adds
    assert h2 is hist and a2 is auc
    assert np.array_equal(hist.cpu().numpy(), 2 * want_h) and np.array_equal(auc.cpu().numpy(), 2 * got_a)


@pytest.mark.parametrize("groups,rpg", [(1, 21), (3, 5500)])
def test_full_rank_stats_keeps_the_overflow_bin_empty(groups, rpg):
    """kh = 128 and every rank below 128: the whole row is np.bincount of the ranks and the overflow column is 0."""
    r = np.random.RandomState(rpg)
    N = groups * rpg
    rank = r.randint(0, 128, N).astype(np.int32)
    nel = (rank + r.randint(0, 50, N)).astype(np.int32)
    hist, _ = ops.full_rank_stats(dev(rank), dev(nel), rpg, 128)
    hist = hist.cpu().numpy()
    assert (hist[:, 128] == 0).all()
    for g in range(groups):
        assert np.array_equal(hist[g], np.bincount(rank[g * rpg:(g + 1) * rpg], minlength=129))
