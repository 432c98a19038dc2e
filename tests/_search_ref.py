"""numpy restatement of the search ops (esm_amd/csrc/search.hip): the per-protein mean and the streaming top-k.  The kernels
reproduce these bit for bit."""
import functools
import math

import numpy as np

F32 = np.float32
NEG_INF = np.float32(-np.inf)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- pooling --------------------------------------------------------------------------------------------------------------
def pool_rows(x, rows, seg_off, E=None):
    """out fp32 [n_seg, E]: per segment the fp64 sum of the listed rows of x [N, >= E] in list order, divided by their count and
    rounded once; an empty segment gives zeros.  Row indices are clamped to [0, N - 1], offsets to [0, seg_off[-1]] and to
    their predecessor; rows None: list entry r is row r."""
    x = np.asarray(x, dtype=F32)
    N = x.shape[0]
    E = x.shape[1] if E is None else E
    seg_off = np.asarray(seg_off, dtype=np.int64)
    total = max(int(seg_off[-1]), 0)
    out = np.zeros((len(seg_off) - 1, E), dtype=F32)
    for s in range(len(seg_off) - 1):
        lo = min(max(int(seg_off[s]), 0), total)
        hi = min(max(int(seg_off[s + 1]), lo), total)
        acc = np.zeros((E,), dtype=np.float64)
        for r in range(lo, hi):
            row = min(max(int(r if rows is None else rows[r]), 0), N - 1)
            acc += x[row, :E].astype(np.float64)  # one addition per row: ascending order
        if hi > lo:
            out[s] = (acc / np.float64(hi - lo)).astype(F32)
    return out


# ---- top-k ----------------------------------------------------------------------------------------------------------------
def order(v):
    """uint32 that ascends with the total order of the IEEE bits: -inf < ... < -0.0 < +0.0 < ... < +inf."""
    b = bits(v)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def topk_merge(row, k, id_base=0, exclude=None, run_val=None, run_id=None):
    """(val fp32 [k], id int32 [k]) of one row: the candidates are (row[j], id_base + j) — NaN values and id == exclude are
    none — and the used slots (id >= 0) of the running list; the k best by value descending in the total order, then id
    ascending; unused slots are (-inf, -1)."""
    row = np.asarray(row, dtype=F32)
    ids = np.arange(len(row), dtype=np.int64) + id_base
    ok = ~np.isnan(row)
    if exclude is not None:
        ok &= ids != exclude
    val, ids = row[ok], ids[ok]
    if run_val is not None:
        used = (np.asarray(run_id) >= 0) & ~np.isnan(np.asarray(run_val, dtype=F32))
        val = np.concatenate([val, np.asarray(run_val, dtype=F32)[used]])
        ids = np.concatenate([ids, np.asarray(run_id, dtype=np.int64)[used]])
    key = (order(val).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - ids.astype(np.uint64))
    best = np.argsort(key, kind="stable")[::-1][:k]
    out_val = np.full((k,), NEG_INF, dtype=F32)
    out_id = np.full((k,), -1, dtype=np.int32)
    out_val[:len(best)] = val[best]
    out_id[:len(best)] = ids[best]
    return out_val, out_id


def topk_rows(S, k, n_cols=None, id_base=0, exclude=None, run_val=None, run_id=None):
    """``topk_merge`` per row of S [R, >= n_cols]: (val [R, k], id [R, k])."""
    S = np.asarray(S, dtype=F32)
    n_cols = S.shape[1] if n_cols is None else n_cols
    got = [topk_merge(S[q, :n_cols], k, id_base, None if exclude is None else int(exclude[q]),
                      None if run_val is None else run_val[q], None if run_id is None else run_id[q]) for q in range(S.shape[0])]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def brute_force_topk(cands, k):
    """The same order without the key: ``cands`` a list of (value, id) Python floats / ints; NaN is dropped; a before b iff
    a's value is greater, or -0.0 meets +0.0 (the positive zero first), or the values are the same and a's id is lower."""
    def before(a, b):
        (va, ia), (vb, ib) = a, b
        if va != vb:
            return -1 if va > vb else 1
        sa, sb = math.copysign(1.0, va), math.copysign(1.0, vb)
        if sa != sb:
            return -1 if sa > sb else 1
        return -1 if ia < ib else (1 if ia > ib else 0)

    kept = sorted([c for c in cands if not math.isnan(c[0])], key=functools.cmp_to_key(before))[:k]
    kept += [(-math.inf, -1)] * (k - len(kept))
    return kept
