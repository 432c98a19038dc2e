"""The two kernels of esm_amd/csrc/search.hip one op at a time, bit for bit against the numpy reference of tests/_search_ref.py:
``esmk_op_pool_rows`` (the per-protein mean) and ``esmk_op_topk_merge`` (one block of the streaming top-k), at the edges of
their tiles — one float4 group, one load of the workgroup (4096 columns), one round (32768 columns) and beyond — and with every
value rule; then planted neighbours through images + GEMM + merge, and every refusal of both entries."""
import ctypes

import numpy as np
import pytest
import torch

import _search_ref as ref
from esm_amd import _native as N
from esm_amd import ops
from esm_amd.search import EmbeddingIndex

pytestmark = pytest.mark.gpu


def same_bits(got, want, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a, b = (ref.bits(got), ref.bits(want)) if got.dtype == np.float32 else (got, want)
    bad = np.argwhere(a != b)
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), [(got[tuple(i)], want[tuple(i)]) for i in bad[:4]])


# ---- pooling --------------------------------------------------------------------------------------------------------------
SEG_LENGTHS = [1, 2, 63, 64, 65, 1025, 0, 3] + [5, 0, 17, 33] * 8  # 40 segments


@pytest.mark.parametrize("wide", [False, True], ids=["ldx=E", "ldx>E"])
@pytest.mark.parametrize("E", [128, 96, 1280])
def test_pool_rows(E, wide):
    rng = np.random.default_rng(E + wide)
    Nr = 700
    ldx = E + 8 if wide else E
    full = (rng.standard_normal((Nr, ldx)) * np.exp(rng.uniform(-6, 6, (Nr, 1)))).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(SEG_LENGTHS)]).astype(np.int32)
    rows = rng.integers(0, Nr, size=off[-1]).astype(np.int32)
    rows[3:6] = rows[3]                       # a repeated row
    rows[10], rows[11], rows[12] = Nr, 2 ** 30, -7  # clamped to N - 1, N - 1 and 0
    x = torch.from_numpy(full).cuda()[:, :E]
    want = ref.pool_rows(full, rows, off, E)
    assert not want[6].any() and not np.isnan(want).any()  # the empty segment: a zero row
    got = ops.pool_rows(x, torch.from_numpy(rows).cuda(), torch.from_numpy(off).cuda())
    same_bits(got, want, "40 segments")
    # the same segment alone, and the list itself as rows (NULL)
    for s in (5, 2, 6):
        alone = ops.pool_rows(x, torch.from_numpy(rows[off[s]:off[s + 1]].copy()).cuda(),
                              torch.tensor([0, SEG_LENGTHS[s]], dtype=torch.int32).cuda())
        same_bits(alone, want[s:s + 1], f"segment {s} alone")
    ident = ops.pool_rows(x, None, torch.tensor([0, 65, 65, 700], dtype=torch.int32).cuda())
    same_bits(ident, ref.pool_rows(full, None, [0, 65, 65, 700], E), "no row list")
    # offsets that lie: clamped to the list's length and to their predecessor
    lying = np.array([-4, 70, 60, 2000, 130], dtype=np.int32)
    same_bits(ops.pool_rows(x, torch.from_numpy(rows).cuda(), torch.from_numpy(lying).cuda()), ref.pool_rows(full, rows, lying, E), "lying offsets")


# ---- top-k ----------------------------------------------------------------------------------------------------------------
N_COLS = [1, 7, 64, 65, 1023, 1024, 1025, 5000, 70000]
KS = [1, 2, 64, 257, 1024]


def value_rows(n, rng):
    """The rows every case stands on, fp32 [R, n]."""
    rows = [rng.integers(0, 4, n).astype(np.float32),                      # ties everywhere: the lowest id wins
            np.full(n, 0.25, dtype=np.float32),                            # all equal
            np.arange(n, dtype=np.float32) / 8,                            # ascending: every column passes the running threshold
            -np.arange(n, dtype=np.float32) / 8,                           # descending
            rng.choice(np.array([0.0, -0.0], dtype=np.float32), n),        # +0.0 before -0.0
            rng.choice(np.array([np.inf, -np.inf, 1.0, -1.0], dtype=np.float32), n),
            rng.standard_normal(n).astype(np.float32),
            np.full(n, np.nan, dtype=np.float32)]                          # no candidate at all
    scattered = rng.standard_normal(n).astype(np.float32)
    scattered[rng.random(n) < 0.3] = np.nan
    rows.append(scattered)
    cos = np.clip(rng.standard_normal(n) * 0.1, -1, 1).astype(np.float32)  # what a search sees
    rows.append(cos)
    return np.stack(rows)


def poisoned(rows, ld):
    """[R, ld] with NaN behind the rows' columns"""
    S = np.full((rows.shape[0], ld), np.nan, dtype=np.float32)
    S[:, :rows.shape[1]] = rows
    return S


@pytest.mark.parametrize("n_cols", N_COLS)
def test_topk_merge_one_block(n_cols):
    rng = np.random.default_rng(n_cols)
    base = value_rows(n_cols, rng)
    R0 = base.shape[0]
    rows = np.concatenate([base] * 4)  # 40 rows: every kind in several workgroups
    ld = (n_cols + 3) // 4 * 4 + 8
    S = torch.from_numpy(poisoned(rows, ld)).cuda()
    id_base = 12345
    inside = (id_base + rng.integers(0, n_cols, len(rows))).astype(np.int32)
    top = np.array([int(np.nanargmax(np.where(np.isnan(r), -np.inf, r))) if not np.isnan(r).all() else 0 for r in rows])
    inside[:R0] = id_base + top[:R0]          # the best column itself is excluded
    outside = np.where(np.arange(len(rows)) % 2 == 0, -1, id_base + n_cols).astype(np.int32)
    # the reference once per exclude list at the largest k: the k best are the first k of the 1024 best
    full = {what: ref.topk_rows(rows, max(KS), n_cols, id_base, ex) for what, ex in (("no exclude", None), ("inside", inside), ("outside", outside))}
    for k in KS:
        for what, ex in (("no exclude", None), ("inside", inside), ("outside", outside)):
            want_val, want_id = full[what][0][:, :k].copy(), full[what][1][:, :k].copy()
            val, ids = ops.topk_merge(S, k, n_cols=n_cols, id_base=id_base, exclude=None if ex is None else torch.from_numpy(ex).cuda())
            same_bits(ids, want_id, (n_cols, k, what, "ids"))
            same_bits(val, want_val, (n_cols, k, what, "values"))
            if what == "outside":
                assert np.array_equal(want_id, full["no exclude"][1][:, :k])
        if k > n_cols:
            assert (want_id[0, n_cols:] == -1).all() and np.isneginf(want_val[0, n_cols:]).all()
        # a row alone gives what it gives inside the 40
        full_val, full_id = ops.topk_merge(S, k, n_cols=n_cols, id_base=id_base)
        for q in (2, 8, 17):
            one_val, one_id = ops.topk_merge(S[q:q + 1], k, n_cols=n_cols, id_base=id_base)
            assert torch.equal(one_id, full_id[q:q + 1]) and torch.equal(one_val.view(torch.int32), full_val[q:q + 1].view(torch.int32))


@pytest.mark.parametrize("k", [1, 2, 64, 257, 1024])
def test_topk_merge_streams(k):
    """Blocks of 300 + 1 + 700 + 4000 columns through the running lists equal the one-shot result; ``first`` ignores what the
    lists held."""
    rng = np.random.default_rng(k)
    n = 5001
    rows = value_rows(n, rng)
    R = rows.shape[0]
    want_val, want_id = ref.topk_rows(rows, k)
    S = torch.from_numpy(poisoned(rows, n + 7)).cuda()
    shot_val, shot_id = ops.topk_merge(S, k, n_cols=n)
    same_bits(shot_id, want_id, "one shot ids")
    same_bits(shot_val, want_val, "one shot values")
    val = torch.from_numpy(rng.choice(np.array([np.nan, np.inf, 7.0], dtype=np.float32), (R, k))).cuda()  # garbage
    ids = torch.from_numpy(rng.integers(-5, 10 ** 6, (R, k)).astype(np.int32)).cuda()
    exclude = torch.from_numpy(want_id[:, 0].copy()).cuda()
    ex_val, ex_id = val.clone(), ids.clone()
    lo = 0
    for width in (300, 1, 700, 4000):
        ld = (width + 3) // 4 * 4 + 4
        block = torch.from_numpy(poisoned(rows[:, lo:lo + width], ld)).cuda()
        ops.topk_merge(block, k, val, ids, n_cols=width, id_base=lo, first=lo == 0)
        ops.topk_merge(block, k, ex_val, ex_id, n_cols=width, id_base=lo, exclude=exclude, first=lo == 0)
        if lo == 0:  # after the first block the lists are that block's result alone
            v0, i0 = ref.topk_rows(rows[:, :300], k)
            same_bits(ids, i0, "first block ids")
            same_bits(val, v0, "first block values")
        lo += width
    same_bits(ids, want_id, "streamed ids")
    same_bits(val, want_val, "streamed values")
    ex_want_val, ex_want_id = ref.topk_rows(rows, k, exclude=want_id[:, 0])
    same_bits(ex_id, ex_want_id, "streamed ids with exclude")
    same_bits(ex_val, ex_want_val, "streamed values with exclude")


def test_planted_neighbours():
    """2000 random unit vectors at E = 128 with exact copies of 5 of them, through images + GEMM + merge: a query's copy and
    itself are bit-equal similarities at ranks 0 - 1, the lower id first; with ``exclude_self`` the copy is rank 0."""
    rng = np.random.default_rng(7)
    n, E = 2000, 128
    v = rng.standard_normal((n, E)).astype(np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    src = np.array([0, 7, 640, 999, 1500])
    dst = np.array([1999, 300, 641, 12, 1501])
    v[dst] = v[src]
    index = EmbeddingIndex(v, [str(i) for i in range(n)], np.ones(n)).to("cuda")
    assert index.image.shape == (2048, 3 * E) and index.image.dtype == torch.float16 and not index.image[n:].any()
    out = index.search(torch.from_numpy(v[src]).cuda(), 10)
    ids, scores = out["ids"].cpu().numpy(), out["scores"].cpu().numpy()
    for q in range(5):
        assert sorted(ids[q, :2].tolist()) == sorted([src[q], dst[q]]) and ids[q, 0] < ids[q, 1], (q, ids[q])
        assert ref.bits(scores[q, :1]) == ref.bits(scores[q, 1:2]) and abs(scores[q, 0] - 1) < 1e-5 and scores[q, 2] < 0.6
    # the index against itself: every vector finds itself first (or its copy, when that has the lower id) ...
    own = index.search(index, 3, return_similarity=True)
    first = own["ids"][:, 0].cpu().numpy()
    partner = np.arange(n)
    partner[src], partner[dst] = dst, src
    assert np.array_equal(first, np.minimum(np.arange(n), partner))
    want_val, want_id = ref.topk_rows(own["similarity"].cpu().numpy(), 3)
    same_bits(own["ids"], want_id, "self search ids")
    same_bits(own["scores"], want_val, "self search values")
    # ... and with exclude_self the copy is rank 0
    ex = index.search(index, 3, exclude_self=True)
    ex_ids = ex["ids"].cpu().numpy()
    assert np.array_equal(ex_ids[src, 0], dst) and np.array_equal(ex_ids[dst, 0], src)
    assert not (ex_ids == np.arange(n)[:, None]).any()
    want_val, want_id = ref.topk_rows(own["similarity"].cpu().numpy(), 3, exclude=np.arange(n))
    same_bits(ex["ids"], want_id, "exclude_self ids")
    same_bits(ex["scores"], want_val, "exclude_self values")


# ---- refusals -------------------------------------------------------------------------------------------------------------
def refused(rc, *words):
    assert rc != 0
    msg = N.lib.esmk_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)


def test_refusals():
    S = torch.zeros((4, 16), dtype=torch.float32, device="cuda")
    val = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    ids = torch.zeros((4, 8), dtype=torch.int32, device="cuda")
    st = N.cur_stream()
    null = ctypes.c_void_p(0)
    name = "esmk_op_topk_merge"

    def topk(S_=N.ptr(S), ld=16, n_rows=4, n_cols=16, id_base=0, k=8, val_=N.ptr(val), ids_=N.ptr(ids)):
        return N.lib.esmk_op_topk_merge(S_, ld, n_rows, n_cols, id_base, null, k, val_, ids_, 1, st)

    assert topk() == 0 and topk(n_rows=0) == 0
    refused(topk(S_=null), name, "null")
    refused(topk(val_=null), name, "null")
    refused(topk(ids_=null), name, "null")
    refused(topk(k=0), name, "k must be 1 .. 1024")
    refused(topk(k=1025), name, "k must be 1 .. 1024")
    refused(topk(n_cols=0), name, "n_cols must be 1 .. 2^22")
    refused(topk(n_cols=(1 << 22) + 1, ld=(1 << 22) + 4), name, "n_cols must be 1 .. 2^22")
    refused(topk(ld=12), name, "ldS")
    refused(topk(ld=18, n_cols=16), name, "ldS")
    refused(topk(id_base=-1), name, "id_base")
    refused(topk(id_base=2 ** 31 - 16), name, "id_base")
    assert topk(id_base=2 ** 31 - 17) == 0
    refused(topk(n_rows=-1), name, "n_rows")
    refused(topk(S_=ctypes.c_void_p(S.data_ptr() + 4)), name, "aligned")
    torch.cuda.synchronize()

    x = torch.zeros((8, 16), dtype=torch.float32, device="cuda")
    off = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
    out = torch.zeros((1, 16), dtype=torch.float32, device="cuda")
    name = "esmk_op_pool_rows"

    def pool(x_=N.ptr(x), ldx=16, Nr=8, off_=N.ptr(off), n_seg=1, out_=N.ptr(out), E=16):
        return N.lib.esmk_op_pool_rows(x_, ldx, Nr, null, off_, n_seg, out_, E, st)

    assert pool() == 0 and pool(n_seg=0) == 0
    refused(pool(x_=null), name, "null")
    refused(pool(off_=null), name, "null")
    refused(pool(out_=null), name, "null")
    refused(pool(E=0), name, "E must be")
    refused(pool(E=6), name, "E must be")
    refused(pool(Nr=0), name, "N")
    refused(pool(n_seg=-1), name, "n_seg")
    refused(pool(ldx=12), name, "ldx")
    refused(pool(ldx=18), name, "ldx")
    refused(pool(x_=ctypes.c_void_p(x.data_ptr() + 4)), name, "aligned")
    refused(pool(out_=ctypes.c_void_p(out.data_ptr() + 8)), name, "aligned")
    torch.cuda.synchronize()
