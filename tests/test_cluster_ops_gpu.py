"""The kernels of esm_amd/csrc/cluster.hip one op at a time, exactly against the numpy reference of tests/_cluster_ref.py:
``esmk_op_range_rows`` (count and fill pass of the thresholded row scan) at the edges of its tiles — one float4 group, one
wavefront, one load of the workgroup (1024 columns), one round (8192 columns) and beyond — with every value rule, streamed in
blocks and with offsets that lie; the round kernels and the assignment on hand-made graphs; every refusal of the four entries."""
import ctypes

import numpy as np
import pytest
import torch

import _cluster_ref as cref
import _search_ref as ref
from esm_amd import _native as N
from esm_amd import cluster as C
from esm_amd import ops

pytestmark = pytest.mark.gpu


def same_bits(got, want, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a, b = (ref.bits(got), ref.bits(want)) if got.dtype == np.float32 else (got, want)
    bad = np.argwhere(a != b)
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), [(got[tuple(i)], want[tuple(i)]) for i in bad[:4]])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- range_rows -----------------------------------------------------------------------------------------------------------
N_COLS = [1, 7, 64, 65, 1023, 1024, 1025, 5000, 70000]
SENTINEL_ID, SENTINEL_SCORE = -77, np.float32(-123.0)


def value_rows(n, rng, thr):
    """The rows every case stands on, fp32 [R, n], around the threshold ``thr``."""
    t = np.float32(thr)
    just_below = np.nextafter(t, np.float32(-np.inf), dtype=np.float32)
    rows = [np.full(n, t - 1, dtype=np.float32),                               # all below
            np.full(n, t + 1, dtype=np.float32),                               # all above: every column is written
            np.full(n, t, dtype=np.float32),                                   # exactly at the threshold: a tie passes
            rng.choice(np.array([t, just_below], dtype=np.float32), n),        # at it or one ulp below
            rng.choice(np.array([0.0, -0.0], dtype=np.float32), n),            # with thr = 0 both pass
            rng.choice(np.array([np.inf, -np.inf, 1.0, -1.0], dtype=np.float32), n),
            (t + rng.standard_normal(n)).astype(np.float32)]                   # half pass
    scattered = (t + rng.standard_normal(n)).astype(np.float32)
    scattered[rng.random(n) < 0.3] = np.nan                                    # NaN never passes
    rows.append(scattered)
    rows.append(np.full(n, np.nan, dtype=np.float32))
    sparse = np.clip(rng.standard_normal(n) * 0.1, -1, 1).astype(np.float32)   # what a search sees: a few neighbours
    sparse[rng.random(n) < 30.0 / max(n, 30)] = t + np.float32(0.25)
    rows.append(sparse)
    return np.stack(rows)


def poisoned(rows, ld, what=np.nan):
    """[R, ld] with NaN (or ``what``) behind the rows' columns"""
    S = np.full((rows.shape[0], ld), what, dtype=np.float32)
    S[:, :rows.shape[1]] = rows
    return S


def two_passes(S, thr, n_cols, id_base=0, exclude=None):
    """count pass, cumulative sum, fill pass on a device S: (counts, offsets, ids, scores, cursor) as numpy arrays"""
    R = S.shape[0]
    counts = torch.zeros((R,), dtype=torch.int64, device="cuda")
    ops.range_rows(S, thr, counts=counts, n_cols=n_cols, id_base=id_base, exclude=exclude)
    offsets = torch.zeros((R + 1,), dtype=torch.int64, device="cuda")
    offsets[1:] = counts.cumsum(0)
    total = int(offsets[-1])
    ids = torch.full((total + 5,), SENTINEL_ID, dtype=torch.int32, device="cuda")  # (five slots nobody owns)
    scores = torch.full((total + 5,), float(SENTINEL_SCORE), dtype=torch.float32, device="cuda")
    cursor = offsets[:-1].clone()
    ops.range_rows(S, thr, offsets=offsets, cursor=cursor, ids=ids, scores=scores, n_cols=n_cols, id_base=id_base, exclude=exclude)
    assert (ids[total:] == SENTINEL_ID).all() and (scores[total:] == float(SENTINEL_SCORE)).all()
    return counts.cpu().numpy(), offsets.cpu().numpy(), ids[:total].cpu().numpy(), scores[:total].cpu().numpy(), cursor.cpu().numpy()


@pytest.mark.parametrize("n_cols", N_COLS)
def test_range_rows_one_block(n_cols):
    rng = np.random.default_rng(n_cols)
    id_base = 12345
    for thr in (0.5, 0.0):
        base = value_rows(n_cols, rng, thr)
        rows = np.concatenate([base] * 4)  # 40 rows: every kind in several workgroups
        R = len(rows)
        ld = (n_cols + 3) // 4 * 4 + 8
        S = dev(poisoned(rows, ld))
        inside = (id_base + rng.integers(0, n_cols, R)).astype(np.int32)
        outside = np.where(np.arange(R) % 2 == 0, -1, id_base + n_cols).astype(np.int32)
        for what, ex in (("no exclude", None), ("inside", inside), ("outside", outside)):
            want_counts, want_ids, want_scores = cref.range_rows(rows, thr, n_cols, id_base, ex)
            counts, offsets, ids, scores, cursor = two_passes(S, thr, n_cols, id_base, None if ex is None else dev(ex))
            same_bits(counts, want_counts, (n_cols, thr, what, "counts"))
            same_bits(ids, want_ids, (n_cols, thr, what, "ids"))
            same_bits(scores, want_scores, (n_cols, thr, what, "scores"))
            same_bits(cursor, offsets[1:], (n_cols, thr, what, "cursor"))
        assert want_counts[0] == 0 and want_counts[1] == n_cols and want_counts[2] == n_cols and want_counts[8] == 0
        if thr == 0.0:
            assert want_counts[4] == n_cols  # -0.0 >= +0.0
        # a row alone gives what it gives among the 40; +inf behind n_cols never passes either
        want_counts, want_ids, want_scores = cref.range_rows(rows, thr, n_cols, id_base)
        off = np.concatenate([[0], np.cumsum(want_counts)])
        S_inf = dev(poisoned(rows, ld, np.inf))
        for q in (1, 6, 17, 29):
            for src in (S, S_inf):
                counts, _, ids, scores, _ = two_passes(src[q:q + 1], thr, n_cols, id_base)
                assert counts.tolist() == [want_counts[q]]
                same_bits(ids, want_ids[off[q]:off[q + 1]], (n_cols, thr, q, "alone ids"))
                same_bits(scores, want_scores[off[q]:off[q + 1]], (n_cols, thr, q, "alone scores"))
    # thresholds at the ends of the line
    for thr, passing in ((-np.inf, ~np.isnan(rows)), (np.inf, rows == np.inf), (np.nan, np.zeros_like(rows, dtype=bool))):
        counts, _, ids, _, _ = two_passes(S, thr, n_cols, id_base)
        assert np.array_equal(counts, passing.sum(1)), thr
        assert np.array_equal(ids, id_base + np.nonzero(passing)[1]), thr


def test_range_rows_streams():
    """Blocks of 300 + 1 + 700 + 4000 columns through counts and cursors equal the one-shot result: counts, ids, scores, order."""
    rng = np.random.default_rng(5)
    n, thr = 5001, 0.5
    rows = value_rows(n, rng, thr)
    R = rows.shape[0]
    exclude = rng.integers(0, n, R).astype(np.int32)
    for ex in (None, exclude):
        want_counts, want_ids, want_scores = cref.range_rows(rows, thr, exclude=ex)
        ex_dev = None if ex is None else dev(ex)
        shot = two_passes(dev(poisoned(rows, n + 7)), thr, n, 0, ex_dev)
        same_bits(shot[0], want_counts, "one shot counts")
        same_bits(shot[2], want_ids, "one shot ids")
        same_bits(shot[3], want_scores, "one shot scores")
        blocks, lo = [], 0
        for width in (300, 1, 700, 4000):
            blocks.append((lo, width, dev(poisoned(rows[:, lo:lo + width], (width + 3) // 4 * 4 + 4))))
            lo += width
        counts = torch.zeros((R,), dtype=torch.int64, device="cuda")
        for lo, width, block in blocks:
            ops.range_rows(block, thr, counts=counts, n_cols=width, id_base=lo, exclude=ex_dev)
        same_bits(counts, want_counts, "streamed counts")
        offsets = torch.zeros((R + 1,), dtype=torch.int64, device="cuda")
        offsets[1:] = counts.cumsum(0)
        cursor = offsets[:-1].clone()
        ids = torch.full((len(want_ids),), SENTINEL_ID, dtype=torch.int32, device="cuda")
        scores = torch.full((len(want_ids),), float(SENTINEL_SCORE), dtype=torch.float32, device="cuda")
        for k, (lo, width, block) in enumerate(blocks):
            ops.range_rows(block, thr, offsets=offsets, cursor=cursor, ids=ids, scores=scores, n_cols=width, id_base=lo, exclude=ex_dev)
            if k == 0:  # after the first block every cursor stands behind that block's pairs
                same_bits(cursor - offsets[:-1], cref.range_rows(rows[:, :300], thr, exclude=ex)[0], "cursor after the first block")
        same_bits(ids, want_ids, "streamed ids")
        same_bits(scores, want_scores, "streamed scores")
        same_bits(cursor, offsets[1:].cpu().numpy(), "streamed cursor")


def test_range_rows_clamps_offsets():
    """Offsets too small for the rows, and offsets and cursors that lie: the row's first pairs up to its range's end are
    written, nothing outside the ranges, and the call returns."""
    rng = np.random.default_rng(9)
    n, thr = 3000, 0.5
    rows = value_rows(n, rng, thr)
    R = rows.shape[0]
    S = dev(poisoned(rows, n + 8))
    want_counts, want_ids, want_scores = cref.range_rows(rows, thr)
    true_off = np.concatenate([[0], np.cumsum(want_counts)])

    def fill(offsets, cursor, cap):
        ids = torch.full((cap,), SENTINEL_ID, dtype=torch.int32, device="cuda")
        scores = torch.full((cap,), float(SENTINEL_SCORE), dtype=torch.float32, device="cuda")
        cur = dev(np.asarray(cursor, dtype=np.int64))
        ops.range_rows(S, thr, offsets=dev(np.asarray(offsets, dtype=np.int64)), cursor=cur, ids=ids, scores=scores, n_cols=n)
        torch.cuda.synchronize()
        return ids.cpu().numpy(), scores.cpu().numpy(), cur.cpu().numpy()

    def expect(offsets, cursor, cap):
        ids = np.full((cap,), SENTINEL_ID, dtype=np.int32)
        scores = np.full((cap,), SENTINEL_SCORE, dtype=np.float32)
        out_cur = np.zeros((R,), dtype=np.int64)
        for q in range(R):
            lo = min(max(int(offsets[q]), 0), cap)
            end = min(max(int(offsets[q + 1]), lo), cap)
            cur = min(max(int(cursor[q]), lo), end)
            take = min(int(want_counts[q]), end - cur)
            ids[cur:cur + take] = want_ids[true_off[q]:true_off[q] + take]
            scores[cur:cur + take] = want_scores[true_off[q]:true_off[q] + take]
            out_cur[q] = min(cur + int(want_counts[q]), end)
        return ids, scores, out_cur

    half = np.concatenate([[0], np.cumsum(want_counts // 2)])  # every row has room for half of its pairs
    cap = int(half[-1]) + 6
    lying = np.array([-5, 3, 3, 40, 40, 40, 2000, 2000, 2001, 10 ** 12, 2 ** 62])  # clamped into [0, cap] and to the predecessor
    lying_cursor = np.array([-7, 100, 2, 41, 0, 39, 0, 2 ** 40, -1, 2100])
    assert len(lying) == R + 1 and len(lying_cursor) == R and cap > 2001
    for what, offsets, cursor in (("half", half, half[:-1]), ("lying", lying, lying_cursor), ("no room", np.zeros(R + 1), np.zeros(R))):
        got, want = fill(offsets, cursor, cap), expect(offsets, cursor, cap)
        same_bits(got[0], want[0], (what, "ids"))
        same_bits(got[1], want[1], (what, "scores"))
        same_bits(got[2], want[2], (what, "cursor"))
    assert (want[0] == SENTINEL_ID).all()  # "no room": nothing was written


# ---- the rounds and the assignment ------------------------------------------------------------------------------------------
def csr_of_lists(lists, rng=None, palette=(0.5, 0.625, 0.75, -0.0, 0.0)):
    """(offsets int64, ids int32, scores fp32) of per-node out-lists (ascending ids); scores from a small palette: equal ones abound"""
    rng = np.random.default_rng(0) if rng is None else rng
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    ids = np.array([w for x in lists for w in sorted(x)], dtype=np.int32)
    return offsets, ids, rng.choice(np.array(palette, dtype=np.float32), len(ids))


def check_graph(lists, priority, what, rng=None, lanes=(None, 1, 8, 64)):
    offsets, ids, scores = csr_of_lists(lists, rng)
    n = len(lists)
    want_rank = cref.rank_of(priority)
    rank64, order = C.rank_of(dev(np.asarray(priority)))
    same_bits(rank64.to(torch.int32), want_rank, (what, "rank"))
    rank = rank64.to(torch.int32)
    is_rep, want_rounds = cref.rounds_of(offsets, ids, want_rank)
    d_off, d_ids, d_scores = dev(offsets), dev(ids), dev(scores)
    wanted = {assign: cref.greedy(offsets, ids, scores, want_rank, assign) for assign in ("first", "nearest")}
    for ln in lanes:
        state, rounds = C.greedy_rounds(d_off, d_ids, rank, lanes=ln, max_rounds=n + C.ROUNDS_PER_READ)
        assert rounds == want_rounds, (what, ln, rounds, want_rounds)
        state = state.cpu().numpy()
        assert np.array_equal(state != C.COVERED, is_rep) and not (state == C.UNDECIDED).any(), (what, ln)
        for assign in ("first", "nearest"):
            got = C.assign_members(d_off, d_ids, d_scores, rank, order, dev(state), assign, lanes=ln)
            for g, w, name in zip(got, wanted[assign], ("rep_of", "representatives", "sizes")):
                same_bits(g, w, (what, ln, assign, name))
    return want_rounds, wanted["first"]


def test_rounds_on_hand_made_graphs():
    n = 70
    rounds, (rep_of, reps, sizes) = check_graph([[] for _ in range(n)], np.arange(n), "empty graph")
    assert rounds == 1 and reps.tolist() == list(range(n - 1, -1, -1)) and (sizes == 1).all()  # everyone is a representative
    rounds, (rep_of, reps, sizes) = check_graph([[w for w in range(n) if w != u] for u in range(n)], np.ones(n), "clique")
    assert reps.tolist() == [0] and sizes.tolist() == [n] and rounds == 2
    star = [[w for w in range(1, n)]] + [[0] for _ in range(n - 1)]
    rounds, (rep_of, reps, sizes) = check_graph(star, [9] + [1] * (n - 1), "star, the centre first")
    assert reps.tolist() == [0] and rounds == 2
    rounds, (rep_of, reps, sizes) = check_graph(star, [0] + [1] * (n - 1), "star, the centre last")
    assert reps.tolist() == list(range(1, n)) and rep_of[0] == 1 and sizes.tolist() == [2] + [1] * (n - 2) and rounds == 2
    # an asymmetric pair, u -> w without w -> u, in both rank orders
    _, (rep_of, _, _) = check_graph([[1], []], [2, 1], "pair, u first")
    assert rep_of.tolist() == [0, 0]
    _, (rep_of, _, _) = check_graph([[1], []], [1, 2], "pair, w first")
    assert rep_of.tolist() == [0, 1]
    # priority ties go to the lower id
    _, (rep_of, reps, _) = check_graph([[1, 2], [0, 2], [0, 1]], [4, 4, 4], "ties")
    assert reps.tolist() == [0] and rep_of.tolist() == [0, 0, 0]


def test_a_directed_chain_takes_a_round_per_node():
    """300 nodes, u -> u + 1, in rank order: node k is decided in round k, and the result is still the sequential loop's."""
    n = 300
    lists = [[u + 1] for u in range(n - 1)] + [[]]
    rounds, (rep_of, reps, sizes) = check_graph(lists, np.arange(n, 0, -1), "chain", lanes=(None, 64))
    assert rounds == n and reps.tolist() == list(range(0, n, 2)) and (sizes == 2).all()
    # the same chain against the rank order: every node but the last is covered by ... nobody earlier: one round
    rounds, (rep_of, reps, sizes) = check_graph(lists, np.arange(n), "chain, reversed ranks", lanes=(None,))
    assert rounds == 1 and len(reps) == n


@pytest.mark.parametrize("density", [0.002, 0.02, 0.2])
def test_random_directed_graphs(density):
    rng = np.random.default_rng(int(density * 1000))
    n = 500
    adj = rng.random((n, n)) < density
    np.fill_diagonal(adj, False)
    lists = [np.nonzero(adj[u])[0].tolist() for u in range(n)]
    for priority in (rng.integers(0, 6, n), rng.standard_normal(n), np.array([len(x) for x in lists])):  # ties; floats; the degree
        check_graph(lists, priority, (density, priority.dtype), rng, lanes=(None, 4))


def test_the_assignment_with_equal_scores():
    """Three representatives list node 3 (ranks 0, 1, 2): "first" takes rank 0; "nearest" the largest score, the lower rank among
    equal ones, +0.0 above -0.0."""
    offsets, ids = dev(np.array([0, 1, 2, 3, 3], dtype=np.int64)), dev(np.array([3, 3, 3], dtype=np.int32))
    rank64, order = C.rank_of(dev(np.array([9, 8, 7, 1])))
    rank = rank64.to(torch.int32)
    state, rounds = C.greedy_rounds(offsets, ids, rank)
    assert state.cpu().tolist() == [C.REP, C.REP, C.REP, C.COVERED] and rounds == 2
    for scores, nearest in (([0.5, 0.7, 0.6], 1), ([0.7, 0.7, 0.6], 0), ([0.5, 0.7, 0.7], 1), ([-0.0, 0.0, -0.0], 1), ([0.0, -0.0, 0.0], 0)):
        sc = np.array(scores, dtype=np.float32)
        for assign, want in (("first", 0), ("nearest", nearest)):
            rep_of, reps, sizes = C.assign_members(offsets, ids, dev(sc), rank, order, state, assign)
            assert rep_of.cpu().tolist() == [0, 1, 2, want] and reps.cpu().tolist() == [0, 1, 2], (scores, assign)
            assert sizes.cpu().tolist() == [1 + (want == u) for u in range(3)]
            host = cref.greedy(np.array([0, 1, 2, 3, 3]), np.array([3, 3, 3], dtype=np.int32), sc, cref.rank_of([9, 8, 7, 1]), assign)
            assert host[0].tolist() == [0, 1, 2, want]


# ---- refusals -------------------------------------------------------------------------------------------------------------
def refused(rc, *words):
    assert rc != 0
    msg = N.lib.esmk_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)


def test_range_rows_refusals():
    S = torch.zeros((4, 16), dtype=torch.float32, device="cuda")
    counts = torch.zeros((4,), dtype=torch.int64, device="cuda")
    offsets = torch.zeros((5,), dtype=torch.int64, device="cuda")
    cursor = torch.zeros((4,), dtype=torch.int64, device="cuda")
    ids = torch.zeros((8,), dtype=torch.int32, device="cuda")
    scores = torch.zeros((8,), dtype=torch.float32, device="cuda")
    st, null = N.cur_stream(), ctypes.c_void_p(0)
    name = "esmk_op_range_rows"

    def call(S_=N.ptr(S), ld=16, n_rows=4, n_cols=16, id_base=0, fill=0, counts_=N.ptr(counts), off_=N.ptr(offsets), cur_=N.ptr(cursor),
             ids_=N.ptr(ids), scores_=N.ptr(scores), cap=8):
        return N.lib.esmk_op_range_rows(S_, ld, n_rows, n_cols, id_base, null, 1.0, fill, counts_, off_, cur_, ids_, scores_, cap, st)

    assert call() == 0 and call(fill=1) == 0 and call(n_rows=0) == 0
    assert call(off_=null, cur_=null, ids_=null, scores_=null) == 0 and call(fill=1, counts_=null) == 0  # what a pass does not read
    refused(call(S_=null), name, "null")
    refused(call(counts_=null), name, "null counts")
    for missing in ("off_", "cur_", "ids_", "scores_"):
        refused(call(fill=1, **{missing: null}), name, "null offsets, cursor, ids or scores")
    refused(call(n_cols=0), name, "n_cols must be 1 .. 2^22")
    refused(call(n_cols=(1 << 22) + 1, ld=(1 << 22) + 4), name, "n_cols must be 1 .. 2^22")
    refused(call(ld=12), name, "ldS")
    refused(call(ld=18, n_cols=16), name, "ldS")
    refused(call(id_base=-1), name, "id_base")
    refused(call(id_base=2 ** 31 - 16), name, "id_base")
    refused(call(n_rows=-1), name, "n_rows")
    refused(call(fill=1, cap=-1), name, "cap")
    refused(call(S_=ctypes.c_void_p(S.data_ptr() + 4)), name, "aligned")
    refused(call(counts_=ctypes.c_void_p(counts.data_ptr() + 4)), name, "aligned")
    refused(call(fill=1, off_=ctypes.c_void_p(offsets.data_ptr() + 4)), name, "aligned")
    torch.cuda.synchronize()
    assert not counts.any() and not ids.any()  # (the threshold 1.0 passes none of the zeros)


def test_graph_entry_refusals():
    n = 6
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
    ids = torch.zeros((4,), dtype=torch.int32, device="cuda")
    scores = torch.zeros((4,), dtype=torch.float32, device="cuda")
    rank = torch.arange(n, dtype=torch.int32, device="cuda")
    state, blocked, covered = (torch.zeros((n,), dtype=torch.int32, device="cuda") for _ in range(3))
    remaining = torch.zeros((1,), dtype=torch.int32, device="cuda")
    key = torch.zeros((n,), dtype=torch.int64, device="cuda")
    st, null = N.cur_stream(), ctypes.c_void_p(0)
    P = N.ptr

    def mark(off_=P(offsets), ids_=P(ids), n_=n, nnz=4, rank_=P(rank), state_=P(state), blocked_=P(blocked), covered_=P(covered), lanes=8):
        return N.lib.esmk_op_cluster_mark(off_, ids_, n_, nnz, rank_, state_, blocked_, covered_, lanes, st)

    def assign(off_=P(offsets), ids_=P(ids), scores_=P(scores), n_=n, nnz=4, rank_=P(rank), state_=P(state), nearest=1, key_=P(key), lanes=8):
        return N.lib.esmk_op_cluster_assign(off_, ids_, scores_, n_, nnz, rank_, state_, nearest, key_, lanes, st)

    def decide(state_=P(state), blocked_=P(blocked), covered_=P(covered), n_=n, rem_=P(remaining)):
        return N.lib.esmk_op_cluster_decide(state_, blocked_, covered_, n_, rem_, st)

    assert mark() == 0 and mark(ids_=null, nnz=0) == 0 and assign(nearest=0, scores_=null) == 0
    for call, name, flags in ((mark, "esmk_op_cluster_mark", ("blocked_", "covered_")), (assign, "esmk_op_cluster_assign", ("key_",))):
        for missing in ("off_", "rank_", "state_") + flags:
            refused(call(**{missing: null}), name, "null")
        refused(call(ids_=null), name, "null ids")
        refused(call(n_=0), name, "n <= 2^24")
        refused(call(n_=(1 << 24) + 1), name, "n <= 2^24")
        refused(call(nnz=-1), name, "nnz")
        for lanes in (0, 3, 128, -8):
            refused(call(lanes=lanes), name, "lanes")
        refused(call(off_=ctypes.c_void_p(offsets.data_ptr() + 4)), name, "aligned")
    refused(assign(scores_=null), "esmk_op_cluster_assign", "null scores")
    refused(assign(key_=ctypes.c_void_p(key.data_ptr() + 4)), "esmk_op_cluster_assign", "aligned")
    name = "esmk_op_cluster_decide"
    for missing in ("state_", "blocked_", "covered_", "rem_"):
        refused(decide(**{missing: null}), name, "null")
    refused(decide(n_=0), name, "n <= 2^24")
    refused(decide(state_=ctypes.c_void_p(state.data_ptr() + 2)), name, "aligned")
    torch.cuda.synchronize()
    assert not state.any() and not key.any() and not remaining.any()  # (decide was never launched: every call above was refused)
