"""numpy restatement of the range search and the clustering (esm_amd/csrc/cluster.hip, esm_amd/cluster.py): the centre
arithmetic, the thresholded CSR of a given fp32 similarity matrix, and greedy incremental clustering as the plain sequential
loop with both assignment rules.  The kernels reproduce these exactly."""
import numpy as np

from _search_ref import F32, order


# ---- centring -------------------------------------------------------------------------------------------------------------
def center_of(vectors):
    """(center fp32 [E], centred vectors fp32 [N, E]): per column the fp64 sum in ascending i, divided by N, rounded once;
    then one fp32 subtraction per element."""
    vectors = np.asarray(vectors, dtype=F32)
    acc = np.zeros((vectors.shape[1],), dtype=np.float64)
    for i in range(vectors.shape[0]):
        acc = acc + vectors[i].astype(np.float64)
    center = (acc / np.float64(vectors.shape[0])).astype(F32)
    return center, (vectors - center[None, :]).astype(F32)


# ---- the thresholded CSR --------------------------------------------------------------------------------------------------
def range_rows(S, threshold, n_cols=None, id_base=0, exclude=None):
    """(counts int64 [R], ids int32 [nnz], scores fp32 [nnz]) of S fp32 [R, >= n_cols]: per row, in ascending column, every
    column with S >= threshold as a float comparison (NaN never, a tie and -0.0 against +0.0 do) whose id is not exclude[row]."""
    S = np.asarray(S, dtype=F32)
    n_cols = S.shape[1] if n_cols is None else n_cols
    thr = F32(threshold)
    col_ids = id_base + np.arange(n_cols, dtype=np.int64)
    counts, ids, scores = [], [], []
    with np.errstate(invalid="ignore"):
        for q in range(S.shape[0]):
            ok = S[q, :n_cols] >= thr  # float32 against float32
            if exclude is not None:
                ok &= col_ids != int(exclude[q])
            counts.append(int(ok.sum()))
            ids.append(col_ids[ok])
            scores.append(S[q, :n_cols][ok])
    return np.array(counts, dtype=np.int64), np.concatenate(ids).astype(np.int32), np.concatenate(scores).astype(F32)


def csr_of(S, threshold, exclude_self=False):
    """(offsets int64 [R + 1], ids, scores) of a whole similarity matrix, as ``EmbeddingIndex.range_search`` returns it.
    Vectorised: the same rule as ``range_rows`` (``>=`` on float32)."""
    S = np.asarray(S, dtype=F32)
    ok = S >= F32(threshold)
    if exclude_self:
        ok[np.arange(min(S.shape)), np.arange(min(S.shape))] = False
    rows, cols = np.nonzero(ok)  # row-major: ascending column within a row
    offsets = np.concatenate([[0], np.cumsum(ok.sum(1))]).astype(np.int64)
    return offsets, cols.astype(np.int32), S[rows, cols]


# ---- greedy incremental clustering ------------------------------------------------------------------------------------------
def rank_of(priority):
    """rank int32 [N]: the position of every node when all are sorted by priority descending, ties to the lower id."""
    priority = np.asarray(priority)
    if priority.dtype.kind == "f" and np.isnan(priority).any():
        raise ValueError("NaN priority")
    nodes = sorted(range(len(priority)), key=lambda i: (-priority[i].item(), i))
    rank = np.empty((len(priority),), dtype=np.int32)
    rank[nodes] = np.arange(len(priority), dtype=np.int32)
    return rank


def rounds_of(offsets, ids, rank):
    """The device's rounds, restated: (is_rep bool [N], rounds).  A round: every undecided u blocks, and every representative
    of the round before covers, the w of its out-list with rank(w) > rank(u); then an undecided node that is covered becomes
    a member and one that is neither covered nor blocked a representative.  The count is the round after which none is left."""
    n = len(rank)
    UNDECIDED, REP_NEW, REP, COVERED = 0, 1, 2, 3
    state = np.zeros((n,), dtype=np.int64)
    rounds = 0
    while (state == UNDECIDED).any():
        blocked, covered = np.zeros((n,), dtype=bool), np.zeros((n,), dtype=bool)
        for u in np.nonzero((state == UNDECIDED) | (state == REP_NEW))[0]:
            out = ids[int(offsets[u]):int(offsets[u + 1])]
            later = out[rank[out] > rank[u]]
            (blocked if state[u] == UNDECIDED else covered)[later] = True
        und = state == UNDECIDED
        state[state == REP_NEW] = REP
        state[und & covered] = COVERED
        state[und & ~covered & ~blocked] = REP_NEW
        rounds += 1
    return state != COVERED, max(rounds, 1)


def greedy(offsets, ids, scores, rank, assign="first"):
    """The sequential loop.  (rep_of int32 [N], representatives int32 [R] in rank order, sizes int32 [R]).  Walk the nodes by
    rank; a node no earlier node has covered becomes a representative and covers the undecided nodes of its out-list.  A member
    belongs to ("first") the representative that covered it, or ("nearest") among the earlier-ranked representatives that list
    it to the one with the largest score in the total order of the IEEE bits, ties to the lower rank."""
    n = len(rank)
    nodes = np.argsort(rank, kind="stable")
    UNDECIDED, REP, COVERED = 0, 1, 2
    state = np.zeros((n,), dtype=np.int64)
    rep_of = np.full((n,), -1, dtype=np.int32)
    best = {}  # member -> (order(score), representative) of "nearest"
    score_order = order(np.asarray(scores, dtype=F32)) if len(ids) else np.zeros((0,), dtype=np.uint32)
    reps = []
    for u in nodes:
        u = int(u)
        if state[u] != UNDECIDED:
            continue
        state[u] = REP
        rep_of[u] = u
        reps.append(u)
        for i in range(int(offsets[u]), int(offsets[u + 1])):
            w = int(ids[i])
            if state[w] == UNDECIDED:
                state[w] = COVERED
                rep_of[w] = u
            if assign == "nearest" and state[w] == COVERED and rank[w] > rank[u]:
                o = int(score_order[i])
                if w not in best or o > best[w][0]:  # (a later representative has a higher rank: it needs a greater score)
                    best[w] = (o, u)
    if assign == "nearest":
        for w, (_, u) in best.items():
            rep_of[w] = u
    reps = np.array(reps, dtype=np.int32)
    sizes = np.array([(rep_of == u).sum() for u in reps], dtype=np.int32)
    return rep_of, reps, sizes
