"""Cluster a library by embedding: greedy incremental clustering (the CD-HIT / MMseqs2 style) on a pooled-embedding index.

    index = esm_amd.EmbeddingIndex.load("db.npz").centered().to("cuda")
    near = index.range_search(queries, 0.5)                      # CSR: offsets int64 [Q + 1], ids int32, scores fp32 [nnz]
    out = index.cluster(0.5, priority="length", assign="first")   # = esm_amd.cluster_embeddings(index, 0.5, ...)
    out["rep_of"], out["representatives"], out["sizes"]           # int32 [N], [R], [R] on the device

    python -m esm_amd.cluster --index db.npz --threshold T [--center] [--priority length|degree] [--assign first|nearest]
                              --output clusters.tsv [--representatives reps.fasta] [--max-edges N] [--max-bytes B]

Definition (tests/_cluster_ref.py restates it as the plain sequential loop, and the kernels reproduce that exactly).
1. The graph: G = ``index.range_search(index, threshold, exclude_self=True)``; the out-list of u is out(u) = {j : S[u][j] >=
   threshold, j != u}, S the similarity matrix of the search.  S is not bitwise symmetric (the f16x3 partial products of
   S[j][i] add up in another order), so the graph is directed by definition — "u covers j" — and nothing relies on symmetry.
2. ``rank``: the position of a node when all nodes are sorted by priority descending, ties to the lower id.  ``priority``:
   "length" (``index.lengths``: CD-HIT's rule, the longest member represents its family), "degree" (the out-degree |out(u)|)
   or an int or float array [N] of the caller's; NaN in it is a ValueError.
3. Walk the nodes in rank order: a node that no earlier node has covered becomes a representative and covers every not yet
   decided node of its out-list.
4. ``assign="first"``: a member w belongs to the first representative that covered it, the one of the lowest rank among the
   representatives u with rank(u) < rank(w) and w in out(u).
5. ``assign="nearest"``: among those same representatives the one with the largest S[u][w] — in the total order of the IEEE
   bits, as the search's top-k — ties to the lower rank (CD-HIT's ``-g 1``).

On the device the walk runs in rounds (csrc/cluster.hip).  A node is undecided, a representative or covered.  The mark launch:
every undecided u sets blocked[w] and every new representative u sets covered[w] for the w of out(u) with rank(w) > rank(u);
the decide launch: an undecided node with covered set becomes a member, one that is neither covered nor blocked a
representative.  A representative can only cover later ranks, and an undecided earlier u with w in out(u) blocks w: when w is
decided, every earlier node that lists it is decided and has, if a representative, covered it, so by induction over rank
the result is the sequential loop's.  The undecided node of the lowest rank is never blocked: every round decides a node.
Family-structured graphs finish in a few rounds; a chain u1 -> u2 -> ... in rank order takes one round per node.  The host reads the
undecided counts of ``ROUNDS_PER_READ`` = 4 rounds in one copy, after every fourth round, and stops at the first zero.  The
assignment is one launch of an integer atomic max of [order(score) | ~rank]; ``sizes`` and the list of representatives are
torch index operations.

Not built: whitening; connected-component and Leiden / MCL clustering; re-clustering the survivors with the aligner's scores;
an index larger than one GPU's memory; a symmetric-closure graph; a single-pass fill that avoids the second GEMM; a few-query
GEMV search; the MSA Transformer and windows.
"""
import numpy as np
import torch

ROUNDS_PER_READ = 4
UNDECIDED, REP_NEW, REP, COVERED = 0, 1, 2, 3  # csrc/cluster.hip
PRIORITIES = ("length", "degree")
ASSIGN = ("first", "nearest")


def check_args(threshold, priority="length", assign="first", n=None):
    """ValueErrors of ``cluster_embeddings`` that need no device.  Returns the caller's priority as a numpy array, or None."""
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("cluster: the threshold is NaN")
    if assign not in ASSIGN:
        raise ValueError(f"cluster: assign must be 'first' or 'nearest', got {assign!r}")
    if isinstance(priority, str):
        if priority not in PRIORITIES:
            raise ValueError(f"cluster: priority must be 'length', 'degree' or an array [N], got {priority!r}")
        return None
    if isinstance(priority, torch.Tensor):
        priority = priority.detach().cpu().numpy()
    priority = np.asarray(priority)
    if priority.dtype.kind not in "iuf":
        raise ValueError(f"cluster: a priority array must hold ints or floats, got {priority.dtype}")
    priority = priority.astype(np.float64 if priority.dtype.kind == "f" else np.int64)
    if priority.ndim != 1 or (n is not None and priority.shape[0] != n):
        raise ValueError(f"cluster: a priority array must be [N] = [{n}], got {list(priority.shape)}")
    if priority.dtype.kind == "f" and np.isnan(priority).any():
        raise ValueError("cluster: the priority array holds NaN")
    return priority


def rank_of(priority):
    """(rank int64 [N], order int64 [N]) of a device or host tensor of priorities: ``order`` lists the nodes by priority
    descending, ties to the lower id (a stable sort); ``rank[order[r]] = r``."""
    order = torch.sort(priority, descending=True, stable=True).indices
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel(), device=order.device)
    return rank, order


def list_lanes(nnz, n):
    """The lanes that walk one out-list: the power of two at or above the mean list length, 1 .. 64.  Short lists get few
    lanes (a wavefront holds many lists, no lane idles through a loop it has no part in), long ones a whole wavefront
    (consecutive lanes read consecutive ids)."""
    mean = -(-int(nnz) // max(int(n), 1))
    lanes = 1
    while lanes < min(mean, 64):
        lanes *= 2
    return lanes


def greedy_rounds(offsets, ids, rank, lanes=None, max_rounds=None):
    """The rounds on a CSR of out-lists on the device (``rank`` int32 [N]): (state int32 [N], rounds)."""
    from . import ops

    n = rank.numel()
    dev = rank.device
    lanes = list_lanes(ids.numel(), n) if lanes is None else int(lanes)
    state = torch.zeros((n,), dtype=torch.int32, device=dev)
    blocked, covered = torch.zeros_like(state), torch.zeros_like(state)
    rounds = 0
    while max_rounds is None or rounds < max_rounds:
        remaining = torch.zeros((ROUNDS_PER_READ,), dtype=torch.int32, device=dev)
        for r in range(ROUNDS_PER_READ):
            ops.cluster_mark(offsets, ids, rank, state, blocked, covered, lanes)
            ops.cluster_decide(state, blocked, covered, remaining[r:r + 1])
        left = remaining.cpu().tolist()  # the one read of these rounds
        if 0 in left:
            return state, rounds + left.index(0) + 1
        rounds += ROUNDS_PER_READ
    raise RuntimeError(f"cluster: {max_rounds} rounds did not decide every node")


def assign_members(offsets, ids, scores, rank, order, state, assign="first", lanes=None):
    """(rep_of, representatives, sizes) int32 on the device from the final states (module docstring, 4 and 5)."""
    from . import ops

    n = rank.numel()
    lanes = list_lanes(ids.numel(), n) if lanes is None else int(lanes)
    key = ops.cluster_assign(offsets, ids, scores, rank, state, assign == "nearest", lanes=lanes)
    is_rep = state != COVERED
    rep_rank = (0xFFFFFFFF - (key & 0xFFFFFFFF)).clamp_(0, n - 1)  # (a representative's own key is 0: clamped, then unused)
    nodes = torch.arange(n, device=rank.device)
    rep_of = torch.where(is_rep, nodes, order[rep_rank])
    representatives = order[is_rep[order]]
    sizes = torch.bincount(rep_of, minlength=n)[representatives]
    return rep_of.to(torch.int32), representatives.to(torch.int32), sizes.to(torch.int32)


def cluster_embeddings(index, threshold, priority="length", assign="first", max_edges=1 << 28, max_bytes=2 << 30):
    """Greedy incremental clustering of an index on the device (module docstring).  Returns a dict of device tensors
    ``rep_of`` int32 [N] (a representative names itself), ``representatives`` int32 [R] in rank order, ``sizes`` int32 [R],
    ``rank`` int32 [N], the host int ``rounds`` and ``neighbors``, the CSR of ``range_search``.  Cluster a centred index
    (``index.centered()``): a threshold on raw cosines separates nothing."""
    n = len(index)
    own = check_args(threshold, priority, assign, n)
    G = index.range_search(index, threshold, exclude_self=True, max_edges=max_edges, max_bytes=max_bytes)
    dev = G["offsets"].device
    with torch.cuda.device(dev):
        if own is not None:
            prio = torch.from_numpy(own).to(dev)
        elif priority == "length":
            prio = torch.from_numpy(np.asarray(index.lengths, dtype=np.int64)).to(dev)
        else:
            prio = G["offsets"][1:] - G["offsets"][:-1]
        rank64, order = rank_of(prio)
        rank = rank64.to(torch.int32)
        state, rounds = greedy_rounds(G["offsets"], G["ids"], rank, max_rounds=n + ROUNDS_PER_READ)
        rep_of, representatives, sizes = assign_members(G["offsets"], G["ids"], G["scores"], rank, order, state, assign)
    return dict(rep_of=rep_of, representatives=representatives, sizes=sizes, rank=rank, rounds=rounds, neighbors=G)


# ---- text -------------------------------------------------------------------------------------------------------------------
TSV_HEADER = ("member", "representative", "cosine", "cluster_size")


def member_cosines(rep_of, offsets, ids, scores):
    """Per node the cosine to its representative as the CSR stores it, S[rep][member]; 1 for a representative.  numpy arrays."""
    out = np.ones((len(rep_of),), dtype=np.float32)
    for w, u in enumerate(rep_of):
        if u != w:
            lo, hi = int(offsets[u]), int(offsets[u + 1])
            i = lo + int(np.searchsorted(ids[lo:hi], w))
            if i >= hi or ids[i] != w:
                raise ValueError(f"cluster: node {w} is not in the out-list of its representative {u}")
            out[w] = scores[i]
    return out


def write_tsv(fh, labels, rep_of, cosine, sizes_of_rep):
    """One line per protein in id order: member label, representative label, cosine of the member to its representative (1
    for the representative itself), cluster size.  ``sizes_of_rep``: {representative id: size}."""
    fh.write("\t".join(TSV_HEADER) + "\n")
    for w, u in enumerate(rep_of):
        fh.write("\t".join([labels[w], labels[int(u)], f"{float(cosine[w]):.6f}", str(int(sizes_of_rep[int(u)]))]) + "\n")


# ---- command line -----------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    import argparse

    p = argparse.ArgumentParser(prog="python -m esm_amd.cluster", description="Greedy incremental clustering of a pooled-embedding index")
    p.add_argument("--index", required=True, help="the .npz written by python -m esm_amd.search index")
    p.add_argument("--threshold", type=float, required=True, help="cosine at or above which a representative covers a protein")
    p.add_argument("--center", action="store_true", help="subtract the database mean first (an index that is not centred yet)")
    p.add_argument("--priority", choices=PRIORITIES, default="length", help="who represents: the longest or the best connected")
    p.add_argument("--assign", choices=ASSIGN, default="first", help="a member's representative: the first that covered it or the nearest")
    p.add_argument("--output", required=True, help="the TSV: member, representative, cosine, cluster size")
    p.add_argument("--representatives", default=None, help="also write the representatives as FASTA (needs an index with sequences)")
    p.add_argument("--max-edges", type=int, default=1 << 28, help="refuse a threshold that passes more pairs")
    p.add_argument("--max-bytes", type=int, default=2 << 30, help="scratch of one similarity block")
    args = p.parse_args(argv)
    if args.threshold != args.threshold:
        p.error("--threshold is NaN")
    if args.max_edges < 0:
        p.error("--max-edges must not be negative")
    return args


def main(argv=None):
    args = parse_args(argv)
    from .search import EmbeddingIndex

    index = EmbeddingIndex.load(args.index)
    if args.representatives and index.sequences is None:
        raise ValueError("cluster: --representatives needs an index with sequences (it was written with --no-sequences)")
    if args.center:
        if index.center is not None:
            raise ValueError("cluster: --center on an index that is centred already")
        index = index.centered()
    index.to("cuda")
    out = cluster_embeddings(index, args.threshold, priority=args.priority, assign=args.assign, max_edges=args.max_edges,
                             max_bytes=args.max_bytes)
    rep_of = out["rep_of"].cpu().numpy()
    reps, sizes = out["representatives"].cpu().numpy(), out["sizes"].cpu().numpy()
    G = {k: v.cpu().numpy() for k, v in out["neighbors"].items()}
    with open(args.output, "w") as fh:
        write_tsv(fh, index.labels, rep_of, member_cosines(rep_of, G["offsets"], G["ids"], G["scores"]), dict(zip(reps.tolist(), sizes.tolist())))
    if args.representatives:
        with open(args.representatives, "w") as fh:
            for u in reps.tolist():
                fh.write(f">{index.labels[u]}\n{index.sequences[u]}\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
