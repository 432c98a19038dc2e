"""numpy and plain-Python restatement of esm_amd/msa_build.py and esm_amd/csrc/msa_build.hip, written from their rules: the
projection of alignment paths onto the query's columns with its six integers, the gap-aware pairwise identity, the rank
order, the row filter, the sequential redundancy walk, and the a3m text.  The kernels and the pipeline reproduce these
exactly (bytes, integers, fp32 bit patterns)."""
import numpy as np

F32 = np.float32
GAP = ord("-")


# ---- the projection -------------------------------------------------------------------------------------------------------
def project(cols, col_offsets, seqs, seq_off, seq_len, query, ld=None):
    """(msa uint8 [P, ld], stats int32 [P, 6]).  ``cols`` [n, 2], ``col_offsets`` [P + 1] into it, ``seqs`` the blob (bytes or a
    uint8 array), ``seq_off`` / ``seq_len`` [P], ``query`` bytes [Lq].  Everything that names something outside its buffer is
    clamped or ignored, as the header states."""
    cols = np.asarray(cols, dtype=np.int64).reshape(-1, 2)
    seqs = np.frombuffer(bytes(seqs), dtype=np.uint8) if not isinstance(seqs, np.ndarray) else seqs
    query = np.frombuffer(bytes(query), dtype=np.uint8) if not isinstance(query, np.ndarray) else query
    P, Lq, n, nbytes = len(col_offsets) - 1, len(query), len(cols), len(seqs)
    ld = (Lq + 3) // 4 * 4 if ld is None else ld
    msa = np.zeros((P, ld), dtype=np.uint8)
    msa[:, :Lq] = GAP
    stats = np.zeros((P, 6), dtype=np.int32)
    for p in range(P):
        lo = min(max(int(col_offsets[p]), 0), n)
        hi = min(max(int(col_offsets[p + 1]), lo), n)
        off = int(seq_off[p])
        length = min(max(int(seq_len[p]), 0), nbytes - off) if 0 <= off < nbytes else 0
        path = cols[lo:hi]
        kind = []  # per path column: "m", "d", "i" or None
        for i, j in path:
            qi, tj = 0 <= i < Lq, 0 <= j < length
            kind.append("m" if qi and tj else "d" if qi and j == -1 else "i" if i == -1 and tj else None)
        at = [c for c, k in enumerate(kind) if k == "m"]
        for c in at:
            i, j = path[c]
            msa[p, i] = seqs[off + j]
        n_ident = sum(1 for c in at if seqs[off + path[c][1]] == query[path[c][0]])
        inside = range(at[0] + 1, at[-1]) if at else range(0)
        stats[p] = [len(at), n_ident, sum(1 for c in inside if kind[c] == "i"), sum(1 for c in inside if kind[c] == "d"),
                    path[at[0]][0] if at else -1, path[at[-1]][0] if at else -1]
    return msa, stats


# ---- pairwise identity ------------------------------------------------------------------------------------------------------
def pair_identity(msa, L=None, gap=GAP, min_overlap=1, ldS=None):
    """fp32 [N, ldS] (ldS: N rounded up to 4): same / both over the columns below L, 0 where both < min_overlap and in the
    columns behind N."""
    msa = np.asarray(msa, dtype=np.uint8)
    N = msa.shape[0]
    L = msa.shape[1] if L is None else L
    ldS = (N + 3) // 4 * 4 if ldS is None else ldS
    m = msa[:, :L]
    letter = m != gap
    S = np.zeros((N, ldS), dtype=F32)
    for r in range(N):
        shared = letter[r][None, :] & letter
        both = shared.sum(1).astype(np.int64)
        same = (shared & (m[r][None, :] == m)).sum(1).astype(np.int64)
        ok = both >= max(int(min_overlap), 1)
        S[r, :N][ok] = same[ok].astype(F32) / both[ok].astype(F32)
    return S


# ---- rank, filters ----------------------------------------------------------------------------------------------------------
def rank_order(scores, passed):
    """The rows in rank order: row 0, then the hits that passed by score descending, ties to the lower row, then the others
    likewise.  ``scores`` [N] (row 0 unused), ``passed`` bool [N]."""
    hits = sorted(range(1, len(scores)), key=lambda r: (not bool(passed[r]), -float(scores[r]), r))
    return [0] + hits


def row_filter(stats, Lq, min_coverage, min_query_identity):
    """bool [N]: n_match >= 1, n_match >= min_coverage * Lq and n_ident >= min_query_identity * n_match, the products in fp64."""
    nm, ni = stats[:, 0].astype(np.float64), stats[:, 1].astype(np.float64)
    return (stats[:, 0] >= 1) & (nm >= np.float64(min_coverage) * np.float64(Lq)) & (ni >= np.float64(min_query_identity) * nm)


def redundancy_walk(S, rows, max_identity):
    """The kept rows of ``rows`` (in rank order): a row stays unless an earlier kept row k has S[k][row] >= max_identity, a
    float32 comparison."""
    thr = F32(max_identity)
    kept = []
    for r in rows:
        if not any(S[k, r] >= thr for k in kept):
            kept.append(r)
    return kept


def build(query, hit_seqs, scores, cols, col_offsets, min_coverage=0.5, max_identity=0.9, min_query_identity=0.0, min_overlap=8):
    """Steps 2 to 4 for one query: (the kept rows of [query; hits] in rank order, msa uint8 [P + 1, Lq], stats int32 [P + 1, 6],
    passed bool [P + 1]).  ``hit_seqs``: the P hits' sequences in the prefilter's order; ``scores`` [P]; ``cols`` /
    ``col_offsets`` [P + 1] their paths."""
    Lq, P = len(query), len(hit_seqs)
    lens = [len(s) for s in hit_seqs]
    off = np.concatenate([[0], np.cumsum(lens)])[:P] if P else np.zeros((0,), dtype=np.int64)
    hits, hstats = project(cols, col_offsets, "".join(hit_seqs).encode("ascii"), off, lens, query.encode("ascii"), ld=Lq)
    msa = np.concatenate([np.frombuffer(query.encode("ascii"), dtype=np.uint8)[None, :], hits], 0)
    stats = np.concatenate([np.array([[Lq, Lq, 0, 0, 0, Lq - 1]], dtype=np.int32), hstats], 0)
    passed = row_filter(stats, Lq, min_coverage, min_query_identity)
    passed[0] = True
    order = rank_order(np.concatenate([[np.inf], np.asarray(scores, dtype=np.float64)]), passed)
    rows = [r for r in order if passed[r]]
    if max_identity is not None and P:
        rows = redundancy_walk(pair_identity(msa, Lq, GAP, min_overlap), rows, max_identity)
    return rows, msa, stats, passed


# ---- the text ---------------------------------------------------------------------------------------------------------------
def a3m_row(row, seq, cols, insertions=True):
    """The a3m row of a hit from its match states ``row``, its residues ``seq`` and its path."""
    Lq = len(row)
    cols = [(int(i), int(j)) for i, j in cols]
    match = [c for c, (i, j) in enumerate(cols) if 0 <= i < Lq and 0 <= j < len(seq)]
    if not match:
        return "-" * Lq
    text = "-" * cols[match[0]][0]
    for i, j in cols[match[0]:match[-1] + 1]:
        if i >= 0:
            text += row[i] if j >= 0 else "-"
        elif insertions:
            text += seq[j].lower()
    return text + "-" * (Lq - 1 - cols[match[-1]][0])


def a3m_text(labels, rows, seqs, paths, insertions=True):
    """The file: ``labels`` / ``rows`` [R] (the query first), ``seqs`` / ``paths`` [R - 1] of the hits."""
    lines = [f">{labels[0]}", rows[0]]
    for k in range(1, len(rows)):
        lines += [f">{labels[k]}", a3m_row(rows[k], seqs[k - 1], paths[k - 1], insertions)]
    return "\n".join(lines) + "\n"


# ---- test inputs: valid paths from a host generator -------------------------------------------------------------------------
LETTERS = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)


def random_path(rng, Lq, Ls, local):
    """A valid path of a query of Lq against a hit of Ls residues: ascending, every step a match, (i, -1) or (-1, j).  Global:
    from (0, 0) to the end of both; local: a sub-rectangle, beginning and ending in a match."""
    def walk(i, j, i1, j1):  # every residue of [i, i1) and [j, j1) once
        cols = []
        while i < i1 or j < j1:
            step = int(rng.integers(0, 10))
            if i < i1 and j < j1 and step < 7:
                cols.append((i, j))
                i, j = i + 1, j + 1
            elif i < i1 and (j >= j1 or step < 9):
                cols.append((i, -1))
                i += 1
            else:
                cols.append((-1, j))
                j += 1
        return cols

    if not local:
        return walk(0, 0, Lq, Ls)
    i0, j0 = int(rng.integers(0, Lq)), int(rng.integers(0, Ls))
    i1, j1 = int(rng.integers(i0, Lq)), int(rng.integers(j0, Ls))  # the last match
    if i1 == i0 or j1 == j0:
        return [(i0, j0)]
    return [(i0, j0)] + walk(i0 + 1, j0 + 1, i1, j1) + [(i1, j1)]


def case(rng, Lq, P, cap=None, special=False):
    """(paths [P] of lists, seqs [P] of uint8 arrays, query uint8 [Lq])."""
    query = rng.choice(LETTERS, Lq)
    paths, seqs = [], []
    for p in range(P):
        Ls = int(rng.integers(1, min(Lq + 10, cap or 1 << 30) + 1))
        seq = rng.choice(LETTERS, Ls)
        if Lq > 3 and Ls > 3 and rng.integers(0, 2):  # share letters with the query, so that n_ident is not all noise
            n = min(Lq, Ls)
            seq[:n] = np.where(rng.random(n) < 0.6, query[:n], seq[:n])
        seqs.append(seq)
        paths.append(random_path(rng, Lq, Ls, local=bool(p % 2)))
    if special:
        assert P >= 5
        paths[0] = []                                                   # an empty path
        paths[1] = [(i, -1) for i in range(min(Lq, 3))] + [(-1, 0)]      # gaps only
        seqs[2] = seqs[2][:1]
        paths[2] = [(Lq // 2, 0)]                                       # a hit of one residue
        seqs[3] = rng.choice(LETTERS, Lq + 2)
        paths[3] = [(-1, 0)] + [(i, i + 1) for i in range(Lq)] + [(-1, Lq + 1)]  # every query column
    return paths, seqs, query


def tables(paths, seqs):
    cols = np.array([c for path in paths for c in path], dtype=np.int32).reshape(-1, 2)
    col_offsets = np.concatenate([[0], np.cumsum([len(path) for path in paths])]).astype(np.int64)
    lens = np.array([len(s) for s in seqs], dtype=np.int32)
    seq_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return cols, col_offsets, np.concatenate(seqs).astype(np.uint8), seq_off, lens
