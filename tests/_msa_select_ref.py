"""numpy references of the MSA row-selection kernels (esm_amd/csrc/msa_select.hip), written from their definitions in
include/esmk.h: brute-force mismatch counts and neighbour counts, the integer greedy pick, the race keys on the Philox
reference of tests/_sampling_ref.py, ranks, and a seeded generator of family-structured alignments.  No torch, no engine: the
CPU tests check this file against answers worked out by hand, the GPU tests check the kernels against it."""
import numpy as np

import _sampling_ref as R

RACE = 2  # counter word 2 of the race keys (0 and 1: the sampler's permutation and token draw)
ALPHABET = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY-", dtype=np.uint8)


def mism(msa, L=None):
    """int64 [N, N]: the number of columns below L in which two rows differ.  msa uint8 [N, ld]."""
    a = np.asarray(msa, dtype=np.uint8)[:, :L]
    out = np.zeros((a.shape[0], a.shape[0]), dtype=np.int64)
    for i in range(a.shape[0]):
        out[i] = (a != a[i]).sum(1)
    return out


def mismatch_rows(msa, query, L=None):
    a = np.asarray(msa, dtype=np.uint8)[:, :L]
    n = a.shape[0]
    return np.stack([(a != a[min(max(int(q), 0), n - 1)]).sum(1) for q in query]).astype(np.int64)


def neighbor_counts(msa, max_mismatch, L=None):
    """count[i] = #{j : mism(i, j) <= max_mismatch}, j = i included; row by row, so a large alignment needs no N x N matrix."""
    a = np.asarray(msa, dtype=np.uint8)[:, :L]
    out = np.zeros(a.shape[0], dtype=np.int64)
    for i in range(a.shape[0]):
        out[i] = int(((a != a[i]).sum(1) <= max_mismatch).sum())
    return out


def max_mismatch(theta, L):
    """The largest integer m with float(m) < theta * L (fp64 product), found by search; -1 when there is none."""
    p = float(theta) * float(L)
    m = -1
    while float(m + 1) < p and m + 1 <= L:
        m += 1
    return m


def greedy(msa, num, first=0, mode=0, L=None):
    """The pick order of the integer rule: sel[0] = first; sel[k] = the unselected row with the largest (mode 0) / smallest
    (mode 1) sum of mismatches to sel[0 .. k-1], ties to the lowest row."""
    a = np.asarray(msa, dtype=np.uint8)[:, :L]
    n = a.shape[0]
    sums = np.zeros(n, dtype=np.int64)
    taken = np.zeros(n, dtype=bool)
    sel = [int(first)]
    taken[first] = True
    for _ in range(1, num):
        sums += (a != a[sel[-1]]).sum(1)
        cand = np.nonzero(~taken)[0]
        s = sums[cand]
        best = s.max() if mode == 0 else s.min()
        j = int(cand[np.nonzero(s == best)[0][0]])  # cand ascends: the first is the lowest row
        sel.append(j)
        taken[j] = True
    return sel


def race_u(n, seed, subsample):
    """fp64 u_i = (word0 >> 8) * 2^-24 at counter (subsample, 0, 2, i) under the key seed: exact."""
    w = R.word0(seed, subsample, 0, RACE, np.arange(n))
    return (w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def race_keys(n, seed, subsample, counts=None):
    u = race_u(n, seed, subsample)
    c = np.ones(n, dtype=np.int64) if counts is None else np.asarray(counts, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        key = -np.log(u) * c.astype(np.float64)
    key[(u == 0.0) | (c <= 0)] = np.inf
    return key


def ranks(key):
    """rank_i = #{j : key_j < key_i, or key_j == key_i and j < i}; NaN after everything, among NaNs the lower index first."""
    key = np.asarray(key, dtype=np.float64)
    n = key.shape[0]
    idx = np.arange(n)
    out = np.zeros(n, dtype=np.int64)
    nan = np.isnan(key)
    for i in range(n):
        if nan[i]:
            out[i] = int((~nan).sum() + (nan & (idx < i)).sum())
        else:
            with np.errstate(invalid="ignore"):
                out[i] = int(((key < key[i]) | ((key == key[i]) & (idx < i))).sum())
    return out


def weighted_pick(n, num, seed, subsample, counts=None):
    """The rows of a weighted / uniform subsample: the query plus the rows of rank below num, ascending."""
    key = race_keys(n, seed, subsample, counts)
    key[0] = -1.0
    return np.nonzero(ranks(key) < num)[0].tolist()


def min_relative_gap(key):
    """The smallest (b - a) / b over neighbouring distinct finite keys a < b in sorted order; inf when there are fewer than two."""
    k = np.sort(np.asarray(key, dtype=np.float64))
    k = k[np.isfinite(k)]
    d = np.diff(k)
    keep = d > 0
    return float((d[keep] / np.abs(k[1:][keep])).min()) if keep.any() else float("inf")


def family_msa(n, L, seed, n_families=5):
    """A seeded family-structured alignment uint8 [n, L] over the 20 residues and the gap: row 0 is the query, a few ancestors
    are mutated copies of it, every other row is a copy of a random ancestor mutated at its own rate (0.02 .. 0.5), and the last
    row duplicates row n // 2 so that exact ties exist."""
    rng = np.random.default_rng(seed)
    query = rng.integers(0, 20, L)
    anc = [query]
    for _ in range(n_families - 1):
        a = query.copy()
        hit = rng.random(L) < 0.35
        a[hit] = rng.integers(0, 21, int(hit.sum()))
        anc.append(a)
    rows = np.empty((n, L), dtype=np.int64)
    rows[0] = query
    for i in range(1, n):
        r = anc[int(rng.integers(0, n_families))].copy()
        hit = rng.random(L) < rng.uniform(0.02, 0.5)
        r[hit] = rng.integers(0, 21, int(hit.sum()))
        rows[i] = r
    if n >= 4:
        rows[n - 1] = rows[n // 2]
    return ALPHABET[rows]


def records(msa):
    """[(label, sequence)] of a byte alignment."""
    return [(f"seq{i}", bytes(row.tolist()).decode("ascii")) for i, row in enumerate(np.asarray(msa, dtype=np.uint8))]
