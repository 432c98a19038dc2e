"""numpy references of the tempering kernels (esm_amd/csrc/tempering.hip): lm-design's n-gram term restated with
``collections.Counter`` over tuples, the acceptance with a temperature per chain and a third energy term, and a swap round of
replica exchange — the last two with the margin of tests/_design_ref.py that says which decisions a comparison may count.  No
torch, no engine: tests/test_tempering_cpu.py checks this file against hand-worked cases, the GPU tests check the kernels
against it."""
import math
from collections import Counter

import numpy as np

import _design_ref as R
from _sampling_ref import MASK32, philox4x32_10

SWAP = 4  # counter word 2, next to R.PROPOSAL and R.ACCEPTANCE
UNDECIDED_MARGIN = R.UNDECIDED_MARGIN
STANDARD = "ACDEFGHIKLMNPQRSTVWY"


def encode(seq, alphabet=STANDARD):
    """The codes of a string: the index in ``alphabet``, -1 outside it."""
    return [alphabet.find(ch) for ch in seq]


def ngram_counts(codes, n):
    """Counter of the windows of order ``n`` (tuples of codes) that hold no negative code."""
    codes = [int(c) for c in codes]
    return Counter(w for w in (tuple(codes[i: i + n]) for i in range(len(codes) - n + 1)) if min(w) >= 0)


def key_of(window, A):
    key = 0
    for c in window:
        key = key * A + c
    return key


def ngram_terms(codes, tables, A):
    """The fp64 terms p log(p / q) of every distinct n-gram of every order of ``tables`` (order -> dense table), ascending order."""
    terms = []
    for n in sorted(tables):
        counts = ngram_counts(codes, n)
        total = sum(counts.values())
        for window, c in counts.items():
            p = np.float64(c) / np.float64(total)
            terms.append(float(p * np.log(p / np.float64(tables[n][key_of(window, A)]))))
    return terms


def ngram_energy(codes, tables, A):
    """(energy, bound): the exactly rounded sum of the terms, and the bound m * 2^-51 * mean|term| of a comparison with a sum of
    the same m terms in another order whose logarithms may each differ by one ulp (the form of ``_design_ref.contact_energy``)."""
    t = ngram_terms(codes, tables, A)
    if not t:
        return 0.0, 0.0
    return float(math.fsum(t)), float(len(t) * 2.0 ** -51 * np.abs(t).mean())


def uniform_tables(A, orders):
    return {n: np.full((A ** n,), 1.0 / A ** n) for n in orders}


def random_tables(A, orders, seed):
    """Dense positive tables: a normalised random table with a floor of 1e-5, as ``Background.from_sequences`` leaves one."""
    rng = np.random.default_rng(seed)
    out = {}
    for n in orders:
        q = rng.gamma(0.5, size=A ** n)
        out[n] = np.maximum(q / q.sum(), 1e-5)
    return out


# ---- esmk_op_mh_accept_ex -------------------------------------------------------------------------------------------------------
EX_TEMPERATURES = (1.0, 1e6, 0.25)
EX_W_EXTRA = 0.5


def accept_ex_case(n=192):
    """``R.accept_case`` plus a rung per chain (0, 1, 2 in turn, shuffled) and an extra energy term."""
    case = R.accept_case(n=n)
    rng = np.random.default_rng(777)
    case["rung"] = rng.permutation(np.arange(n) % len(EX_TEMPERATURES)).astype(np.int32)
    case["e_extra"] = rng.uniform(0.0, 2.0, n)
    case["e_cur"] = case["e_cur"] + EX_W_EXTRA * case["e_extra"] + rng.uniform(-0.3, 0.3, n)
    return case


def combine_ex(w_contact, e_contact, w_lm, lp_sum, n_res, w_extra=0.0, e_extra=None):
    """E' = (w_contact * e_contact + w_lm * e_lm) + w_extra * e_extra, one rounding per operation; ``e_extra`` None: the sum of two."""
    e = np.float64(R.combine(w_contact, e_contact, w_lm, lp_sum, n_res)[0])
    if e_extra is None:
        return float(e)
    return float(e + np.float64(w_extra) * np.float64(e_extra))


def accept_ex(case, w_contact, w_lm, w_extra, inv_t, step, seed=R.ACCEPT_SEED):
    """(e_prop, u, accepted, undecided) arrays: chain c at ``inv_t[case["rung"][c]]``, the extra term from ``case["e_extra"]``."""
    n = case["tok"].shape[0]
    e_prop, u, acc, und = np.zeros(n), np.zeros(n), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for c in range(n):
        e_prop[c] = combine_ex(w_contact, case["e_contact"][c], w_lm, case["lp_sum"][c], case["n_res"][c], w_extra, case["e_extra"][c])
        u[c] = R.accept_uniform(seed, case["chain"][c], step)
        h = 0.0 if case["hastings"] is None else case["hastings"][c]
        k = min(max(int(case["rung"][c]), 0), len(inv_t) - 1)
        acc[c], und[c] = R.accept(e_prop[c], case["e_cur"][c], inv_t[k], h, u[c], case["tok"][c])
    return e_prop, u, acc, und


# ---- esmk_op_replica_swap -------------------------------------------------------------------------------------------------------
def swap_uniform(seed, ladder_id, rnd, k):
    """u = (word0 >> 8) * 2^-24 at counter (ladder id, round, 4, k), as a Python float (exact)."""
    seed = int(seed)
    w = philox4x32_10((int(ladder_id) & MASK32, int(rnd) & MASK32, SWAP, int(k)), (seed & MASK32, seed >> 32))
    return float(int(w[0]) >> 8) * 2.0 ** -24


def swap_round(rung, e_cur, inv_t, ladder_ids, seed, rnd):
    """(rung after the round int32 [n], accepted uint8 [n], u fp64 [n], undecided bool [n]) of swap round ``rnd`` on ladders of K =
    len(inv_t) consecutive chains.  Undecided (both chains of the pair): u within UNDECIDED_MARGIN of exp(a) where u decides."""
    rung = np.asarray(rung, dtype=np.int32)
    K = len(inv_t)
    out, acc = rung.copy(), np.zeros(rung.shape[0], dtype=np.uint8)
    u_out, und = np.full(rung.shape[0], -1.0), np.zeros(rung.shape[0], dtype=bool)
    for l, lid in enumerate(ladder_ids):
        mine = rung[l * K: (l + 1) * K].tolist()
        for k in range(rnd % 2, K - 1, 2):
            x, y = l * K + mine.index(k), l * K + mine.index(k + 1)
            a = float((np.float64(inv_t[k]) - np.float64(inv_t[k + 1])) * (np.float64(e_cur[x]) - np.float64(e_cur[y])))
            u = swap_uniform(seed, lid, rnd, k)
            u_out[x] = u_out[y] = u
            if a != a:
                ok = False
            elif a >= 0.0:
                ok = True
            else:
                ea = math.exp(a)
                ok = u < ea
                und[x] = und[y] = abs(u - ea) < UNDECIDED_MARGIN
            if ok:
                out[x], out[y] = k + 1, k
                acc[x] = acc[y] = 1
    return out, acc, u_out, und


SWAP_SEED = 0x5A7A91ADDE2  # the Philox key of the synthetic swap cases (no undecided decision: test_tempering_cpu.py)
SWAP_KS = (1, 2, 3, 8)
SWAP_LADDERS = 24


def swap_case(K, n_ladder=SWAP_LADDERS):
    """Synthetic ladders: rungs permuted at random, energies at the scale of the differences of 1 / T, so that a round holds
    accepted and rejected pairs."""
    rng = np.random.default_rng(9000 + K)
    rung = np.concatenate([rng.permutation(K) for _ in range(n_ladder)]).astype(np.int32)
    e_cur = rng.uniform(0.0, 4.0, n_ladder * K)
    inv_t = 1.0 / (0.5 * 1.7 ** np.arange(K))
    ladder_ids = (np.arange(n_ladder) * 7 + 3).astype(np.int32)
    return dict(rung=rung, e_cur=e_cur, inv_t=inv_t, ladder_ids=ladder_ids)
