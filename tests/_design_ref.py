"""numpy references of the design kernels (esm_amd/csrc/design.hip): the uniform single-site proposal in integer arithmetic on
the Philox words of tests/_sampling_ref.py, the contact term of the energy in fp64, the energy's arithmetic and the acceptance
rule with the margin that says which decisions a comparison may count.  No torch, no engine: tests/test_design_cpu.py checks
this file against hand-worked cases, the GPU tests check the kernels against it."""
import math

import numpy as np

from _sampling_ref import MASK32, philox4x32_10

PROPOSAL, ACCEPTANCE = 2, 3  # counter word 2
P_MIN, P_MAX = np.float32(2.0 ** -24), np.float32(1.0 - 2.0 ** -24)
UNDECIDED_MARGIN = 2.0 ** -40  # a decision is undecided when |u - exp(a)| is below this
MAX_UNDECIDED = 1  # per test case


def words(seed, chain, step, purpose):
    """The four output words at counter (chain, step, purpose, 0) under the key (seed & 0xffffffff, seed >> 32), as ints."""
    seed = int(seed)
    w = philox4x32_10((int(chain) & MASK32, int(step) & MASK32, purpose, 0), (seed & MASK32, seed >> 32))
    return [int(x) for x in w]


def proposal(seed, chain, step, positions, row, allowed_mask, force_new, V=64):
    """(site, old, token) of one chain: ``positions`` its list, ``row`` its current token row."""
    if len(positions) == 0:
        return -1, -1, -1
    w = words(seed, chain, step, PROPOSAL)
    site = int(positions[(w[0] * len(positions)) >> 32])
    old = int(row[site])
    cand = [v for v in range(V) if (allowed_mask >> v) & 1 and not (force_new and v == old)]
    if not cand:
        return site, old, -1
    return site, old, cand[(w[1] * len(cand)) >> 32]


def accept_uniform(seed, chain, step):
    """u = (word0 >> 8) * 2^-24 at counter (chain, step, 3, 0), as a Python float (exact)."""
    return float(words(seed, chain, step, ACCEPTANCE)[0] >> 8) * 2.0 ** -24


def contact_terms(p, target, min_sep, kind):
    """The fp64 terms of one map in row-major order of the counted pairs: p fp32 [S, S], target uint8 [S, S]."""
    p = np.asarray(p, dtype=np.float32)
    S = p.shape[0]
    i, j = np.nonzero((np.arange(S)[None, :] - np.arange(S)[:, None]) >= min_sep)
    y = np.asarray(target)[i, j]
    keep = (y == 1) if kind == "pos" else (y != 2)
    i, j, y = i[keep], j[keep], y[keep]
    q = np.minimum(np.maximum(p[i, j], P_MIN), P_MAX).astype(np.float64)
    return np.where(y == 1, np.log(q), np.log(1.0 - q))


def contact_energy(p, target, min_sep, kind):
    """(energy, count, bound): -mean of the terms (0.0 without terms), and the bound n * 2^-51 * mean|term| of a comparison with
    a sum of the same terms in another order whose logarithms may each differ by one ulp."""
    t = contact_terms(p, target, min_sep, kind)
    if t.size == 0:
        return 0.0, 0, 0.0
    return float(-(math.fsum(t) / t.size)), int(t.size), float(t.size * 2.0 ** -51 * np.abs(t).mean())


def combine(w_contact, e_contact, w_lm, lp_sum, n_res):
    """(E, e_lm) with one rounding per operation, as esmk_op_mh_accept: numpy float64 scalars do not fuse."""
    e_lm = -(np.float64(lp_sum) / np.float64(n_res)) if n_res > 0 else np.float64(0.0)
    return float(np.float64(w_contact) * np.float64(e_contact) + np.float64(w_lm) * e_lm), float(e_lm)


def accept(e_prop, e_cur, inv_t, hastings, u, tok):
    """(accepted, undecided) of the rule: tok >= 0 and (a >= 0 or u < exp(a)), a = -(e_prop - e_cur) * inv_t + hastings; inv_t =
    inf: tok >= 0 and e_prop <= e_cur.  Undecided: u within UNDECIDED_MARGIN of exp(a) where the comparison with u decides."""
    if tok < 0:
        return False, False
    dE = np.float64(e_prop) - np.float64(e_cur)
    if math.isinf(inv_t):
        return bool(dE <= 0.0), False
    a = float(-dE * np.float64(inv_t) + np.float64(hastings))
    if a != a:
        return False, False
    if a >= 0.0:
        return True, False
    ea = math.exp(a)
    return bool(u < ea), abs(u - ea) < UNDECIDED_MARGIN


ACCEPT_SEED = 0xD5E16A11CE  # the Philox key of the synthetic acceptance cases (no undecided decision: test_design_cpu.py)
ACCEPT_TEMPERATURES = (0.0, 1.0, 1e6)
ACCEPT_WEIGHTS = ((1.0, 1.0), (0.75, 0.0), (0.0, 2.5))


def accept_case(n=192, with_hastings=True):
    """Synthetic inputs of esmk_op_mh_accept for n chains: proposal energies with dE < 0, dE == 0 and dE > 0 in turn (the
    current energy is built from the proposal's, so dE == 0 is exact for weights (1, 1)), every eighth chain without a proposal
    (tok = -1).  Returns a dict of numpy arrays."""
    rng = np.random.default_rng(20240607)
    e_contact = rng.uniform(0.5, 6.0, n)
    n_res = rng.integers(20, 70, n).astype(np.int32)
    lp_sum = -rng.uniform(1.0, 4.0, n) * n_res
    shift = np.where(np.arange(n) % 3 == 0, -1.0, np.where(np.arange(n) % 3 == 1, 0.0, 1.0)) * rng.uniform(0.01, 3.0, n)
    base = np.array([combine(1.0, e_contact[c], 1.0, lp_sum[c], n_res[c])[0] for c in range(n)])
    e_cur = base - shift  # dE = shift (up to one rounding where shift != 0)
    tok = np.where(np.arange(n) % 8 == 7, -1, rng.integers(4, 24, n)).astype(np.int32)
    site = rng.integers(1, 40, n).astype(np.int32)
    hastings = rng.standard_normal(n) if with_hastings else None
    chain = (np.arange(n) * 3 + 5).astype(np.int32)
    return dict(e_contact=e_contact, lp_sum=lp_sum, n_res=n_res, e_cur=e_cur, tok=tok, site=site, hastings=hastings, chain=chain)


def accept_reference(case, w_contact, w_lm, temperature, step, seed=ACCEPT_SEED):
    """(e_prop, u, accepted, undecided) arrays of the reference on an ``accept_case``."""
    n = case["tok"].shape[0]
    inv_t = 1.0 / temperature if temperature > 0 else float("inf")
    e_prop, u, acc, und = np.zeros(n), np.zeros(n), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for c in range(n):
        e_prop[c] = combine(w_contact, case["e_contact"][c], w_lm, case["lp_sum"][c], case["n_res"][c])[0]
        u[c] = accept_uniform(seed, case["chain"][c], step)
        h = 0.0 if case["hastings"] is None else case["hastings"][c]
        acc[c], und[c] = accept(e_prop[c], case["e_cur"][c], inv_t, h, u[c], case["tok"][c])
    return e_prop, u, acc, und
