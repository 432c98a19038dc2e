"""The tempering kernels one launch at a time (esm_amd/csrc/tempering.hip through esm_amd/ops.py) against the numpy references of
tests/_tempering_ref.py: the n-gram term within the reordering bound of its fp64 additions and one ulp per logarithm — and bit for
bit between B = 1 and a place inside B = 5 —, the acceptance with rungs and a third term on synthetic energies with the decisions
the margin rule may count (and bit for bit equal to ``ops.mh_accept`` without either), and the swap rounds of replica exchange."""
import functools

import numpy as np
import pytest
import torch

import _design_ref as R
import _tempering_ref as TR
from esm_amd import ops

pytestmark = pytest.mark.gpu
A, V = 20, 33
X = 24  # a token outside the background's alphabet
ORDER_MASKS = ((1,), (4,), (1, 2, 3), (1, 2, 3, 4))


def dev(x, dtype):
    return torch.as_tensor(np.asarray(x)).to(dtype).cuda()


# ---- esmk_op_ngram_energy -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def background():
    """(code int32 [V], its inverse, tables order -> fp64 [A^n]): tokens 4 .. 23 carry the 20 codes in a shuffled order."""
    rng = np.random.default_rng(41)
    code = np.full(V, -1, dtype=np.int32)
    code[4:24] = rng.permutation(A)
    token_of = {int(c): t for t, c in enumerate(code) if c >= 0}
    return code, token_of, TR.random_tables(A, (1, 2, 3, 4), seed=42)


def chains(S):
    """int64 [7, S + 2] and the codes of every chain: one repeated residue, code A - 1 throughout (the last key of every table), two
    random chains, and random chains with a token outside the alphabet at residue 0, at S - 1 and in the middle."""
    code, token_of, _ = background()
    rng = np.random.default_rng(500 + S)
    rows = [np.full(S, 3), np.full(S, A - 1)] + [rng.integers(0, A, S) for _ in range(2)]
    rows += [rng.integers(0, 4, S) for _ in range(3)]  # four letters: n-grams repeat at every order
    tokens = np.zeros((7, S + 2), dtype=np.int64)
    tokens[:, -1] = 2
    for b, row in enumerate(rows):
        tokens[b, 1:-1] = [token_of[int(c)] for c in row]
    tokens[4, 1], tokens[5, S], tokens[6, 1 + S // 2] = X, X, X
    codes = [[int(code[t]) for t in tokens[b, 1:-1]] for b in range(7)]
    return tokens, codes


@pytest.mark.parametrize("S", [1, 2, 3, 4, 5, 255, 256, 257, 1022])
def test_ngram_energy_against_the_counter_restatement_and_across_batches(S):
    code, _, tables = background()
    tokens, codes = chains(S)
    tok_d, code_d = dev(tokens, torch.int64), dev(code, torch.int32)
    q_d = {n: dev(q, torch.float64) for n, q in tables.items()}
    assert codes[4][0] == -1 and codes[5][-1] == -1 and codes[6][S // 2] == -1 and min(min(c) for c in codes[:4]) >= 0
    for orders in ORDER_MASKS:
        chosen = {n: q_d[n] for n in orders}
        got = ops.ngram_energy(tok_d, 1, S, code_d, A, chosen)
        assert got.dtype == torch.float64 and got.shape == (7,)
        for b in range(7):
            want, bound = TR.ngram_energy(codes[b], {n: tables[n] for n in orders}, A)
            print(f"S={S} orders={orders} chain={b} got={got[b].item()!r} want={want!r} bound={bound!r}")
            assert abs(got[b].item() - want) <= bound, (S, orders, b, got[b].item(), want, bound)
            if S < min(orders):
                assert got[b].item() == 0.0  # no window: exactly 0
        # the same chain alone and inside a batch of five: the same bits
        five = ops.ngram_energy(tok_d[:5].contiguous(), 1, S, code_d, A, chosen)
        alone = ops.ngram_energy(tok_d[3:4].contiguous(), 1, S, code_d, A, chosen)
        assert torch.equal(five, got[:5]) and torch.equal(alone, five[3:4])
    if S == 1:  # the only residue is outside the alphabet: no valid window at any order
        assert ops.ngram_energy(tok_d, 1, S, code_d, A, q_d)[4].item() == 0.0


def test_ngram_energy_reads_the_residues_it_is_given():
    """``first`` and ``S`` choose the residues: a prefix of a longer row is the energy of that prefix alone."""
    code, _, tables = background()
    tokens, codes = chains(300)
    q_d = {n: dev(tables[n], torch.float64) for n in (1, 2, 3)}
    got = ops.ngram_energy(dev(tokens, torch.int64), 11, 200, dev(code, torch.int32), A, q_d)
    for b in range(7):
        want, bound = TR.ngram_energy(codes[b][10:210], {n: tables[n] for n in (1, 2, 3)}, A)
        assert abs(got[b].item() - want) <= bound, b


# ---- esmk_op_mh_accept_ex -------------------------------------------------------------------------------------------------------
T = 70


def run_accept(case, tokens, ex, **kw):
    """One call of ``ops.mh_accept`` (``ex`` False) or ``ops.mh_accept_ex`` on fresh device copies: every output and the state."""
    n = case["tok"].shape[0]
    tok_d, e_cur = dev(tokens, torch.int64), dev(case["e_cur"], torch.float64)
    ecc, elc = torch.full((n,), -7.0, dtype=torch.float64).cuda(), torch.full((n,), -9.0, dtype=torch.float64).cuda()
    exc = torch.full((n,), -11.0, dtype=torch.float64).cuda()
    common = dict(e_contact=dev(case["e_contact"], torch.float64), lp_sum=dev(case["lp_sum"], torch.float64),
                  n_res=dev(case["n_res"], torch.int32), hastings=dev(case["hastings"], torch.float64), w_contact=1.0, w_lm=1.0,
                  seed=R.ACCEPT_SEED, e_contact_cur=ecc, e_lm_cur=elc)
    args = (tok_d, dev(case["site"], torch.int32), dev(case["tok"], torch.int32), dev(case["chain"], torch.int32), e_cur)
    if ex:
        out = ops.mh_accept_ex(*args, e_extra_cur=exc, **common, **kw)
    else:
        out = ops.mh_accept(*args, **common, **kw)
    return [t.cpu().numpy() for t in out] + [tok_d.cpu().numpy(), e_cur.cpu().numpy(), ecc.cpu().numpy(), elc.cpu().numpy(),
                                            exc.cpu().numpy()]


def test_accept_ex_without_extras_is_mh_accept_bit_for_bit():
    case = R.accept_case()
    n = case["tok"].shape[0]
    tokens = np.random.default_rng(9).integers(4, 24, size=(n, T))
    for step, temperature in enumerate(R.ACCEPT_TEMPERATURES):
        inv_t = 1.0 / temperature if temperature > 0 else float("inf")
        plain = run_accept(case, tokens, False, inv_temperature=inv_t, step=step)
        ex = run_accept(case, tokens, True, inv_t=dev([inv_t], torch.float64), step=step)
        for a, b in zip(plain[:-1], ex[:-1]):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (step, temperature)
        assert (ex[-1] == -11.0).all()  # no extra term: its current value is not written
        assert 0 < plain[0].sum() < n


def test_accept_ex_with_three_rungs_and_a_third_term():
    case = TR.accept_ex_case()
    n = case["tok"].shape[0]
    tokens = np.random.default_rng(9).integers(4, 24, size=(n, T))
    inv_t = [1.0 / t for t in TR.EX_TEMPERATURES]
    e_prop, u, acc, und = TR.accept_ex(case, 1.0, 1.0, TR.EX_W_EXTRA, inv_t, 0)
    assert und.sum() <= R.MAX_UNDECIDED
    got, u_d, e_prop_d, tok_after, e_after, ecc, elc, exc = run_accept(
        case, tokens, True, inv_t=dev(inv_t, torch.float64), rung=dev(case["rung"], torch.int32),
        e_extra=dev(case["e_extra"], torch.float64), w_extra=TR.EX_W_EXTRA, step=0)
    assert np.array_equal(e_prop_d.view(np.uint64), e_prop.view(np.uint64))
    assert np.array_equal(u_d.view(np.uint64), u.view(np.uint64))
    got = got.astype(bool)
    assert np.array_equal(got[~und], acc[~und])
    assert 0 < got.sum() < n and not got[case["tok"] < 0].any()
    want_tokens, want_e, want_x = tokens.copy(), case["e_cur"].copy(), np.full(n, -11.0)
    for c in np.nonzero(got)[0]:
        want_tokens[c, case["site"][c]] = case["tok"][c]
        want_e[c], want_x[c] = e_prop[c], case["e_extra"][c]
    assert np.array_equal(tok_after, want_tokens) and np.array_equal(e_after.view(np.uint64), want_e.view(np.uint64))
    assert np.array_equal(exc, want_x) and np.array_equal(ecc[got], case["e_contact"][got]) and (ecc[~got] == -7.0).all()
    # a rung outside the table is clamped
    wild = case["rung"].copy()
    wild[case["rung"] == 0], wild[case["rung"] == 2] = -5, 99
    again = run_accept(case, tokens, True, inv_t=dev(inv_t, torch.float64), rung=dev(wild, torch.int32),
                       e_extra=dev(case["e_extra"], torch.float64), w_extra=TR.EX_W_EXTRA, step=0)
    assert np.array_equal(again[0].astype(bool), got)


# ---- esmk_op_replica_swap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", TR.SWAP_KS)
def test_swap_rounds_against_the_reference(K):
    c = TR.swap_case(K)
    n = c["rung"].shape[0]
    for rnd in (0, 1):
        want, acc, u, und = TR.swap_round(c["rung"], c["e_cur"], c["inv_t"], c["ladder_ids"], TR.SWAP_SEED, rnd)
        rung_d = dev(c["rung"], torch.int32)
        acc_d, u_d = ops.replica_swap(rung_d, dev(c["e_cur"], torch.float64), dev(c["inv_t"], torch.float64), c["inv_t"],
                                      dev(c["ladder_ids"], torch.int32), seed=TR.SWAP_SEED, round=rnd)
        got, got_acc, got_u = rung_d.cpu().numpy(), acc_d.cpu().numpy(), u_d.cpu().numpy()
        assert und.sum() <= R.MAX_UNDECIDED
        assert np.array_equal(got_u.view(np.uint64), u.view(np.uint64)), (K, rnd)
        assert np.array_equal(got[~und], want[~und]) and np.array_equal(got_acc[~und], acc[~und]), (K, rnd)
        untouched = u < 0  # rung 0 in an odd round, the last rung where the round cannot pair it
        assert np.array_equal(got[untouched], c["rung"][untouched]) and not got_acc[untouched].any()
        assert np.array_equal(np.sort(got.reshape(-1, K), axis=1), np.tile(np.arange(K), (n // K, 1)))  # still permutations
        first = c["rung"] == 0
        last = c["rung"] == K - 1
        if rnd == 1:
            assert untouched[first].all()
        if (K - 1) % 2 == rnd % 2:
            assert untouched[last].all()
        if K == 1:
            assert np.array_equal(got, c["rung"]) and untouched.all()
        elif K >= 3 or rnd == 0:
            assert 0 < got_acc.sum() < (~untouched).sum() and not np.array_equal(got, c["rung"])
        if K % 2 == 1:  # an odd K: exactly one rung per ladder sits out, in either round
            assert untouched.reshape(-1, K).sum(axis=1).tolist() == [1] * (n // K)
