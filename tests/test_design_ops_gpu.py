"""The design kernels one launch at a time (esm_amd/csrc/design.hip through esm_amd/ops.py) against the numpy references of
tests/_design_ref.py: the proposal bit for bit, the contact term within the reordering bound of n fp64 additions and one ulp per
logarithm — and bit for bit between B = 1 and a place inside B = 5 —, the acceptance on synthetic energies with the decisions the
margin rule may count, and the Hastings term exactly."""
import numpy as np
import pytest
import torch

import _design_ref as R
from esm_amd import ops

pytestmark = pytest.mark.gpu
SEED = 0x5EED0DE5167
T, V = 70, 33
STANDARD = sum(1 << v for v in range(4, 24))


def dev(x, dtype):
    return torch.as_tensor(np.asarray(x)).to(dtype).cuda()


# ---- esmk_op_propose_mutations ------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 2, 63, 64, 65)


def chains():
    rng = np.random.default_rng(3)
    tokens = rng.integers(4, 24, size=(len(LENGTHS), T))
    tokens[:, 0], tokens[:, -1] = 0, 2
    tokens[3, :] = 30  # a chain whose current tokens are all outside the 20 residues
    lists = [sorted(rng.choice(np.arange(1, T - 1), size=n, replace=False).tolist()) for n in LENGTHS]
    return tokens, lists


@pytest.mark.parametrize("force_new", [True, False])
@pytest.mark.parametrize("mask", [STANDARD, 1 << 9, (1 << 9) | (1 << 30)], ids=["standard", "one-bit", "two-bits"])
def test_proposals_are_the_reference_bit_for_bit(force_new, mask):
    tokens, lists = chains()
    tokens[4, :] = 9  # with the one-bit mask: the only candidate is the current token
    ids = [7, 0, 2 ** 31 - 1, 12, 5, 1000003]
    off = np.cumsum([0] + [len(ps) for ps in lists])
    tok_d, off_d = dev(tokens, torch.int64), dev(off, torch.int32)
    pos_d, ids_d = dev([p for ps in lists for p in ps], torch.int32), dev(ids, torch.int32)
    for step in (0, 1, 5, 2 ** 31 - 1):
        site, old, tok = (t.cpu().tolist() for t in ops.propose_mutations(tok_d, off_d, pos_d, ids_d, mask, force_new, SEED, step))
        for c, ps in enumerate(lists):
            want = R.proposal(SEED, ids[c], step, ps, tokens[c], mask, force_new)
            assert (site[c], old[c], tok[c]) == want, (c, step)
        assert (site[0], old[0], tok[0]) == (-1, -1, -1)
        assert old[3] == 30 and (mask >> tok[3]) & 1  # a current token outside the candidates takes nothing away from them
        if mask == 1 << 9:  # chain 4 holds nothing but token 9: with force_new there is no candidate left
            assert tok[4] == (-1 if force_new else 9) and old[4] == 9
    # slots: the same chains read from another row order
    perm = [5, 4, 3, 2, 1, 0]
    shuffled = dev(tokens[perm], torch.int64)
    slots = dev(np.argsort(perm), torch.int32)
    a = ops.propose_mutations(tok_d, off_d, pos_d, ids_d, mask, force_new, SEED, 3)
    b = ops.propose_mutations(shuffled, off_d, pos_d, ids_d, mask, force_new, SEED, 3, slots=slots)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_an_empty_batch_of_lists_proposes_nothing():
    tokens, _ = chains()
    zeros = torch.zeros((len(LENGTHS) + 1,), dtype=torch.int32).cuda()
    site, old, tok = ops.propose_mutations(dev(tokens, torch.int64), zeros, torch.zeros((0,), dtype=torch.int32).cuda(),
                                           dev(range(len(LENGTHS)), torch.int32), STANDARD, True, SEED, 0)
    assert site.tolist() == old.tolist() == tok.tolist() == [-1] * len(LENGTHS)


# ---- esmk_op_contact_energy -----------------------------------------------------------------------------------------------------
def maps(S, B=5):
    rng = np.random.default_rng(100 + S)
    p = rng.uniform(0.0, 1.0, size=(B, S, S)).astype(np.float32)
    p[:, ::3, ::5] = 0.0  # the clamp, both ends
    p[:, 1::4, 2::3] = 1.0
    return p


def targets(S):
    rng = np.random.default_rng(200 + S)
    return {"all-ignore": np.full((S, S), 2, dtype=np.uint8), "all-contact": np.ones((S, S), dtype=np.uint8),
            "mixed": rng.choice(np.array([0, 1, 2], dtype=np.uint8), size=(S, S), p=[0.6, 0.3, 0.1])}


@pytest.mark.parametrize("S", [1, 7, 64, 130])
def test_contact_energy_against_fp64_and_across_batches(S):
    p = maps(S)
    p_d = dev(p, torch.float32)
    for name, target in targets(S).items():
        t_d = dev(target, torch.uint8)
        for min_sep in (1, 6, S, S + 3):
            for kind in ("pos", "bce"):
                energy, count = ops.contact_energy(p_d, t_d, min_sep, kind)
                got, cnt = energy.cpu().tolist(), count.cpu().tolist()
                for b in range(p.shape[0]):
                    want, n, bound = R.contact_energy(p[b], target, min_sep, kind)
                    assert cnt[b] == n, (name, min_sep, kind, b)
                    assert abs(got[b] - want) <= bound, (name, min_sep, kind, b, got[b], want, bound)
                    if n == 0:
                        assert got[b] == 0.0
                if min_sep >= S or name == "all-ignore":
                    assert cnt == [0] * p.shape[0]
                # the same chain alone and inside the batch of five: the same bits
                alone, alone_count = ops.contact_energy(p_d[3:4].contiguous(), t_d, min_sep, kind)
                assert torch.equal(alone, energy[3:4]) and torch.equal(alone_count, count[3:4])
    full = targets(S)["all-contact"]
    n_pairs = S * (S - 1) // 2
    assert ops.contact_energy(p_d, dev(full, torch.uint8), 1, "bce")[1].tolist() == [n_pairs] * 5


# ---- esmk_op_mh_accept ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_hastings", [True, False], ids=["hastings", "null"])
@pytest.mark.parametrize("weights", R.ACCEPT_WEIGHTS)
def test_acceptance_against_the_reference(weights, with_hastings):
    wc, wl = weights
    case = R.accept_case(with_hastings=with_hastings)
    n = case["tok"].shape[0]
    rng = np.random.default_rng(9)
    tokens = rng.integers(4, 24, size=(n, T))
    for step, temperature in enumerate(R.ACCEPT_TEMPERATURES):
        e_prop, u, acc, und = R.accept_reference(case, wc, wl, temperature, step)
        assert und.sum() <= R.MAX_UNDECIDED
        tok_d = dev(tokens, torch.int64)
        e_cur = dev(case["e_cur"], torch.float64)
        ecc, elc = torch.full((n,), -7.0, dtype=torch.float64).cuda(), torch.full((n,), -9.0, dtype=torch.float64).cuda()
        accepted, u_d, e_prop_d = ops.mh_accept(
            tok_d, dev(case["site"], torch.int32), dev(case["tok"], torch.int32), dev(case["chain"], torch.int32), e_cur,
            e_contact=dev(case["e_contact"], torch.float64) if wc != 0 else None,
            lp_sum=dev(case["lp_sum"], torch.float64) if wl != 0 else None, n_res=dev(case["n_res"], torch.int32),
            hastings=dev(case["hastings"], torch.float64) if with_hastings else None, w_contact=wc, w_lm=wl,
            inv_temperature=1.0 / temperature if temperature > 0 else float("inf"), seed=R.ACCEPT_SEED, step=step,
            e_contact_cur=ecc, e_lm_cur=elc)
        assert np.array_equal(e_prop_d.cpu().numpy().view(np.uint64), e_prop.view(np.uint64))
        assert np.array_equal(u_d.cpu().numpy().view(np.uint64), u.view(np.uint64))
        got = accepted.cpu().numpy().astype(bool)
        assert np.array_equal(got[~und], acc[~und]), (weights, temperature)
        assert not got[case["tok"] < 0].any()
        want_tokens = tokens.copy()
        want_e, want_ec, want_el = case["e_cur"].copy(), np.full(n, -7.0), np.full(n, -9.0)
        for c in np.nonzero(got)[0]:
            want_tokens[c, case["site"][c]] = case["tok"][c]
            want_e[c] = e_prop[c]
            want_ec[c] = case["e_contact"][c] if wc != 0 else 0.0
            want_el[c] = R.combine(0.0, 0.0, 1.0, case["lp_sum"][c], case["n_res"][c])[1] if wl != 0 else 0.0
        assert np.array_equal(tok_d.cpu().numpy(), want_tokens)  # a rejected chain, and tok = -1, write nothing
        assert np.array_equal(e_cur.cpu().numpy().view(np.uint64), want_e.view(np.uint64))
        assert np.array_equal(ecc.cpu().numpy(), want_ec) and np.array_equal(elc.cpu().numpy().view(np.uint64), want_el.view(np.uint64))
        assert 0 < got.sum() < n


def test_acceptance_through_slots():
    case = R.accept_case(n=8, with_hastings=False)
    tokens = np.full((8, T), 5)
    slots = np.array([7, 6, 5, 4, 3, 2, 1, 0], dtype=np.int32)
    tok_d = dev(tokens, torch.int64)
    acc, _, _ = ops.mh_accept(tok_d, dev(case["site"], torch.int32), dev(case["tok"], torch.int32), dev(case["chain"], torch.int32),
                              dev(case["e_cur"], torch.float64), e_contact=dev(case["e_contact"], torch.float64),
                              lp_sum=dev(case["lp_sum"], torch.float64), n_res=dev(case["n_res"], torch.int32),
                              inv_temperature=float("inf"), seed=1, step=0, slots=dev(slots, torch.int32))
    want = tokens.copy()
    for c in np.nonzero(acc.cpu().numpy())[0]:
        want[slots[c], case["site"][c]] = case["tok"][c]
    assert acc.sum().item() > 0 and np.array_equal(tok_d.cpu().numpy(), want)


# ---- esmk_op_hastings_rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inv_t", [1.0, 0.7, 3.0])
def test_hastings_rows_are_exact(inv_t):
    rng = np.random.default_rng(5)
    n = 300
    lp = (-rng.uniform(0.0, 12.0, size=(n, V))).astype(np.float32)
    old = rng.integers(0, V, n).astype(np.int32)
    new = rng.integers(0, V, n).astype(np.int32)
    old[::17], new[5::19] = -1, V  # nothing proposed / out of range: 0
    new[3::23] = old[3::23]
    got = ops.hastings_rows(dev(lp, torch.float32), dev(old, torch.int32), dev(new, torch.int32), inv_t).cpu().numpy()
    ok = (old >= 0) & (old < V) & (new >= 0) & (new < V)
    a = lp[np.arange(n), np.clip(old, 0, V - 1)].astype(np.float64)
    b = lp[np.arange(n), np.clip(new, 0, V - 1)].astype(np.float64)
    want = np.where(ok, np.float64(np.float32(inv_t)) * (a - b), 0.0)
    assert np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64)) and (got[~ok] == 0).all() and (got[3::23][ok[3::23]] == 0).all()
