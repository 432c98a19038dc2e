"""Sampling through the model (esm_amd/sampling.py): a recorded trajectory is replayed step by step from the input tokens —
the state before every step, with that step's positions masked, goes through the existing ``masked_joint`` and must give the
recorded log-probability rows bit for bit; the recorded token must be the fp64 draw (tests/_sampling_ref.py) from those rows
and the recorded uniform on every decided draw; the recorded positions must be the reference shuffle.  Every step is checked
against its own recorded state, so an undecided draw cannot cascade.  Synthetic models of esm_amd/synth.py, L = 2, E = 128,
H = 2; B = 4 chains of lengths 70, 41, 41 and 9 at T = 70."""
import argparse
import functools

import numpy as np
import pytest
import torch

import _sampling_ref as R
import esm
from esm_amd import sampling
from esm_amd.synth import esm1_args, synth_esm1_state_dict, synth_esm1b_state_dict, synth_esm2_state_dict, synth_tokens

pytestmark = pytest.mark.gpu
PAD, L, T = 1, 2, 70
LENGTHS = (70, 41, 41, 9)
SEED = 0x5EED0123456789


def batch(cls=0, last=2):
    toks = synth_tokens(4, T - 2, seed=21)
    toks[:, 0] = cls
    for b, n in enumerate(LENGTHS):
        toks[b, n - 1] = last if last is not None else 9
        toks[b, n:] = PAD
    return toks


def esm2_model():
    model = esm.ESM2(L, 128, 2).eval()
    model.load_state_dict(synth_esm2_state_dict(L, 128, 2, seed=3))
    return model.cuda()


def esm1b_model():
    args = argparse.Namespace(arch="roberta_large", layers=L, embed_dim=128, ffn_embed_dim=512, attention_heads=2,
                              max_positions=1024, token_dropout=True, emb_layer_norm_before=True)
    model = esm.ProteinBertModel(args, esm.Alphabet.from_architecture("roberta_large")).eval()
    model.load_state_dict(synth_esm1b_state_dict(L, 128, 2, seed=5), strict=True)
    return model.cuda()


def esm1_model():
    model = esm.ProteinBertModel(esm1_args(L, 128, 2, final_bias=True, token_dropout=True),
                                 esm.Alphabet.from_architecture("protein_bert_base")).eval()
    model.load_state_dict(synth_esm1_state_dict(L, 128, 2, seed=7, final_bias=True), strict=True)
    return model.cuda()


@functools.lru_cache(maxsize=None)
def shared_model():
    return esm2_model()


def host(traj):
    return {k: v.cpu().numpy() for k, v in traj.items()}


def replay(model, toks, final, traj, lists, per_step, epochs, temperature=1.0, force_new=False, chain_ids=None, seed=SEED,
           allowed=None):
    """Checks one recorded run against the references; returns the number of undecided draws."""
    B = toks.shape[0]
    ids = list(range(B)) if chain_ids is None else list(chain_ids)
    mask = sampling.allowed_mask(model, allowed)
    inv_t = 1.0 / temperature if temperature > 0 else 0.0
    tr = host(traj)
    n = tr["token"].shape[0]
    assert n == epochs * sum(len(ps) for ps in lists)
    assert tr["logprobs"].shape == (n, model.alphabet_size) and tr["logprobs"].dtype == np.float32
    # the expected draws, in the order drawn: step-major, chain-major inside a step, the chain's shuffled order inside a chain
    want = []  # (slot, chain id, step word, index, position)
    n_steps = max((len(ps) + per_step - 1) // per_step for ps in lists)
    for e in range(epochs):
        perm = [R.shuffle(ps, seed, ids[b], e) for b, ps in enumerate(lists)]
        for s in range(n_steps):
            for b in range(B):
                for j, p in enumerate(perm[b][s * per_step: (s + 1) * per_step]):
                    want.append((b, ids[b], e * sampling.STEP_STRIDE + s, j, p))
    assert tr["chain"].tolist() == [w[1] for w in want]
    assert tr["step"].tolist() == [w[2] for w in want]
    assert tr["pos"].tolist() == [w[4] for w in want], "the recorded positions are not the reference shuffle"
    want_u = R.uniform(seed, np.array([w[1] for w in want]), np.array([w[2] for w in want]), np.array([w[3] for w in want]))
    assert np.array_equal(tr["u"].view(np.uint32), want_u.view(np.uint32))
    # the state before every step, from the input and the recorded tokens; one masked_joint call over all of them
    state = toks.clone()
    states, sets, src, rows_of, state_of = [], [], [], {}, {}
    r = 0
    while r < n:
        r1 = r
        while r1 < n and want[r1][2] == want[r][2]:
            r1 += 1
        k = len(states)
        states.append(state.clone())
        for b in sorted({w[0] for w in want[r:r1]}):
            mine = [i for i in range(r, r1) if want[i][0] == b]
            order = sorted(mine, key=lambda i: want[i][4])  # masked_joint gives a set's rows in ascending position
            for i in order:
                rows_of[i] = sum(len(x) for x in sets) + order.index(i)
            sets.append([want[i][4] for i in order])
            src.append(k * B + b)
        for i in range(r, r1):
            state_of[i] = k
            old = int(state[want[i][0], want[i][4]])
            tok = int(tr["token"][i])
            if force_new:
                assert tok != old, i
            assert (mask >> tok) & 1, i
            state[want[i][0], want[i][4]] = tok
        r = r1
    assert torch.equal(state, final.cpu()), "the final tokens are not the input plus the recorded draws"
    _, _, lp = model.masked_joint(torch.cat(states), sets, src=src)
    lp = lp.cpu().numpy()
    undecided = 0
    for i in range(n):
        row = lp[rows_of[i]]
        assert np.array_equal(row.view(np.uint32), tr["logprobs"][i].view(np.uint32)), f"draw {i}: the recorded row is not masked_joint's"
        ex = -1
        if force_new:  # the token the draw replaced: what the state held before the step
            ex = int(states[state_of[i]][want[i][0], want[i][4]])
        tok, _, decided = R.draw(row, tr["u"][i], mask, inv_t, ex)
        if not decided:
            undecided += 1
            continue
        assert int(tr["token"][i]) == tok, (i, int(tr["token"][i]), tok)
    assert undecided <= R.UNDECIDED_CAP * n, undecided
    return undecided


def residue_lists(toks, model):
    return sampling._residue_positions(model, toks.clone())


# ---- the replay -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_step", [1, 3])
def test_gibbs_trajectory_replays(per_step):
    model, toks = shared_model(), batch()
    final, traj = model.gibbs_sample(toks, 2, per_step=per_step, seed=SEED, return_trajectory=True)
    assert final.is_cuda and final.dtype == torch.int64 and tuple(final.shape) == (4, T)
    lists = residue_lists(toks, model)
    assert [len(ps) for ps in lists] == [68, 39, 39, 7]
    replay(model, toks, final, traj, lists, per_step, epochs=2)
    # only residues changed: <cls>, <eos> and <pad> are where they were
    keep = torch.ones_like(toks, dtype=torch.bool)
    for b, ps in enumerate(lists):
        keep[b, ps] = False
    assert torch.equal(final.cpu()[keep], toks[keep]) and not torch.equal(final.cpu(), toks)
    assert torch.equal(model.gibbs_sample(toks, 2, per_step=per_step, seed=SEED), final)  # without the trajectory: the same


def test_positions_temperature_and_force_new():
    model, toks = shared_model(), batch()
    lists = [[3, 9, 10, 40, 68], [1, 39], [], [5, 6, 7]]
    final, traj = model.gibbs_sample(toks, 3, per_step=2, positions=lists, temperature=0.7, force_new=True, seed=SEED + 1,
                                     allowed="ACDEFGHIKL", return_trajectory=True)
    replay(model, toks, final, traj, lists, 2, epochs=3, temperature=0.7, force_new=True, seed=SEED + 1, allowed="ACDEFGHIKL")
    changed = (final.cpu() != toks).nonzero().tolist()
    assert all(p in lists[b] for b, p in changed) and torch.equal(final[2].cpu(), toks[2])
    assert torch.equal(model.gibbs_sample(toks, 0), toks.cuda())  # no sweep: the input


def test_inpaint_fills_the_masks_and_nothing_else():
    model, toks = shared_model(), batch()
    mask_idx = model.mask_idx
    holes = [[1, 2, 3, 30, 68], [7, 39], [], [4]]
    start = toks.clone()
    for b, ps in enumerate(holes):
        start[b, ps] = mask_idx
    final, traj = model.inpaint(start, per_step=2, seed=SEED, return_trajectory=True)
    assert not bool((final == mask_idx).any())
    keep = start.ne(mask_idx)
    assert torch.equal(final.cpu()[keep], start[keep])
    replay(model, start, final, traj, holes, 2, epochs=1)
    # positions not yet visited are still <mask> in the state a draw sees: the last step sees everything else committed
    assert torch.equal(model.inpaint(start, per_step=2, seed=SEED), final)


def test_greedy_whole_list_is_the_argmax_of_masked_joint():
    model, toks = shared_model(), batch()
    lists = [[3, 9, 10, 40, 68], [1, 39], [12], [5, 6, 7]]
    final = model.gibbs_sample(toks, 1, per_step=5, positions=lists, temperature=0)
    _, pos, lp = model.masked_joint(toks, lists, src=[0, 1, 2, 3])
    allowed = torch.tensor([(sampling.allowed_mask(model) >> v) & 1 == 1 for v in range(model.alphabet_size)]).cuda()
    best = lp.masked_fill(~allowed, float("-inf")).argmax(-1)
    want = toks.clone().cuda()
    want[torch.tensor([b for b, ps in enumerate(lists) for _ in ps]).cuda(), pos] = best
    assert torch.equal(final, want)


# ---- batch independence, seeds ----------------------------------------------------------------------------------------------
def test_a_chain_runs_the_same_alone_as_in_the_batch():
    model, toks = shared_model(), batch()
    final, traj = model.gibbs_sample(toks, 2, per_step=3, seed=SEED, return_trajectory=True)
    alone, traj1 = model.gibbs_sample(toks[2:3], 2, per_step=3, seed=SEED, chain_ids=[2], return_trajectory=True)
    assert torch.equal(alone[0], final[2])
    mine = traj["chain"] == 2
    assert int(mine.sum()) == 2 * 39 == traj1["token"].numel()
    for name in sampling.TRAJECTORY_FIELDS:
        assert torch.equal(traj[name][mine], traj1[name]), name
    # chain ids name the chain: without them the chain alone is chain 0 and draws something else
    assert not torch.equal(model.gibbs_sample(toks[2:3], 2, per_step=3, seed=SEED)[0], final[2])
    # the same seed twice: the same bits; another seed: other draws
    again, traj2 = model.gibbs_sample(toks, 2, per_step=3, seed=SEED, return_trajectory=True)
    assert torch.equal(again, final) and all(torch.equal(traj[k], traj2[k]) for k in traj)
    other, traj3 = model.gibbs_sample(toks, 2, per_step=3, seed=SEED + 1, return_trajectory=True)
    assert not torch.equal(other, final) and not torch.equal(traj3["u"], traj["u"]) and not torch.equal(traj3["pos"], traj["pos"])


# ---- every model kind --------------------------------------------------------------------------------------------------------
KINDS = {
    "esm2-nofold": (esm2_model, dict(), dict(ESM_AMD_LN_FOLD="0")),
    "esm2-fold": (esm2_model, dict(), dict(ESM_AMD_LN_FOLD="1")),
    "esm1b": (esm1b_model, dict(), dict()),
    "esm1": (esm1_model, dict(cls=32, last=None), dict()),
}


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_path_runs_on_every_model_kind(kind, monkeypatch):
    make, tok_kw, env = KINDS[kind]
    monkeypatch.delenv("ESM_AMD_LN_FOLD", raising=False)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    model = make()
    toks = batch(**tok_kw)
    final, traj = model.gibbs_sample(toks, 1, per_step=4, seed=SEED, return_trajectory=True)
    if "fold" in kind:
        assert model.ln_fold_active() is (env["ESM_AMD_LN_FOLD"] == "1")
    lists = residue_lists(toks, model)
    replay(model, toks, final, traj, lists, 4, epochs=1)
    start = toks.clone()
    start[0, 5:9] = model.mask_idx
    start[3, 2] = model.mask_idx
    filled = model.inpaint(start, per_step=3, seed=SEED)
    assert not bool((filled == model.mask_idx).any()) and torch.equal(filled.cpu()[start.ne(model.mask_idx)],
                                                                      start[start.ne(model.mask_idx)])
