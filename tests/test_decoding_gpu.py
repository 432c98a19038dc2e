"""Confidence-ordered unmasking and filtered draws through the model (esm_amd/sampling.py).  A recorded run of
``inpaint(order=...)`` is replayed from its own recorded states: the state before every step goes through the existing
``masked_joint`` with the positions still masked, and every committed draw's recorded row must be masked_joint's bit for bit,
every score within 4 fp32 ulp of the fp64 score of its row, the committed positions of every chain and step EXACTLY the best
``per_step`` of the recorded fp32 scores under the kernel's tie rule (so selection has no undecided case), every token the
reference draw from its row, kept set and uniform on the decided draws (at most 0.5 % undecided), every uniform the Philox
number at (chain, step, 1, position).  The synthetic models, the batch and the seed are those of tests/test_sampling_gpu.py."""
import numpy as np
import pytest
import torch

import _decoding_ref as D
import _sampling_ref as R
import test_sampling_gpu as G  # models, batch and seed of the plain sampler's test
from esm_amd import sampling

pytestmark = pytest.mark.gpu
SEED, T = G.SEED, G.T
HOLES = [[1, 2, 3, 30, 68], [7, 39], list(range(1, 40)), [4]]  # the third chain is masked from end to end
KIND = {"confidence": D.SCORE_CONFIDENCE, "entropy": D.SCORE_NEG_ENTROPY}
ALL64 = 2 ** 64 - 1


def masked_start(model, toks, holes=HOLES):
    start = toks.clone()
    for b, ps in enumerate(holes):
        start[b, ps] = model.mask_idx
    return start


def host(traj):
    out = {k: v.cpu().numpy() for k, v in traj.items() if k != "scored"}
    out["scored"] = {k: v.cpu().numpy() for k, v in traj["scored"].items()}
    return out


def replay(model, start, final, traj, per_step, order, temperature=1.0, top_k=0, top_p=1.0, chain_ids=None, seed=SEED,
           allowed=None):
    """Checks one recorded ordered run against the references; returns (committed draws, undecided ones)."""
    B = start.shape[0]
    ids = list(range(B)) if chain_ids is None else list(chain_ids)
    mask = sampling.allowed_mask(model, allowed)
    inv_t = 1.0 / temperature if temperature > 0 else 0.0
    tr = host(traj)
    sc = tr["scored"]
    assert set(tr) == set(sampling.TRAJECTORY_FIELDS) | {"score", "kept", "scored"} and set(sc) == {"chain", "step", "pos", "score"}
    holes = [row.nonzero().view(-1).tolist() for row in start.eq(model.mask_idx)]
    n = sum(len(ps) for ps in holes)
    assert tr["token"].shape == (n,) and tr["logprobs"].shape == (n, model.alphabet_size) and tr["score"].dtype == np.float32
    n_steps = max((len(ps) + per_step - 1) // per_step for ps in holes)
    assert sc["score"].shape[0] == sum(max(len(ps) - s * per_step, 0) for ps in holes for s in range(n_steps))
    state = start.clone()
    states, sets, src = [], [], []
    row_of = {}  # (step, slot, position) -> row of masked_joint's output = index into ``scored``
    r = c = 0  # next scored row, next committed draw
    commits = []  # (slot, step, position) of every committed draw, in recorded order
    for s in range(n_steps):
        states.append(state.clone())
        first = len(commits)
        for b in range(B):
            left = state[b].eq(model.mask_idx).nonzero().view(-1).tolist()
            if not left:
                continue  # done: the chain has left the batch
            assert len(left) == len(holes[b]) - s * per_step
            # the step scored every position still masked, chain-major, ascending
            rows = slice(r, r + len(left))
            assert sc["chain"][rows].tolist() == [ids[b]] * len(left) and sc["step"][rows].tolist() == [s] * len(left)
            assert sc["pos"][rows].tolist() == left, (s, b)
            for j, p in enumerate(left):
                row_of[(s, b, p)] = r + j
            sets.append(left)
            src.append(s * B + b)
            # it committed exactly the best min(per_step, left) of the scores it recorded, best first
            k = min(per_step, len(left))
            best = [left[i - r] for i in D.best_first(sc["score"], r, r + len(left))[:k]]
            mine = slice(c, c + k)
            assert tr["chain"][mine].tolist() == [ids[b]] * k and tr["step"][mine].tolist() == [s] * k
            assert tr["pos"][mine].tolist() == best, (s, b, tr["pos"][mine].tolist(), best)
            for j, p in enumerate(best):
                assert np.array_equal(tr["score"][c + j: c + j + 1].view(np.uint32),
                                      sc["score"][row_of[(s, b, p)]: row_of[(s, b, p)] + 1].view(np.uint32))
                commits.append((b, s, p))
            r, c = r + len(left), c + k
        for i in range(first, len(commits)):  # the draws of a step see the state before the step
            b, _, p = commits[i]
            tok = int(tr["token"][i])
            assert (mask >> tok) & 1, i
            state[b, p] = tok
    assert r == sc["score"].shape[0] and c == n
    assert torch.equal(state, final.cpu()), "the final tokens are not the input plus the recorded draws"
    assert not bool((final == model.mask_idx).any())
    keep = start.ne(model.mask_idx)
    assert torch.equal(final.cpu()[keep], start[keep])
    # the uniforms: Philox at (chain, step, 1, position)
    want_u = R.uniform(seed, np.array([ids[b] for b, _, _ in commits]), np.array([s for _, s, _ in commits]),
                       np.array([p for _, _, p in commits]))
    assert np.array_equal(tr["u"].view(np.uint32), want_u.view(np.uint32))
    # one masked_joint call over the recorded states: every row the run scored
    _, _, lp = model.masked_joint(torch.cat(states), sets, src=src)
    lp = lp.cpu().numpy()
    assert lp.shape[0] == sc["score"].shape[0]
    for i in range(lp.shape[0]):
        want = D.score(lp[i], mask, inv_t, KIND[order])
        assert abs(float(sc["score"][i]) - want) <= R.logq_bound(want), (i, float(sc["score"][i]), want)
    undecided = 0
    for i, (b, s, p) in enumerate(commits):
        row = lp[row_of[(s, b, p)]]
        assert np.array_equal(row.view(np.uint32), tr["logprobs"][i].view(np.uint32)), f"draw {i}: the recorded row is not masked_joint's"
        tok, logq, kept, decided = D.draw_ex(row, tr["u"][i], mask, inv_t, top_k, top_p)
        if not decided:
            undecided += 1
            continue
        assert int(tr["kept"][i]) & ALL64 == kept, (i, bin(int(tr["kept"][i]) & ALL64), bin(kept))
        assert int(tr["token"][i]) == tok, (i, int(tr["token"][i]), tok)
        z = row[R.candidates(row.shape[0], kept)].astype(np.float64) * (float(np.float32(inv_t)) or 1.0)
        assert abs(float(tr["logq"][i]) - logq) <= R.logq_bound(np.log(np.exp(z - z.max()).sum())), i
    assert undecided <= R.UNDECIDED_CAP * n, undecided
    return n, undecided


# ---- the replay -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["confidence", "entropy"])
def test_ordered_inpaint_replays(order):
    model, toks = G.shared_model(), G.batch()
    start = masked_start(model, toks)
    final, traj = model.inpaint(start, per_step=2, top_p=0.9, order=order, seed=SEED, return_trajectory=True)
    assert final.is_cuda and final.dtype == torch.int64 and tuple(final.shape) == (4, T)
    n, undecided = replay(model, start, final, traj, 2, order, top_p=0.9)
    print(f"{order}: {n} committed draws, {traj['scored']['score'].numel()} rows scored, {undecided} undecided")
    assert n == 47 and traj["scored"]["score"].numel() == 9 + 2 + 400 + 1  # 5 + 3 + 1, 2, 39 + 37 + ... + 1, 1
    assert torch.equal(model.inpaint(start, per_step=2, top_p=0.9, order=order, seed=SEED), final)  # without the trajectory
    # the order is not the random one, and the two scores do not choose alike
    plain = model.inpaint(start, per_step=2, top_p=0.9, seed=SEED, return_trajectory=True)[1]
    assert not torch.equal(plain["pos"], traj["pos"])


def test_greedy_confidence_is_deterministic():
    model, toks = G.shared_model(), G.batch()
    start = masked_start(model, toks)
    final, traj = model.inpaint(start, per_step=1, temperature=0, order="confidence", seed=SEED, return_trajectory=True)
    replay(model, start, final, traj, 1, "confidence", temperature=0)
    assert bool((traj["logq"] == 0).all())
    other, traj2 = model.inpaint(start, per_step=1, temperature=0, order="confidence", seed=SEED + 99, return_trajectory=True)
    assert torch.equal(other, final)  # the seed does not matter: only u differs
    for name in traj:
        if name not in ("u", "scored"):
            assert torch.equal(traj[name], traj2[name]), name
    # every committed token is the argmax of its row over the candidates
    allowed = torch.tensor([(sampling.allowed_mask(model) >> v) & 1 == 1 for v in range(model.alphabet_size)]).cuda()
    assert torch.equal(traj["logprobs"].masked_fill(~allowed, float("-inf")).argmax(-1).to(torch.int32), traj["token"])


# ---- batch independence, seeds, defaults --------------------------------------------------------------------------------------
def test_a_chain_unmasks_the_same_alone_as_in_the_batch():
    model, toks = G.shared_model(), G.batch()
    start = masked_start(model, toks)
    kw = dict(per_step=2, top_p=0.9, top_k=8, temperature=0.8, order="confidence", seed=SEED, return_trajectory=True)
    final, traj = model.inpaint(start, **kw)
    alone, traj1 = model.inpaint(start[2:3], chain_ids=[2], **kw)
    assert torch.equal(alone[0], final[2])
    mine = traj["chain"] == 2
    assert int(mine.sum()) == 39 == traj1["token"].numel()
    for name in sampling.TRAJECTORY_FIELDS + ("score", "kept"):
        assert torch.equal(traj[name][mine], traj1[name]), name
    scored = traj["scored"]["chain"] == 2
    assert int(scored.sum()) == 400
    for name in ("chain", "step", "pos", "score"):
        assert torch.equal(traj["scored"][name][scored], traj1["scored"][name]), name
    # chain ids name the chain: without them the chain alone is chain 0 and draws something else
    assert not torch.equal(model.inpaint(start[2:3], **dict(kw, return_trajectory=False))[0], final[2])
    # the same seed twice: the same bits; another seed: other draws
    again, traj2 = model.inpaint(start, **kw)
    assert torch.equal(again, final)
    assert all(torch.equal(traj[k], traj2[k]) for k in traj if k != "scored")
    assert all(torch.equal(traj["scored"][k], traj2["scored"][k]) for k in traj["scored"])
    other, traj3 = model.inpaint(start, **dict(kw, seed=SEED + 1))
    assert not torch.equal(other, final) and not torch.equal(traj3["u"], traj["u"])


def test_defaults_are_the_plain_sampler_bit_for_bit():
    model, toks = G.shared_model(), G.batch()
    start = masked_start(model, toks)
    a, ta = model.inpaint(start, per_step=2, seed=SEED, return_trajectory=True)
    b, tb = model.inpaint(start, per_step=2, seed=SEED, return_trajectory=True, order="random", top_k=0, top_p=1.0)
    assert torch.equal(a, b) and set(ta) == set(tb) == set(sampling.TRAJECTORY_FIELDS)
    assert all(torch.equal(ta[k], tb[k]) for k in ta)
    assert torch.equal(model.inpaint(start), model.inpaint(start, order="random", top_k=0, top_p=1.0))
    g, tg = model.gibbs_sample(toks, 1, per_step=3, seed=SEED, return_trajectory=True)
    h, th = model.gibbs_sample(toks, 1, per_step=3, seed=SEED, return_trajectory=True, top_k=0, top_p=1.0, order="random")
    assert torch.equal(g, h) and set(tg) == set(th) == set(sampling.TRAJECTORY_FIELDS) and all(torch.equal(tg[k], th[k]) for k in tg)
    # a filter that keeps everything goes through the filtered kernel and still draws the same tokens
    i, ti = model.gibbs_sample(toks, 1, per_step=3, seed=SEED, return_trajectory=True, top_k=64)
    assert torch.equal(g, i) and all(torch.equal(tg[k], ti[k]) for k in tg) and "kept" in ti


def test_gibbs_top_k_commits_only_the_best_candidates():
    model, toks = G.shared_model(), G.batch()
    final, traj = model.gibbs_sample(toks, 1, per_step=3, top_k=3, temperature=1.5, force_new=True, seed=SEED, return_trajectory=True)
    mask = sampling.allowed_mask(model)
    tr = {k: v.cpu().numpy() for k, v in traj.items()}
    lists = G.residue_lists(toks, model)
    n = sum(len(ps) for ps in lists)
    assert tr["token"].shape == (n,) and tr["kept"].shape == (n,)
    state = toks.clone()
    seen = set()
    for i in range(n):
        b = int(tr["chain"][i])
        old = int(state[b, int(tr["pos"][i])])  # force_new: the token the draw replaces is no candidate
        cand = R.candidates(model.alphabet_size, mask, old)
        best = D.ranked(tr["logprobs"][i], cand)[:3]
        assert int(tr["token"][i]) in best, (i, int(tr["token"][i]), best)
        assert int(tr["kept"][i]) & ALL64 == sum(1 << v for v in best) == D.keep_set(tr["logprobs"][i], mask, 1 / 1.5, 3, 1.0, old)[0]
        seen.add(best.index(int(tr["token"][i])))
        if i + 1 == n or tr["step"][i + 1] != tr["step"][i]:  # the draws of a step see the state before the step
            for j in range(i, -1, -1):
                if tr["step"][j] != tr["step"][i]:
                    break
                state[int(tr["chain"][j]), int(tr["pos"][j])] = int(tr["token"][j])
    assert seen == {0, 1, 2}  # at temperature 1.5 the second and third candidates are drawn too
    assert torch.equal(state, final.cpu())


# ---- every model kind --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(G.KINDS))
def test_the_ordered_path_runs_on_every_model_kind(kind, monkeypatch):
    make, tok_kw, env = G.KINDS[kind]
    monkeypatch.delenv("ESM_AMD_LN_FOLD", raising=False)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    model = make()
    toks = G.batch(**tok_kw)
    start = toks.clone()
    start[0, 5:9] = model.mask_idx
    start[3, 2] = model.mask_idx
    final, traj = model.inpaint(start, per_step=3, top_k=10, order="confidence", seed=SEED, return_trajectory=True)
    if "fold" in kind:
        assert model.ln_fold_active() is (env["ESM_AMD_LN_FOLD"] == "1")
    assert replay(model, start, final, traj, 3, "confidence", top_k=10)[0] == 5
    assert traj["scored"]["score"].numel() == 4 + 1 + 1
