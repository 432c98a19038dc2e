"""``design`` / ``design_energy`` with a ``DistogramTarget``: lm-design's ``dist_cce_pos`` term (esmk_forward_rows_pair +
esmk_op_distogram_energy) in the slot of the contact term.  A recorded run is replayed step by step as tests/test_design_gpu.py
replays its runs — proposals are the reference's (tests/_design_ref.py), the proposal's structure energy is ``design_energy`` of
that sequence alone bit for bit, decisions follow the reference's rule with its UNDECIDED_MARGIN and MAX_UNDECIDED —, the
structure term is the fp64 restatement (tests/_pair_head_ref.py) of the model's own pair logits, a chain alone equals the chain
in a batch, and a run with a contact target still returns the bytes of tests/golden/design_defaults_parent.npz after a
distogram run has used the same engine."""
import os

import numpy as np
import pytest
import torch

import _pair_head_ref as PR
from esm_amd import DistogramTarget, PairHead
from test_design_gpu import L, SEED, chains, esm2_model, replay, side, target_for

D = __import__("importlib").import_module("esm_amd.design")
pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "design_defaults_parent.npz")


def distogram_target(model, T, seed=6, scale=8.0, **kw):
    """A head of lm-design's shape on the model's channels (weights wide enough that one substitution moves the term) and random
    target bins with some ignored pairs; about a third of the pairs are contacts (bin <= 5)."""
    S = side(model, T)
    C = model.num_layers * model.attention_heads
    g = torch.Generator().manual_seed(seed)
    state = {"conv1.weight": torch.randn(36, C, 1, 1, generator=g) * scale, "conv1.bias": torch.randn(36, generator=g),
             "conv2.weight": torch.randn(26, C, 1, 1, generator=g) * scale, "conv2.bias": torch.randn(26, generator=g)}
    head = PairHead.from_linear_projection({"model": state}, model)
    bins = torch.randint(0, 18, (S, S), generator=g).to(torch.uint8)
    bins[torch.rand(S, S, generator=g) < 0.1] = 255
    return DistogramTarget(bins, head, **kw)


def test_design_energy_is_the_restatement_of_the_pair_logits():
    model = esm2_model(2)
    toks = chains(model, 3, 70)
    for min_sep, temp in ((0, 1.0), (6, 0.7)):
        target = distogram_target(model, 70, temperature=temp)
        out = model.design_energy(toks, target, min_sep=min_sep)
        assert tuple(out) == ("energy", "e_contact", "e_lm")
        logits = model.pair_logits(toks, target.head)["dist"]
        counted = torch.where(target.bins <= 5, target.bins, torch.full_like(target.bins, 255))
        assert torch.equal(counted, target.bins)  # only the target's contacts count (dist_cce_pos)
        ref, cnt = PR.distogram_energy_ref(logits, target.bins, min_sep, 1.0 / temp)
        assert cnt > 0 and ((out["e_contact"] - ref).abs() <= 1e-12 * ref.abs()).all()
        assert torch.equal(out["energy"], 1.0 * out["e_contact"] + 1.0 * out["e_lm"])
    # the LM term is the one of a contact target: the same rows through the same head
    with_contacts = model.design_energy(toks, target_for(model, 70))
    assert torch.equal(with_contacts["e_lm"], out["e_lm"])
    # a sequence alone carries the bits it has in the batch
    alone = model.design_energy(toks[1:2], target, min_sep=6)
    assert all(torch.equal(alone[k][0], out[k][1]) for k in out)


@pytest.mark.parametrize("name,kw", [("uniform", dict(temperature=0.05, min_sep=0)),
                                     ("lm", dict(proposal="lm", proposal_temperature=4.0, temperature=0.1)),
                                     ("no-lm-term", dict(w_lm=0.0, temperature=0.02, min_sep=3))])
def test_replay_of_a_recorded_run(name, kw):
    model = esm2_model(2)
    B, T, steps = 4, 70, 16
    toks = chains(model, B, T)
    target = distogram_target(model, T)
    ids = [11, 3, 2 ** 31 - 1, 40]
    final, energy, traj = model.design(toks, target, steps, seed=SEED, chain_ids=ids, return_trajectory=True, **kw)
    energy_kw = {k: kw[k] for k in ("w_contact", "w_lm", "min_sep") if k in kw}
    run_kw = {k: kw[k] for k in ("temperature", "proposal", "proposal_temperature") if k in kw}
    replay(model, toks, target, final, energy, traj, steps, ids, **run_kw, **energy_kw)
    acc = traj["accepted"].sum().item()
    print(f"{name}: {acc} of {steps * B} proposals accepted")
    assert 0 < acc < steps * B, "a run that accepts everything or nothing checks little"


def test_a_chain_alone_equals_the_chain_inside_a_batch():
    model = esm2_model(8)
    B, T, steps = 12, 130, 5
    toks = chains(model, B, T, seed=33)
    target = distogram_target(model, T)
    ids = list(range(100, 100 + B))
    kw = dict(seed=SEED, return_trajectory=True, temperature=0.05)
    final, energy, traj = model.design(toks, target, steps, chain_ids=ids, **kw)
    for c in (0, 7, 11):
        f1, e1, t1 = model.design(toks[c: c + 1], target, steps, chain_ids=[ids[c]], **kw)
        assert torch.equal(f1[0], final[c]) and torch.equal(e1[0], energy[c])
        for k in D.TRAJECTORY_FIELDS:
            assert torch.equal(t1[k][:, 0], traj[k][:, c]), (k, c)
    # batches cut by max_bytes: the same run
    S = side(model, T)
    with torch.cuda.device(toks.device):
        need = model._engine_ready(toks.device).rows_pair_bytes(5, T, 5 * S) + 5 * S * S * 62 * 4
    cut = model.design(toks, target, steps, chain_ids=ids, max_bytes=need, **kw)
    assert torch.equal(cut[0], final) and torch.equal(cut[1], energy) and all(torch.equal(cut[2][k], traj[k]) for k in traj)


def test_a_contact_target_still_gives_the_recorded_bytes():
    """tests/test_design_tempering_gpu.py's check of the defaults, on an engine that has just run a distogram design."""
    model = esm2_model(2)
    toks = chains(model, 4, 70)
    model.design(toks, distogram_target(model, 70), 2, seed=SEED)
    out = model.design(toks, target_for(model, 70), 12, seed=SEED, chain_ids=[11, 3, 2 ** 31 - 1, 40], return_trajectory=True,
                       temperature=0.08)
    with np.load(GOLDEN) as z:
        for k, got in (("tokens", out[0]), ("energy", out[1])) + tuple((k, out[2][k]) for k in D.TRAJECTORY_FIELDS):
            a, b = got.cpu().numpy(), z["uniform_" + k]
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)), k


def test_refusals():
    model = esm2_model(2)
    toks = chains(model, 2, 70)
    target = distogram_target(model, 70)
    with pytest.raises(ValueError, match="min_sep must not be negative"):
        model.design_energy(toks, target, min_sep=-1)
    with pytest.raises(ValueError, match="bins of 68 residues but the chains have 38"):
        model.design_energy(chains(model, 2, 40), target)
    with pytest.raises(ValueError, match="no output 'distance'"):
        DistogramTarget(target.bins, target.head, output="distance")
    with pytest.raises(ValueError, match="bins hold 0 .. 17 or 255"):
        DistogramTarget(torch.full((4, 4), 18, dtype=torch.uint8), target.head)
    with pytest.raises(ValueError, match="temperature"):
        DistogramTarget(target.bins, target.head, temperature=0.0)
    with pytest.raises(ValueError, match="input channels"):
        model.design_energy(toks, distogram_target(esm2_model(8), 70))
