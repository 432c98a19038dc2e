"""Design with the n-gram term and with replica exchange through the model (esm_amd/design.py).  With the new keywords at their
defaults ``design`` returns the bits the code before them returned (tests/golden/design_defaults_parent.npz, recorded from that
commit by the same call).  A recorded replica run is replayed step by step from its own recorded state: proposals are the
reference's (tests/_design_ref.py), the proposal's energy is ``design_energy`` of the proposed sequence alone bit for bit, the
acceptance is the reference's at the chain's recorded rung, the swaps are the reference's (tests/_tempering_ref.py) from the
recorded energies, and the final energy is ``design_energy`` of the final tokens.  A ladder alone equals the same ladder inside a
batch of six; ladders that never swap equal independent constant-temperature calls.  Synthetic models of esm_amd/synth.py, L = 2."""
import os

import numpy as np
import pytest
import torch

import _design_ref as R
import _sampling_ref as SR
import _tempering_ref as TR
from esm_amd import sampling
from esm_amd.ngram import Background
from test_design_gpu import L, SEED, chains, esm2_model, target_for

D = __import__("importlib").import_module("esm_amd.design")
pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "design_defaults_parent.npz")
LADDER = [0.04, 0.08, 0.16, 0.32]  # around the scale of the energy differences on these synthetic weights (test_design_gpu.py)


def background():
    """A background counted from sequences with a skewed composition, so that the term tells sequences apart."""
    rng = np.random.default_rng(12)
    letters = np.array(list(TR.STANDARD))
    p = rng.gamma(1.0, size=20)
    seqs = ["".join(rng.choice(letters, size=120, p=p / p.sum())) for _ in range(40)]
    return Background.from_sequences(seqs, orders=(1, 2, 3))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


# ---- the defaults ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("uniform", dict(temperature=0.08)),
                                     ("lm", dict(proposal="lm", proposal_temperature=4.0, temperature=0.1))])
def test_the_defaults_return_what_the_code_before_them_returned(name, kw):
    """The fixture holds tokens, energy and trajectory of exactly this call on the parent commit."""
    model = esm2_model(2)
    toks, target = chains(model, 4, 70), target_for(model, 70)
    out = model.design(toks, target, 12, seed=SEED, chain_ids=[11, 3, 2 ** 31 - 1, 40], return_trajectory=True, **kw)
    assert len(out) == 3 and tuple(out[2]) == D.TRAJECTORY_FIELDS
    with np.load(GOLDEN) as z:
        assert same_bits(out[0].cpu().numpy(), z[name + "_tokens"]) and same_bits(out[1].cpu().numpy(), z[name + "_energy"])
        for k in D.TRAJECTORY_FIELDS:
            assert same_bits(out[2][k].cpu().numpy(), z[name + "_" + k]), k
    # ... and w_ngram = 0 with a table, or a term weighted 0, is that call too
    again = model.design(toks, target, 12, seed=SEED, chain_ids=[11, 3, 2 ** 31 - 1, 40], return_trajectory=True, w_ngram=0.0,
                         ngram=background(), replicas=None, swap_every=3, **kw)
    assert len(again) == 3 and torch.equal(again[0], out[0]) and torch.equal(again[1], out[1])
    assert tuple(again[2]) == D.TRAJECTORY_FIELDS and all(torch.equal(again[2][k], out[2][k]) for k in out[2])
    assert tuple(model.design_energy(toks, target)) == ("energy", "e_contact", "e_lm")


# ---- the replay of a replica run ------------------------------------------------------------------------------------------------
def replay(model, toks, target, out, steps, ids, K, swap_every, ladder, lm, inv_t_prop, energy_kw):
    final, energy, rung_final, traj = out
    B = toks.shape[0]
    mask = sampling.allowed_mask(model)
    inv_t = D.ladder_inverse_temperatures(ladder, steps, K)
    tr = {k: v.cpu().numpy() for k, v in traj.items()}
    assert tuple(traj) == D.TRAJECTORY_FIELDS + D.NGRAM_FIELDS + D.REPLICA_FIELDS
    for k in tr:
        assert tr[k].shape == (steps, B), k
    assert tr["rung"].dtype == np.int32 and tr["swapped"].dtype == np.uint8 and tr["swap_u"].dtype == np.float64
    lists = sampling._position_lists(model, toks.cpu(), None)
    state = toks.cpu().clone()
    first = model.design_energy(toks, target, **energy_kw)
    assert same_bits(tr["e_cur"][0], first["energy"].cpu().numpy())
    assert tr["rung"][0].tolist() == [b % K for b in range(B)]
    ladder_ids = [ids[l * K] for l in range(B // K)]
    undecided = 0
    for s in range(steps):
        for c in range(B):
            site, old, tok = R.proposal(SEED, ids[c], s, lists[c], state[c].tolist(), mask, not lm)
            assert (tr["site"][s, c], tr["old"][s, c]) == (site, old), (s, c)
            new = int(tr["new"][s, c])
            if not lm:
                assert new == tok and tr["hastings"][s, c] == 0.0, (s, c)
            else:
                _, _, row = model.masked_joint(state[c: c + 1].cuda(), [[site]])
                row = row[0].cpu().numpy()
                want, _, decided = SR.draw(row, SR.uniform(SEED, ids[c], s, site), mask, inv_t_prop)
                assert not decided or new == want, (s, c)
                assert tr["hastings"][s, c] == np.float64(np.float32(inv_t_prop)) * (np.float64(row[old]) - np.float64(row[new])), (s, c)
            proposed = state[c: c + 1].clone()
            proposed[0, site] = new
            alone = model.design_energy(proposed.cuda(), target, **energy_kw)
            for field, key in (("e_prop", "energy"), ("e_contact", "e_contact"), ("e_lm", "e_lm"), ("e_ngram", "e_ngram")):
                assert tr[field][s, c] == alone[key].item(), (field, s, c, tr[field][s, c], alone[key].item())
            assert tr["u"][s, c] == R.accept_uniform(SEED, ids[c], s)
            k = int(tr["rung"][s, c])
            acc, und = R.accept(tr["e_prop"][s, c], tr["e_cur"][s, c], inv_t[s, k], tr["hastings"][s, c], tr["u"][s, c], new)
            undecided += int(und)
            got = bool(tr["accepted"][s, c])
            assert und or got == acc, (s, c)
            if got:
                state[c, site] = new
        after = tr["e_cur"][s + 1] if s + 1 < steps else energy.cpu().numpy()
        assert same_bits(after, np.where(tr["accepted"][s].astype(bool), tr["e_prop"][s], tr["e_cur"][s])), s
        rung_after = tr["rung"][s + 1] if s + 1 < steps else rung_final.cpu().numpy()
        if swap_every > 0 and (s + 1) % swap_every == 0:
            rnd = (s + 1) // swap_every - 1
            want, acc, u, und = TR.swap_round(tr["rung"][s], after, inv_t[s], ladder_ids, SEED, rnd)
            undecided += int(und.sum()) // 2
            assert same_bits(tr["swap_u"][s], u), s
            assert np.array_equal(rung_after[~und], want[~und]) and np.array_equal(tr["swapped"][s][~und], acc[~und]), s
        else:
            assert np.array_equal(rung_after, tr["rung"][s]) and not tr["swapped"][s].any() and (tr["swap_u"][s] == -1.0).all(), s
    assert torch.equal(final.cpu(), state)
    last = model.design_energy(final, target, **energy_kw)["energy"]
    assert torch.equal(last, energy), "the final energy is not design_energy of the final tokens"
    assert undecided <= R.MAX_UNDECIDED


@pytest.mark.parametrize("proposal", ["uniform", "lm"])
def test_replay_of_a_recorded_replica_run(proposal):
    model = esm2_model(2)
    K, B, T, steps, swap_every = 4, 8, 70, 12, 2
    toks, target = chains(model, B, T), target_for(model, T)
    ids = [11, 3, 2 ** 31 - 1, 40, 7, 8, 100, 5]
    energy_kw = dict(w_ngram=0.5, ngram=background())
    lm = proposal == "lm"
    run_kw = dict(proposal="lm", proposal_temperature=4.0) if lm else {}
    out = model.design(toks, target, steps, seed=SEED, chain_ids=ids, return_trajectory=True, replicas=K, swap_every=swap_every,
                       temperature=LADDER, **run_kw, **energy_kw)
    assert len(out) == 4 and out[2].dtype == torch.int32
    replay(model, toks, target, out, steps, ids, K, swap_every, LADDER, lm, 0.25 if lm else 1.0, energy_kw)
    traj = out[3]
    attempted = (traj["swap_u"] >= 0).sum().item()
    assert attempted == (steps // swap_every // 2) * (B // K) * 4 + (steps // swap_every // 2) * (B // K) * 2  # rounds 0, 2, 4: 2 pairs; 1, 3, 5: 1
    print("accepted moves", traj["accepted"].sum().item(), "swapped chains", traj["swapped"].sum().item(), "of", attempted)
    assert 0 < traj["accepted"].sum().item() < steps * B and 0 < traj["swapped"].sum().item()
    assert sorted(out[2].view(-1, K)[0].tolist()) == list(range(K))
    plain = model.design(toks, target, steps, seed=SEED, chain_ids=ids, replicas=K, swap_every=swap_every, temperature=LADDER, **run_kw,
                         **energy_kw)
    assert len(plain) == 3 and all(torch.equal(a, b) for a, b in zip(plain, out[:3]))
    # `steps` ladders, all the same, are that one ladder
    listed = model.design(toks, target, steps, seed=SEED, chain_ids=ids, replicas=K, swap_every=swap_every, temperature=[LADDER] * steps,
                          **run_kw, **energy_kw)
    assert all(torch.equal(a, b) for a, b in zip(listed, out[:3]))


# ---- ladders and batches --------------------------------------------------------------------------------------------------------
def test_a_ladder_alone_equals_the_ladder_inside_a_batch_of_six():
    model = esm2_model(2)
    K, B, T, steps = 4, 24, 70, 6
    toks, target = chains(model, B, T, seed=33), target_for(model, T)
    ids = list(range(100, 100 + B))
    kw = dict(seed=SEED, return_trajectory=True, replicas=K, temperature=LADDER, w_ngram=0.5, ngram=background())
    final, energy, rung, traj = model.design(toks, target, steps, chain_ids=ids, **kw)
    for l in (0, 3, 5):
        part = slice(l * K, (l + 1) * K)
        f1, e1, r1, t1 = model.design(toks[part], target, steps, chain_ids=ids[part], **kw)
        assert torch.equal(f1, final[part]) and torch.equal(e1, energy[part]) and torch.equal(r1, rung[part]), l
        for k in traj:
            assert torch.equal(t1[k], traj[k][:, part]), (k, l)
    assert 0 < traj["swapped"].sum().item() and 0 < traj["accepted"].sum().item()
    # batches cut by max_bytes hold whole ladders: 11 chains would fit, 8 run
    S = T - 2
    with torch.cuda.device(toks.device):
        eng = model._engine_ready(toks.device)
        need = eng.rows_contacts_bytes(11, T, 11 * S)
        small = eng.rows_contacts_bytes(3, T, 3 * S)
    cut = model.design(toks, target, steps, chain_ids=ids, max_bytes=need, **kw)
    assert torch.equal(cut[0], final) and torch.equal(cut[1], energy) and torch.equal(cut[2], rung)
    assert all(torch.equal(cut[3][k], traj[k]) for k in traj)
    with pytest.raises(ValueError, match="a batch holds whole ladders"):
        model.design(toks, target, steps, chain_ids=ids, max_bytes=small, **kw)


def test_ladders_that_never_swap_are_independent_constant_temperature_calls():
    model = esm2_model(2)
    K, B, T, steps = 4, 8, 70, 10
    toks, target = chains(model, B, T), target_for(model, T)
    ids = [11, 3, 2 ** 31 - 1, 40, 7, 8, 100, 5]
    final, energy, rung, traj = model.design(toks, target, steps, seed=SEED, chain_ids=ids, replicas=K, swap_every=0, temperature=LADDER,
                                             return_trajectory=True)
    assert rung.tolist() == [b % K for b in range(B)] and not traj["swapped"].any() and bool((traj["swap_u"] == -1.0).all())
    for k in range(K):
        f1, e1, t1 = model.design(toks[k::K].contiguous(), target, steps, seed=SEED, chain_ids=ids[k::K], temperature=LADDER[k],
                                  return_trajectory=True)
        assert torch.equal(f1, final[k::K]) and torch.equal(e1, energy[k::K]), k
        for name in D.TRAJECTORY_FIELDS:
            assert torch.equal(t1[name], traj[name][:, k::K]), (name, k)
    assert 0 < traj["accepted"].sum().item() < steps * B


# ---- the command line -----------------------------------------------------------------------------------------------------------
def test_command_line_end_to_end_with_replicas_and_the_ngram_term(tmp_path):
    from esm_amd import ngram_table, pretrained
    from esm_amd.synth import write_esm2_checkpoint

    write_esm2_checkpoint(str(tmp_path), "esm2_t2_synth_UR50D", L, 128, 2, seed=3)
    fasta = tmp_path / "bg.fasta"
    fasta.write_text(">a\nMKTAYIAKQRQISFVKSHFSRQLEERLGLIEVQ\n>b\nACDEFGHIKLMNPQRSTVWYAACCDDEEMKTAYIAK\n")
    table = tmp_path / "bg.npz"
    ngram_table.main(["--fasta", str(fasta), "--output", str(table)])
    native = "MKTAYIAKQRQISFVKSHFSRQLEERLGLIEVQ"
    out, log = tmp_path / "o.fasta", tmp_path / "l.csv"
    ckpt = str(tmp_path / "esm2_t2_synth_UR50D.pt")
    D.main(["--model-location", ckpt, "--target-from-sequence", native, "--num-chains", "4", "--steps", "6", "--replicas", "2", "--ladder",
            "1:4", "--w-ngram", "1", "--ngram-table", str(table), "--seed", "4", "--output", str(out), "--log", str(log)])
    recs = out.read_text().splitlines()
    assert len(recs) == 8
    model, alphabet = pretrained.load_model_and_alphabet(ckpt)
    model = model.eval().cuda()
    convert = alphabet.get_batch_converter()
    target = model.predict_contacts(convert([("native", native)])[2].cuda())[0].float().cpu().numpy()
    seqs = [recs[2 * c + 1] for c in range(4)]
    want = model.design_energy(convert([(str(c), s) for c, s in enumerate(seqs)])[2], target, w_ngram=1.0, ngram=Background.load(table))
    rungs = []
    for c in range(4):
        fields = dict(f.split("=") for f in recs[2 * c].split("|")[1:])
        assert recs[2 * c].startswith(f">design|chain={c}|seed=4|energy=") and list(fields) == ["chain", "seed", "energy", "rung"]
        assert fields["energy"] == "%.6f" % want["energy"][c].item() and len(seqs[c]) == len(native)
        rungs.append(int(fields["rung"]))
    assert sorted(rungs[:2]) == sorted(rungs[2:]) == [0, 1]
    rows = log.read_text().splitlines()
    assert rows[0] == "step,chain," + ",".join(D.TRAJECTORY_FIELDS + D.NGRAM_FIELDS + D.REPLICA_FIELDS) and len(rows) == 1 + 6 * 4
    assert [r.split(",")[-3] for r in rows[1:5]] == ["0", "1", "0", "1"]  # the rung of step 0: chain b at b % K
