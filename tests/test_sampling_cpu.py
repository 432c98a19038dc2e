"""The host side of sampling without a GPU: the numpy references of tests/_sampling_ref.py against known answers, the rule
that says which draws a comparison may count, the argument checks of the three C entries (refused before any HIP call, on
fake pointers as in tests/test_scoring_cpu.py), the command line and the refusal of the MSA Transformer."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import _sampling_ref as R
import esm
from esm_amd import _native as N
from esm_amd import sample, sampling

FAKE = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused first
U0 = dict(seed=2024, chain=7, step=3, index=17499144)  # a counter whose uniform is exactly 0 (found by search)


def err():
    return N.lib.esmk_last_error().decode()


# ---- the references ---------------------------------------------------------------------------------------------------------
KNOWN = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    assert " ".join("%08x" % int(w) for w in R.philox4x32_10(counter, key)) == want


def test_philox_is_elementwise_and_keyed_by_the_seed():
    idx = np.arange(5)
    many = R.word0(0x123456789ABCDEF0, 3, 9, R.TOKEN, idx)
    for i in idx:
        one = R.philox4x32_10((3, 9, 1, int(i)), (0x9ABCDEF0, 0x12345678))[0]
        assert int(many[i]) == int(one)
    u = R.uniform(5, np.arange(1000), 2, 0)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all() and len(set(u.tolist())) > 990
    assert R.uniform(U0["seed"], U0["chain"], U0["step"], U0["index"]) == 0.0


def test_reference_shuffle_is_a_permutation_of_its_counter_only():
    for n in (0, 1, 2, 63, 64, 65, 1022):
        src = list(range(100, 100 + n))
        got = R.shuffle(src, seed=11, chain=4, epoch=2)
        assert sorted(got) == src
        assert got == R.shuffle(src, seed=11, chain=4, epoch=2)
    src = list(range(64))
    base = R.shuffle(src, 11, 4, 2)
    assert base != src
    for other in (R.shuffle(src, 12, 4, 2), R.shuffle(src, 11, 5, 2), R.shuffle(src, 11, 4, 3)):
        assert other != base and sorted(other) == src
    # the values shuffled do not enter the random numbers: the same index moves
    assert [x - 100 for x in R.shuffle([x + 100 for x in src], 11, 4, 2)] == base


@pytest.mark.parametrize("temperature", [0.5, 1.0, 2.0])
def test_the_undecided_rule_leaves_out_few_draws(temperature):
    """4096 reference draws on N(0, 3^2) logits: at most 0.5 % are undecided, and on the decided ones an fp32 emulation of the
    kernel's arithmetic draws the fp64 token."""
    n, V = 4096, 33
    rng = np.random.default_rng(17)
    logits = (3.0 * rng.standard_normal((n, V))).astype(np.float32)
    lp = (logits - np.log(np.exp(logits.astype(np.float64)).sum(1, keepdims=True))).astype(np.float32)
    mask = sum(1 << v for v in range(4, 24))
    u = R.uniform(3, np.arange(n) % 64, 5, np.arange(n) // 64)
    undecided = 0
    for i in range(n):
        tok, logq, decided = R.draw(lp[i], u[i], mask, 1.0 / temperature)
        assert (mask >> tok) & 1 and logq <= 0.0
        if not decided:
            undecided += 1
            continue
        assert R.draw_fp32(lp[i], u[i], mask, 1.0 / temperature) == tok, i
    assert undecided <= R.UNDECIDED_CAP * n, undecided


def test_reference_draw_edges():
    row = np.log(np.array([0.1, 0.2, 0.3, 0.4], dtype=np.float32))
    assert R.draw(row, 0.0, 0b1111, 1.0)[0] == 0
    assert R.draw(row, 0.95, 0b1111, 1.0)[0] == 3
    assert R.draw(row, 0.5, 0b0100, 1.0)[:2] == (2, 0.0)  # one candidate: probability 1
    assert R.draw(row, 0.5, 0b0100, 1.0, exclude=2)[0] == -1
    assert R.draw(row, 0.2, 0b1111, 1.0, exclude=0)[0] == 1  # 0.2 * 0.9 = 0.18 < 0.2
    tie = np.array([-1.0, -0.5, -0.5, -2.0], dtype=np.float32)
    assert R.draw(tie, 0.99, 0b1111, 0.0) == (1, 0.0, True)
    tok, logq, _ = R.draw(row, 0.35, 0b1111, 1.0)
    assert tok == 2 and abs(logq - np.log(0.3)) < 1e-6


# ---- the C entries refuse bad arguments before any HIP call -----------------------------------------------------------------
def test_sampling_op_argument_checks():
    perm, draw, commit = N.lib.esmk_op_permute_positions, N.lib.esmk_op_sample_rows, N.lib.esmk_op_commit_tokens

    def p(off=FAKE, pos=FAKE, cid=FAKE, out=FAKE, n_chain=3, total=9, seed=1, epoch=0):
        return perm(off, pos, cid, out, n_chain, total, seed, epoch, None)

    for kw in (dict(off=None), dict(pos=None), dict(cid=None), dict(out=None)):
        assert p(**kw) != 0 and err() == "esmk_op_permute_positions: null argument", kw
    for kw in (dict(n_chain=0), dict(total=0), dict(n_chain=-1), dict(total=-4)):
        assert p(**kw) != 0 and "esmk_op_permute_positions: n_chain and total must be positive" in err(), kw
    assert p(epoch=-1) != 0 and "esmk_op_permute_positions: epoch" in err()

    def d(lp=FAKE, chain=FAKE, index=FAKE, exclude=None, mask=0xFFFFF0, inv_t=1.0, seed=1, step=0, tok=FAKE, logq=FAKE, u=None,
          n=4, V=33):
        return draw(lp, chain, index, exclude, mask, inv_t, seed, step, tok, logq, u, n, V, None)

    for kw in (dict(lp=None), dict(chain=None), dict(index=None), dict(tok=None), dict(logq=None)):
        assert d(**kw) != 0 and err() == "esmk_op_sample_rows: null argument", kw
    for kw in (dict(n=0), dict(n=-2), dict(n=2 ** 24 + 1)):
        assert d(**kw) != 0 and "esmk_op_sample_rows: n must be" in err(), kw
    for kw in (dict(V=0), dict(V=65), dict(V=-1)):
        assert d(**kw) != 0 and "esmk_op_sample_rows: V must be in 1 .. 64" in err(), kw
    for kw in (dict(inv_t=-1.0), dict(inv_t=float("nan")), dict(inv_t=float("inf"))):
        assert d(**kw) != 0 and "esmk_op_sample_rows: inv_temperature" in err(), kw
    assert d(step=-1) != 0 and "esmk_op_sample_rows: step" in err()

    def c(tokens=FAKE, slot=FAKE, pos=FAKE, tok=FAKE, n=4, B=2, T=70):
        return commit(tokens, slot, pos, tok, n, B, T, None)

    for kw in (dict(tokens=None), dict(slot=None), dict(pos=None), dict(tok=None)):
        assert c(**kw) != 0 and err() == "esmk_op_commit_tokens: null argument", kw
    for kw in (dict(n=0), dict(B=0), dict(T=0), dict(n=-1)):
        assert c(**kw) != 0 and "esmk_op_commit_tokens: n, B and T must be positive" in err(), kw
    assert c(B=2 ** 12, T=2 ** 13) != 0 and "2^24" in err()


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def test_allowed_mask_and_position_lists():
    model = esm.ESM2(1, 128, 2)
    a = model.alphabet
    std = sampling.allowed_mask(model)
    assert bin(std).count("1") == 20 and all((std >> a.get_idx(r)) & 1 for r in "ACDEFGHIKLMNPQRSTVWY")
    for special in (a.cls_idx, a.eos_idx, a.padding_idx, a.mask_idx):
        assert not (std >> special) & 1
    assert sampling.allowed_mask(model, "AG") == (1 << a.get_idx("A")) | (1 << a.get_idx("G"))
    assert sampling.allowed_mask(model, [5, 7]) == 0b10100000
    for bad in ("A?", [99], []):
        with pytest.raises(ValueError):
            sampling.allowed_mask(model, bad)
    toks = torch.tensor([[0, 5, 6, 7, 2], [0, 8, 9, 2, 1]])
    assert sampling._position_lists(model, toks, None) == [[1, 2, 3], [1, 2]]
    assert sampling._position_lists(model, toks, [2, 1, 2]) == [[1, 2], [1, 2]]
    assert sampling._position_lists(model, toks, [[3], []]) == [[3], []]
    for bad in ([0], [[4], [1]], [[1], [3]], [[1], [4]], [5]):  # <cls>, <eos>, <eos>, <pad>, outside
        with pytest.raises(ValueError):
            sampling._position_lists(model, toks, bad)


def test_plan_tables():
    """Chains of 5, 2 and 0 positions at per_step 2: three steps; the chain that is done leaves the batch."""
    ids = torch.tensor([10, 11, 12], dtype=torch.int32)
    plan = sampling._Plan([5, 2, 0], 2, 70, ids, torch.device("cpu"))
    assert plan.n_steps == 3 and plan.total == 7
    assert plan.steps == [(0, 4, 0, 2), (4, 6, 2, 3), (6, 7, 3, 4)]
    assert plan.order.tolist() == [0, 1, 5, 6, 2, 3, 4]
    assert plan.slot.tolist() == [0, 0, 1, 1, 0, 0, 0] and plan.index.tolist() == [0, 1, 0, 1, 0, 1, 0]
    assert plan.chain.tolist() == [10, 10, 11, 11, 10, 10, 10]
    assert plan.src.tolist() == [0, 1, 0, 0] and plan.copy_row0.tolist() == [0, 0, 70, 70, 0, 0, 0]
    assert plan.off.tolist() == [0, 2, 4, 4, 6, 6, 7]
    for s, (r0, r1, c0, c1) in enumerate(plan.steps):  # the slice a step hands to esmk_op_mask_rows_multi
        off = plan.off[c0 + s: c1 + s + 1].tolist()
        assert off[0] == r0 and off[-1] == r1 and len(off) == c1 - c0 + 1


def test_sampling_refuses_msa_models_cpu_models_and_bad_arguments():
    args = argparse.Namespace(layers=1, embed_dim=64, ffn_embed_dim=128, attention_heads=2, dropout=0.1, attention_dropout=0.1,
                              activation_dropout=0.1, max_positions=1024, embed_positions_msa=True, embed_positions_msa_dim=64,
                              max_tokens=2 ** 14, max_tokens_per_msa=2 ** 14)
    msa = esm.MSATransformer(args, esm.Alphabet.from_architecture("msa_transformer"))
    toks = torch.zeros((1, 2, 8), dtype=torch.int64)
    for call in (lambda: msa.gibbs_sample(toks, 1), lambda: msa.inpaint(toks), lambda: sampling.gibbs_sample(msa, toks, 1),
                 lambda: sampling.inpaint(msa, toks)):
        with pytest.raises(NotImplementedError, match="MSA Transformer"):
            call()
    model = esm.ESM2(1, 128, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.gibbs_sample(torch.tensor([[0, 5, 2]]), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.inpaint(torch.tensor([[0, 32, 2]]))
    import esm_amd

    assert esm_amd.gibbs_sample is sampling.gibbs_sample and esm_amd.inpaint is sampling.inpaint


# ---- the command line -----------------------------------------------------------------------------------------------------------
def test_cli_parsing(tmp_path):
    a = sample.parse_args(["--model-location", "m.pt", "--sequence", "MKTAY", "--output", "o.fasta"])
    assert (a.mode, a.sweeps, a.per_step, a.temperature, a.num_chains, a.seed) == ("gibbs", 1, 1, 1.0, 1, 0)
    a = sample.parse_args(["--model-location", "m.pt", "--fasta", "in.fasta", "--mode", "inpaint", "--sweeps", "3", "--per-step",
                           "8", "--temperature", "0.5", "--num-chains", "4", "--seed", "99", "--output", "o.fasta"])
    assert (a.mode, a.sweeps, a.per_step, a.temperature, a.num_chains, a.seed) == ("inpaint", 3, 8, 0.5, 4, 99)
    assert str(a.fasta) == "in.fasta" and a.sequence is None
    base = ["--model-location", "m.pt", "--output", "o.fasta"]
    for bad in (base, base + ["--sequence", "MK", "--fasta", "x"], base + ["--sequence", "MK", "--mode", "anneal"],
                base + ["--sequence", "MK", "--per-step", "0"], base + ["--sequence", "MK", "--num-chains", "0"],
                base + ["--sequence", "MK", "--temperature", "-1"], base + ["--sequence", "MK", "--seed", "-1"],
                base + ["--sequence", "MK", "--sweeps", "-1"], ["--sequence", "MK", "--output", "o.fasta"]):
        with pytest.raises(SystemExit):
            sample.parse_args(bad)
    assert sample.prepare_sequence("MK_A<mask>Y", "inpaint") == "MK<mask>A<mask>Y"
    with pytest.raises(ValueError, match="nothing to fill"):
        sample.prepare_sequence("MKTAY", "inpaint")
    with pytest.raises(ValueError, match="inpaint"):
        sample.prepare_sequence("MK_AY", "gibbs")
    chains = sample.chain_records([("a", "MK"), ("b", "TAY")], 2, "gibbs")
    assert chains == [("a", 0, "MK"), ("a", 1, "MK"), ("b", 2, "TAY"), ("b", 3, "TAY")]
    alphabet = esm.Alphabet.from_architecture("ESM-1b")
    _, _, toks = alphabet.get_batch_converter()([("a", "MK<mask>A"), ("b", "TA")])
    assert toks[0].tolist()[3] == alphabet.mask_idx and sample.decode(alphabet, toks[1].tolist()) == "TA"
    out = tmp_path / "o.fasta"
    sample.write_fasta(out, chains, ["MA", "MC", "TAG", "TAW"], seed=5)
    assert out.read_text() == ">a|chain=0|seed=5\nMA\n>a|chain=1|seed=5\nMC\n>b|chain=2|seed=5\nTAG\n>b|chain=3|seed=5\nTAW\n"


def test_cli_refuses_an_msa_model(tmp_path, monkeypatch):
    from esm_amd import pretrained

    args = argparse.Namespace(layers=1, embed_dim=64, ffn_embed_dim=128, attention_heads=2, dropout=0.1, attention_dropout=0.1,
                              activation_dropout=0.1, max_positions=1024, embed_positions_msa=True, embed_positions_msa_dim=64,
                              max_tokens=2 ** 14, max_tokens_per_msa=2 ** 14)
    alphabet = esm.Alphabet.from_architecture("msa_transformer")
    monkeypatch.setattr(pretrained, "load_model_and_alphabet", lambda location: (esm.MSATransformer(args, alphabet), alphabet))
    with pytest.raises(SystemExit, match="MSA Transformer"):
        sample.main(["--model-location", "msa.pt", "--sequence", "MKTAY", "--output", str(tmp_path / "o.fasta")])
    assert not (tmp_path / "o.fasta").exists()
