"""MSA row selection end to end on the MI355X (esm_amd/msa_select.py and what is built on it): the greedy pick against the lists
the reference notebook's own ``greedy_select`` returned, the weighted and uniform draws against the numpy reference, the
ensemble score against the mean of its parts, contact maps of a subsample, and the two modes of ``python -m
esm_amd.predict_msa``.  The model is the tiny MSA Transformer of tests/test_msa_scoring_gpu.py."""
import argparse
import importlib
import json
import os

import numpy as np
import pytest
import torch

import _msa_select_ref as M
import esm
import esm_amd
from esm_amd import msa_scoring, msa_select, predict_msa
from esm_amd.synth import synth_msa_state_dict

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msa_select_greedy.json")
L_, E, H, F = 2, 128, 2, 256


@pytest.fixture(scope="module")
def tiny():
    args = argparse.Namespace(layers=L_, embed_dim=E, ffn_embed_dim=F, attention_heads=H, dropout=0.1, attention_dropout=0.1,
                              activation_dropout=0.1, max_positions=1024, embed_positions_msa=True, embed_positions_msa_dim=E,
                              max_tokens=2 ** 14, max_tokens_per_msa=2 ** 14)
    alphabet = esm.Alphabet.from_architecture("msa_transformer")
    model = esm.MSATransformer(args, alphabet).eval()
    model.load_state_dict(synth_msa_state_dict(L_, E, H, F, seed=24), strict=True)
    return model.cuda(), alphabet


@pytest.fixture(scope="module")
def deep():
    """A 48 x 24 generator alignment as records, its byte matrix and its brute-force neighbour counts at theta 0.2."""
    a = M.family_msa(48, 24, 5)
    return M.records(a), a, M.neighbor_counts(a, M.max_mismatch(0.2, 24))


def variants_of(seq, n=6):
    """Single and double substitutions of the query at residues that are no gap, 1-based."""
    letters = "ACDEFGHIKLMNPQRSTVWY"
    at = [i for i, c in enumerate(seq) if c != "-"]
    out = [f"{seq[i]}{i + 1}{letters[(letters.index(seq[i]) + 3) % 20]}" for i in at[:n]]
    return out + [out[0] + ":" + out[3]]


def test_greedy_is_the_notebook_choice():
    with open(GOLDEN) as fh:
        g = json.load(fh)
    gen = g["generator"]
    a = M.family_msa(gen["n"], gen["L"], gen["seed"])
    msa = M.records(a)
    assert msa_select.subsample_indices(msa, g["num_seqs"], "greedy") == g["max"]
    assert msa_select.subsample_indices(msa, g["num_seqs"], "greedy-min") == g["min"]
    assert esm_amd.subsample_msa(msa, g["num_seqs"]) == [msa[i] for i in g["max"]]  # greedy is the default
    assert msa_select.subsample_indices(torch.from_numpy(a), g["num_seqs"], "greedy") == g["max"]  # a byte matrix as it is


def test_weighted_and_uniform_draws(deep, tiny):
    msa, a, counts = deep
    _, alphabet = tiny
    n = len(msa)
    assert np.array_equal(msa_select.msa_neighbor_counts(msa, 0.2).cpu().numpy(), counts)
    w = msa_select.msa_sequence_weights(msa, 0.2)
    assert w.dtype == torch.float64 and np.array_equal(w.cpu().numpy(), 1.0 / counts)
    assert msa_select.msa_neff(msa, 0.2) == float(w.sum()) and 1.0 < msa_select.msa_neff(msa) < n
    assert np.array_equal(msa_select.msa_mismatches(msa, [0, 7]).cpu().numpy(), M.mismatch_rows(a, [0, 7]))
    _, _, toks = alphabet.get_batch_converter()(msa)
    seen = set()
    for sub in (0, 1, 2):
        idx = msa_select.subsample_indices(msa, 12, "weighted", seed=3, subsample=sub)
        assert idx == M.weighted_pick(n, 12, 3, sub, counts)
        assert idx[0] == 0 and len(idx) == 12 and idx == sorted(set(idx))
        assert msa_select.subsample_indices(msa, 12, "weighted", seed=3, subsample=sub) == idx  # the same rows again
        assert msa_select.subsample_indices(toks, 12, "weighted", seed=3, subsample=sub) == idx  # strings or tokens
        assert msa_select.subsample_indices(toks[0].cuda(), 12, "weighted", seed=3, subsample=sub) == idx
        assert msa_select.subsample_msa(msa, 12, "weighted", seed=3, subsample=sub) == [msa[i] for i in idx]
        assert torch.equal(msa_select.subsample_msa(toks, 12, "weighted", seed=3, subsample=sub), toks[:, idx])
        seen.add(tuple(idx))
        uni = msa_select.subsample_indices(msa, 12, "uniform", seed=3, subsample=sub)
        assert uni == M.weighted_pick(n, 12, 3, sub) and uni[0] == 0 and uni != idx
        other = M.records(M.family_msa(n, 24, 77))  # other rows, other neighbour counts: the uniform draw does not look
        assert msa_select.subsample_indices(other, 12, "uniform", seed=3, subsample=sub) == uni
        assert msa_select.subsample_indices(msa, 12, "uniform", theta=0.9, seed=3, subsample=sub) == uni
    assert len(seen) == 3  # different subsample numbers, different rows
    assert msa_select.subsample_indices(msa, 12, "weighted", seed=4) != msa_select.subsample_indices(msa, 12, "weighted", seed=3)


def test_ensemble_is_the_mean_of_its_subsamples(deep, tiny):
    msa, _, _ = deep
    model, alphabet = tiny
    variants = variants_of(msa[0][1])
    for strategy in ("weighted", "uniform"):
        mean, per = model.msa_score_variants_ensemble(alphabet, msa, variants, 8, n_subsamples=3, subsample=strategy, seed=2,
                                                      offset_idx=1)
        assert per.dtype == torch.float64 and tuple(per.shape) == (3, len(variants)) and len(mean) == len(variants)
        total = np.zeros(len(variants))
        for s in range(3):
            rows = msa_select.subsample_msa(msa, 8, strategy, seed=2, subsample=s)
            assert len(rows) == 8 and rows[0] == msa[0]
            got = msa_scoring.msa_score_variants(model, alphabet, rows, variants, offset_idx=1)
            assert per[s].tolist() == got  # bit for bit
            total = total + np.asarray(got, dtype=np.float64)
        assert mean == (total / 3).tolist()
        assert not torch.equal(per[0], per[1])  # different rows, different scores
    again = esm_amd.msa_score_variants_ensemble(model, alphabet, msa, variants, 8, 3, "uniform", seed=2, offset_idx=1)
    assert again[0] == mean and torch.equal(again[1], per)
    with pytest.raises(ValueError, match="n_subsamples"):
        model.msa_score_variants_ensemble(alphabet, msa, variants, 8, n_subsamples=0)
    with pytest.raises(ValueError, match="strategy"):
        model.msa_score_variants_ensemble(alphabet, msa, variants, 8, subsample="random")


def test_contacts_of_a_subsample(deep, tiny):
    msa, _, _ = deep
    model, alphabet = tiny
    _, _, toks = alphabet.get_batch_converter()(msa)
    toks = toks.cuda()
    idx = msa_select.subsample_indices(msa, 10, "greedy")
    assert idx[0] == 0 and len(idx) == 10
    with torch.no_grad():
        got = model.predict_contacts(msa_select.subsample_msa(toks, 10, "greedy"))
        want = model.predict_contacts(toks[:, idx])
        _, _, sub_toks = alphabet.get_batch_converter()(msa_select.subsample_msa(msa, 10, "greedy"))
        assert torch.equal(got, want) and torch.equal(got, model.predict_contacts(sub_toks.cuda()))
    assert tuple(got.shape) == (1, 24, 24)


# ---- python -m esm_amd.predict_msa ------------------------------------------------------------------------------------------------
@pytest.fixture()
def cli_files(deep, tiny, tmp_path, monkeypatch):
    msa, _, _ = deep
    model, alphabet = tiny
    a3m = tmp_path / "deep.a3m"
    # insertions in one record; a ragged record at the very end, which only a run that reads the whole file would meet
    text = "".join(f">{label}\n{seq[:5]}abc{seq[5:]}\n" if i == 3 else f">{label}\n{seq}\n" for i, (label, seq) in enumerate(msa))
    variants = variants_of(msa[0][1])
    scan = tmp_path / "scan.csv"
    scan.write_text("mutant,fitness\n" + "".join(f"{v},{0.25 * i}\n" for i, v in enumerate(variants)))
    from esm_amd import checkpoint

    monkeypatch.setattr(checkpoint, "load_model_and_alphabet", lambda location: (model, alphabet))
    return a3m, text, scan, variants, tmp_path


def expected_table(variants, scores):
    return [",mutant,fitness,tiny"] + [f"{i},{v},{0.25 * i},{float(s)!r}" for i, (v, s) in enumerate(zip(variants, scores))]


def test_predict_msa_defaults_take_the_first_records(deep, tiny, cli_files):
    msa, _, _ = deep
    model, alphabet = tiny
    a3m, text, scan, variants, tmp = cli_files
    a3m.write_text(text + ">ragged\nMKT\n")
    out = tmp / "first.csv"
    base = ["--model-location", "tiny", "--msa-path", str(a3m), "--dms-input", str(scan), "--dms-output", str(out),
            "--offset-idx", "1", "--msa-samples", "9"]
    assert predict_msa.main(base) == 0
    first = esm_amd.read_msa(a3m, 9)
    assert first == msa[:9]
    want = predict_msa.score_table(model, alphabet, first, variants, "masked-marginals", 1, ":")
    assert out.read_text().splitlines() == expected_table(variants, want)
    out2 = tmp / "first2.csv"
    assert predict_msa.main(base[:7] + [str(out2)] + base[8:] + ["--msa-subsample", "first", "--msa-ensemble", "1"]) == 0
    assert out2.read_bytes() == out.read_bytes()


def test_predict_msa_ensemble_writes_the_mean(deep, tiny, cli_files):
    msa, _, _ = deep
    model, alphabet = tiny
    a3m, text, scan, variants, tmp = cli_files
    a3m.write_text(text)
    out = tmp / "ens.csv"
    assert predict_msa.main(["--model-location", "tiny", "--msa-path", str(a3m), "--dms-input", str(scan), "--dms-output", str(out),
                             "--offset-idx", "1", "--msa-samples", "9", "--msa-subsample", "weighted", "--msa-ensemble", "2",
                             "--msa-seed", "6", "--msa-theta", "0.3"]) == 0
    mean, per = msa_scoring.msa_score_variants_ensemble(model, alphabet, msa, variants, 9, 2, "weighted", 0.3, 6, offset_idx=1)
    assert out.read_text().splitlines() == expected_table(variants, mean)
    assert mean == ((per[0] + per[1]) / 2).tolist()
    # one greedy subsample: the rows of subsample_msa, scored once
    out = tmp / "greedy.csv"
    assert predict_msa.main(["--model-location", "tiny", "--msa-path", str(a3m), "--dms-input", str(scan), "--dms-output", str(out),
                             "--offset-idx", "1", "--msa-samples", "9", "--msa-subsample", "greedy"]) == 0
    want = predict_msa.score_table(model, alphabet, msa_select.subsample_msa(msa, 9, "greedy"), variants, "masked-marginals", 1)
    assert out.read_text().splitlines() == expected_table(variants, want)


def test_subsample_msa_command_line(deep, cli_files, capsys):
    msa, a, counts = deep
    a3m, text, _, _, tmp = cli_files
    a3m.write_text(text)
    cli = importlib.import_module("esm_amd.subsample_msa")
    out, wout = tmp / "picked.a3m", tmp / "w.npy"
    assert cli.main(["--msa-path", str(a3m), "--num-seqs", "10", "--output", str(out), "--weights-out", str(wout)]) == 0
    idx = msa_select.subsample_indices(msa, 10, "greedy")
    assert esm_amd.read_msa(out) == [msa[i] for i in idx]  # insertions removed, query first, file order
    assert np.array_equal(np.load(wout), 1.0 / counts)
    said = capsys.readouterr().out
    assert "N = 48" in said and "L = 24" in said and f"Neff = {float((1.0 / counts).sum()):.1f}" in said
    assert cli.main(["--msa-path", str(a3m), "--num-seqs", "10", "--output", str(out), "--strategy", "weighted", "--seed", "3",
                     "--subsample", "1"]) == 0
    assert esm_amd.read_msa(out) == [msa[i] for i in M.weighted_pick(48, 10, 3, 1, counts)]
