"""The host side of multi-mutant variant scoring: ``parse_variant``, the argument checks of ``esmk_op_mask_rows_multi`` and
``esmk_op_score_rows`` (refused before any HIP call, on fake pointers as in tests/test_scoring_cpu.py), the refusal of a CPU
model and of the MSA Transformer, and the ``--mutation-sep`` option."""
import argparse
import ctypes

import pytest
import torch

import esm
import esm_amd
from esm_amd import _native as N
from esm_amd import predict, scoring

FAKE = ctypes.c_void_p(0x1000)


def err():
    return N.lib.esmk_last_error().decode()


def test_parse_variant():
    assert scoring.parse_variant("A42G") == [("A", 42, "G")]
    assert scoring.parse_variant("A2G:K4R") == [("A", 2, "G"), ("K", 4, "R")]
    assert scoring.parse_variant("K4R:A2G", offset_idx=1) == [("K", 3, "R"), ("A", 1, "G")]  # the order written
    assert scoring.parse_variant("A2G,K4R,T10C", sep=",") == [("A", 2, "G"), ("K", 4, "R"), ("T", 10, "C")]
    assert scoring.parse_variant(" A2G : K4R ") == [("A", 2, "G"), ("K", 4, "R")]
    with pytest.raises(ValueError, match="twice"):
        scoring.parse_variant("A2G:A2C")
    with pytest.raises(ValueError, match="form"):
        scoring.parse_variant("A2G:")
    with pytest.raises(ValueError, match="form"):
        scoring.parse_variant("A2G,K4R")  # ',' is not the separator here
    with pytest.raises(ValueError, match="form"):
        scoring.parse_mutation("A42G:K50R")  # parse_mutation itself is unchanged
    assert esm_amd.parse_variant is scoring.parse_variant and esm_amd.score_variants is scoring.score_variants


def test_variant_op_argument_checks():
    m, s = N.lib.esmk_op_mask_rows_multi, N.lib.esmk_op_score_rows

    def mask(tokens=FAKE, src=None, off=FAKE, pos=FAKE, out=FAKE, B=1, T=70, n=4, total=9, mask_idx=32):
        return m(tokens, src, off, pos, out, B, T, n, total, mask_idx, None)

    for kw in (dict(tokens=None), dict(off=None), dict(pos=None), dict(out=None)):
        assert mask(**kw) != 0 and "esmk_op_mask_rows_multi: null" in err(), kw
    for kw in (dict(B=0), dict(T=0), dict(n=0), dict(n=-2)):
        assert mask(**kw) != 0 and "esmk_op_mask_rows_multi: B, T and n must be positive" in err(), kw
    assert mask(total=-1) != 0 and "esmk_op_mask_rows_multi: total" in err()
    assert mask(T=1 << 20, n=1 << 10) != 0 and "2^24" in err()

    def score(lp=FAKE, wt=FAKE, mt=FAKE, off=FAKE, out=FAKE, n_rows=5, n_var=2, V=33):
        return s(lp, wt, mt, off, out, n_rows, n_var, V, None)

    for kw in (dict(lp=None), dict(wt=None), dict(mt=None), dict(off=None), dict(out=None)):
        assert score(**kw) != 0 and "esmk_op_score_rows: null" in err(), kw
    for kw in (dict(n_rows=0), dict(n_var=0), dict(V=0), dict(n_var=-1)):
        assert score(**kw) != 0 and "esmk_op_score_rows: n_rows, n_var and V must be positive" in err(), kw


def test_score_variants_checks_and_cpu_refusal():
    alphabet = esm.Alphabet.from_architecture("ESM-1b")
    model = esm.ESM2(1, 128, 2)
    seq = "MKTAY"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scoring.score_variants(model, alphabet, seq, ["K2G:A4C"], offset_idx=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.score_variants(alphabet, seq, ["K2G"], strategy="wt-marginals", offset_idx=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.masked_joint(torch.tensor([[0, 5, 6, 2]]), [[1, 2]])
    # the variants are checked against the sequence before anything runs: the errors of score_mutations
    with pytest.raises(ValueError, match="wild type"):
        scoring.score_variants(model, alphabet, seq, ["K2G:T4C"], offset_idx=1)  # residue 4 is A
    with pytest.raises(ValueError, match="outside"):
        scoring.score_variants(model, alphabet, seq, ["K2G:Y6C"], offset_idx=1)
    with pytest.raises(ValueError, match="form"):
        scoring.score_variants(model, alphabet, seq, ["K2G:A-C"], offset_idx=1)
    with pytest.raises(ValueError, match="twice"):
        scoring.score_variants(model, alphabet, seq, ["K2G:K2C"], offset_idx=1)
    with pytest.raises(ValueError, match="strategy"):
        scoring.score_variants(model, alphabet, seq, ["K2G"], strategy="something-else", offset_idx=1)


def test_msa_transformer_variant_methods_are_refused():
    args = argparse.Namespace(layers=1, embed_dim=64, ffn_embed_dim=128, attention_heads=2, dropout=0.1, attention_dropout=0.1,
                              activation_dropout=0.1, max_positions=1024, embed_positions_msa=True, embed_positions_msa_dim=64,
                              max_tokens=2 ** 14, max_tokens_per_msa=2 ** 14)
    alphabet = esm.Alphabet.from_architecture("msa_transformer")
    model = esm.MSATransformer(args, alphabet)
    with pytest.raises(NotImplementedError, match="MSA Transformer"):
        model.masked_joint(torch.zeros((1, 2, 8), dtype=torch.int64), [[1, 2]])
    with pytest.raises(NotImplementedError, match="MSA Transformer"):
        model.score_variants(alphabet, "MKTAY", ["K2G:A4C"], offset_idx=1)
    with pytest.raises(NotImplementedError, match="MSA Transformer"):
        scoring.score_variants(model, alphabet, "MKTAY", ["K2G:A4C"], offset_idx=1)
    with pytest.raises(NotImplementedError, match="MSA Transformer"):
        predict.score_table(model, alphabet, "MKTAY", ["K2G:A4C"], "masked-marginals", 1)


def test_cli_mutation_separator_option():
    base = ["--model-location", "m", "--sequence", "M", "--dms-input", "i", "--dms-output", "o"]
    p = predict.create_parser()
    assert p.parse_args(base).mutation_sep == ":"
    assert p.parse_args(base + ["--mutation-sep", ","]).mutation_sep == ","
