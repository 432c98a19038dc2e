"""The host side of variant scoring: ``score_mutations`` on hand-worked values, the argument checks of
``esmk_forward_rows`` / ``esmk_rows_workspace_bytes`` and of the two op entries (refused before any HIP call, on fake
pointers as in tests/test_c_abi_validation_cpu.py), the option parser and table handling of ``python -m esm_amd.predict``,
and the refusal of the MSA Transformer."""
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


def make(**kw):
    cfg = N.EsmkConfig(2, 128, 2, 512, 33, 1, 32, 0, 2, 1, 1, 1, N.dtype_code(torch.float16), 0, 0, 0)
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    assert N.lib.esmk_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, err()
    return h


# ---- score_mutations ---------------------------------------------------------------------------------------------------
def table(alphabet, T):
    """log-probability table with a recognisable value per (row, column): row r, column c -> -(r + c / 100)."""
    V = len(alphabet)
    return -(torch.arange(T, dtype=torch.float64).unsqueeze(1) + torch.arange(V, dtype=torch.float64) / 100)


def test_score_mutations_hand_worked():
    alphabet = esm.Alphabet.from_architecture("ESM-1b")  # prepends <cls>: residue idx sits in row idx + 1
    seq = "MKTAY"
    lp = table(alphabet, len(seq) + 2)
    a = alphabet.get_idx
    # K2G with 1-based numbering: residue index 1, row 2 -> lp[2, G] - lp[2, K] = (a(K) - a(G)) / 100
    assert scoring.score_mutations(lp, seq, "K2G", alphabet, offset_idx=1) == pytest.approx((a("K") - a("G")) / 100, abs=1e-12)
    # the same residue with 0-based numbering, and a [1, T, V] table
    assert scoring.score_mutations(lp.unsqueeze(0), seq, "K1G", alphabet) == pytest.approx((a("K") - a("G")) / 100, abs=1e-12)
    # the BOS shift: a table whose row idx + 1 alone is non-zero
    only = torch.zeros_like(lp)
    only[1 + 4] = lp[1 + 4]
    got = scoring.score_mutations(only, seq, ["Y5W", "M1A"], alphabet, offset_idx=1)
    assert got[0] == pytest.approx((a("Y") - a("W")) / 100, abs=1e-12) and got[1] == 0.0
    # offset 10: 'T12C' is residue index 2
    assert scoring.score_mutations(lp, seq, "T12C", alphabet, offset_idx=10) == pytest.approx((a("T") - a("C")) / 100, abs=1e-12)
    # an alphabet without <cls> has no shift
    class NoBos:
        prepend_bos = False
        get_idx = staticmethod(alphabet.get_idx)
    assert scoring.score_mutations(only, seq, "Y5W", NoBos, offset_idx=1) == 0.0  # row 4 is zero, row 5 was residue 4's
    assert esm_amd.score_mutations is scoring.score_mutations


def test_score_mutations_refuses_a_wrong_wild_type():
    alphabet = esm.Alphabet.from_architecture("ESM-1b")
    lp = table(alphabet, 7)
    with pytest.raises(ValueError, match="wild type"):
        scoring.score_mutations(lp, "MKTAY", "A2G", alphabet, offset_idx=1)  # residue 2 is K
    with pytest.raises(ValueError, match="wild type"):
        scoring.score_mutations(lp, "MKTAY", "K2G", alphabet, offset_idx=0)  # 0-based: index 2 is T
    with pytest.raises(ValueError, match="outside"):
        scoring.score_mutations(lp, "MKTAY", "Y6G", alphabet, offset_idx=0)
    with pytest.raises(ValueError, match="form"):
        scoring.score_mutations(lp, "MKTAY", "K-G", alphabet)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
def test_forward_rows_argument_checks():
    h = make()
    n, off = ctypes.c_size_t(), ctypes.c_size_t()
    q = N.lib.esmk_rows_workspace_bytes
    assert q(h, 2, 70, 65, ctypes.byref(n), ctypes.byref(off)) == 0 and 0 < off.value < n.value
    base = ctypes.c_size_t()
    assert N.lib.esmk_workspace_bytes(h, 2, 70, N.OUT_LOGITS, ctypes.byref(base)) == 0
    assert off.value >= base.value and n.value - off.value >= 65 * 33 * 4  # behind the forward's workspace; holds the logits
    assert q(h, 2, 70, 65, ctypes.byref(n), None) == 0  # the offset is optional
    assert q(None, 2, 70, 65, ctypes.byref(n), None) != 0 and "esmk_rows_workspace_bytes: null" in err()
    assert q(h, 2, 70, 65, None, None) != 0 and "esmk_rows_workspace_bytes: null" in err()
    assert q(h, 2, 70, 0, ctypes.byref(n), None) != 0 and "esmk_rows_workspace_bytes: n_sel" in err()
    assert q(h, 0, 70, 5, ctypes.byref(n), None) != 0 and "esmk_rows_workspace_bytes: B and T" in err()
    assert q(h, 1 << 14, 1 << 11, 5, ctypes.byref(n), None) != 0 and "2^24" in err()

    def call(handle=h, packed=FAKE, tokens=FAKE, B=2, T=70, sel=FAKE, n_sel=5, out=FAKE, ws=FAKE, ws_bytes=1 << 40):
        return N.lib.esmk_forward_rows(handle, packed, tokens, B, T, sel, n_sel, out, ws, ctypes.c_size_t(ws_bytes), None)

    for kw in (dict(handle=None), dict(packed=None), dict(tokens=None), dict(sel=None), dict(out=None), dict(ws=None)):
        assert call(**kw) != 0 and "esmk_forward_rows: null argument" in err(), kw
    assert call(n_sel=0) != 0 and "esmk_forward_rows: n_sel must be positive" in err()
    assert call(n_sel=-3) != 0 and "esmk_forward_rows: n_sel must be positive" in err()
    assert call(T=0) != 0 and "esmk_forward_rows: B and T" in err()
    assert call() != 0 and "esmk_forward_rows: esmk_set_rope_inv_freq was not called" in err()
    assert call(ws_bytes=base.value) != 0 and "esmk_forward_rows: workspace too small" in err()
    N.lib.esmk_destroy(h)
    big = make(vocab=65)
    assert q(big, 2, 70, 5, ctypes.byref(n), None) != 0 and "vocabulary above 64" in err()
    N.lib.esmk_destroy(big)


def test_forward_rows_refuses_an_msa_handle():
    cfg = N.EsmkMsaConfig(2, 128, 2, 256, 33, 1, 32, 0, 2, 1, 0, 1026, 1, N.dtype_code(torch.float16))
    hm = ctypes.c_void_p()
    assert N.lib.esmk_msa_create(ctypes.byref(cfg), ctypes.byref(hm)) == 0
    n = ctypes.c_size_t()
    assert N.lib.esmk_rows_workspace_bytes(hm, 1, 16, 4, ctypes.byref(n), None) != 0
    assert "esmk_rows_workspace_bytes: MSA handle" in err()
    assert N.lib.esmk_forward_rows(hm, FAKE, FAKE, 1, 16, FAKE, 4, FAKE, FAKE, ctypes.c_size_t(1 << 40), None) != 0
    assert "esmk_forward_rows: MSA handle" in err()
    N.lib.esmk_destroy(hm)


def test_scoring_op_argument_checks():
    m, s = N.lib.esmk_op_mask_rows, N.lib.esmk_op_log_softmax_rows
    assert m(None, None, FAKE, FAKE, 1, 70, 4, 32, None) != 0 and "esmk_op_mask_rows: null" in err()
    assert m(FAKE, None, None, FAKE, 1, 70, 4, 32, None) != 0 and "esmk_op_mask_rows: null" in err()
    assert m(FAKE, None, FAKE, FAKE, 1, 70, 0, 32, None) != 0 and "positive" in err()
    assert m(FAKE, None, FAKE, FAKE, 1, 1 << 20, 1 << 10, 32, None) != 0 and "2^24" in err()
    assert s(None, FAKE, None, None, 4, 33, None) != 0 and "esmk_op_log_softmax_rows: null" in err()
    assert s(FAKE, FAKE, FAKE, None, 4, 33, None) != 0 and "go together" in err()
    assert s(FAKE, FAKE, None, None, 0, 33, None) != 0 and "n must be" in err()
    assert s(FAKE, FAKE, None, None, 4, 65, None) != 0 and "V must be" in err()


# ---- python -m esm_amd.predict ---------------------------------------------------------------------------------------------
def test_cli_parser_takes_the_reference_options():
    p = predict.create_parser()
    a = p.parse_args(["--model-location", "m1.pt", "m2.pt", "--sequence", "MKTAY", "--dms-input", "in.csv", "--mutation-col",
                      "mut", "--dms-output", "out.csv", "--offset-idx", "24", "--scoring-strategy", "masked-marginals"])
    assert a.model_location == ["m1.pt", "m2.pt"] and a.sequence == "MKTAY" and a.mutation_col == "mut"
    assert str(a.dms_input) == "in.csv" and str(a.dms_output) == "out.csv" and a.offset_idx == 24
    assert a.scoring_strategy == "masked-marginals"
    d = p.parse_args(["--model-location", "m", "--sequence", "M", "--dms-input", "i", "--dms-output", "o"])
    assert d.mutation_col == "mutant" and d.offset_idx == 0 and d.scoring_strategy == "wt-marginals"
    for s in ("wt-marginals", "masked-marginals", "pseudo-ppl"):
        p.parse_args(["--model-location", "m", "--sequence", "M", "--dms-input", "i", "--dms-output", "o",
                      "--scoring-strategy", s])
    with pytest.raises(SystemExit):
        p.parse_args(["--model-location", "m", "--sequence", "M", "--dms-input", "i", "--dms-output", "o",
                      "--scoring-strategy", "something-else"])


def test_cli_tables_and_msa_refusal(tmp_path):
    src = tmp_path / "scan.csv"
    src.write_text("mutant,fitness\nK2G,0.5\nT3C,-1.25\n")
    fields, rows = predict.read_table(src, "mutant")
    assert fields == ["mutant", "fitness"] and [r["mutant"] for r in rows] == ["K2G", "T3C"]
    with pytest.raises(SystemExit, match="no column"):
        predict.read_table(src, "variant")
    for r, s in zip(rows, (0.25, -3.0)):
        r["model"] = repr(s)
    out = tmp_path / "scored.csv"
    predict.write_table(out, fields + ["model"], rows)
    assert out.read_text().splitlines() == [",mutant,fitness,model", "0,K2G,0.5,0.25", "1,T3C,-1.25,-3.0"]
    with pytest.raises(SystemExit, match="MSA Transformer"):
        predict.main(["--model-location", "m", "--sequence", "MK", "--dms-input", str(src), "--dms-output", str(out),
                      "--msa-path", str(tmp_path / "x.a3m")])


def test_msa_transformer_methods_are_refused():
    args = argparse.Namespace(layers=1, embed_dim=64, ffn_embed_dim=128, attention_heads=2, dropout=0.1, attention_dropout=0.1,
                              activation_dropout=0.1, max_positions=1024, embed_positions_msa=True, embed_positions_msa_dim=64,
                              max_tokens=2 ** 14, max_tokens_per_msa=2 ** 14)
    model = esm.MSATransformer(args, esm.Alphabet.from_architecture("msa_transformer"))
    assert model.supports_scoring is False and esm.ESM2.supports_scoring is True
    for call in (model.masked_marginals, model.wt_marginals, model.pseudo_log_likelihood):
        with pytest.raises(NotImplementedError, match="MSA Transformer"):
            call(torch.zeros((1, 2, 8), dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        esm.ESM2(1, 128, 2).masked_marginals(torch.tensor([[0, 5, 2]]))


def test_position_lists_of_numpy_integers():
    """A flat list of numpy integers is one list for every sequence, not a list of per-sequence iterables."""
    import numpy as np

    model = esm.ESM2(1, 128, 2)
    toks = torch.tensor([[0, 5, 6, 7, 2], [0, 8, 9, 2, 1]])
    src, pos = scoring._position_rows(model, toks, list(np.array([1, 3])), residues_only=False)
    assert src.tolist() == [0, 0, 1, 1] and pos.tolist() == [1, 3, 1, 3]
    assert [t.tolist() for t in scoring._position_rows(model, toks, np.array([1, 3]), False)] == [[0, 0, 1, 1], [1, 3, 1, 3]]
    src, pos = scoring._position_rows(model, toks, [[1], np.array([2, 3])], residues_only=False)
    assert src.tolist() == [0, 1, 1] and pos.tolist() == [1, 2, 3]
    src, pos = scoring._position_rows(model, toks, None, residues_only=True)  # residues: no <cls>, <eos>, <pad>
    assert src.tolist() == [0, 0, 0, 1, 1] and pos.tolist() == [1, 2, 3, 1, 2]
    with pytest.raises(ValueError, match="<pad>"):
        scoring._position_rows(model, toks, [4], residues_only=False)
