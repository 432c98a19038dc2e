"""The host side of variant scoring with the MSA Transformer (esm_amd/msa_scoring.py over ``esmk_msa_forward_rows``): the
argument checks of the two new C entries (refused before any HIP call, on fake pointers as in tests/test_scoring_cpu.py),
``read_msa``, the ValueErrors of the Python layer (raised before a device is asked for), the option parser and table handling
of ``python -m esm_amd.predict_msa``, the refusals the single-sequence names keep, and the oracle against the table the
reference's own MSA loop produced (tests/golden/make_golden_msa_scoring.py)."""
import argparse
import ctypes
import os

import pytest
import torch

import esm
import esm_amd
from esm_amd import _native as N
from esm_amd import msa_scoring, predict, predict_msa, scoring

FAKE = ctypes.c_void_p(0x1000)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msa_scoring_tiny.pt")


def err():
    return N.lib.esmk_last_error().decode()


def make_msa(**kw):
    cfg = N.EsmkMsaConfig(2, 128, 2, 256, 33, 1, 32, 0, 2, 1, 0, 1026, 1, N.dtype_code(torch.float16), 0)
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    assert N.lib.esmk_msa_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, err()
    return h


def tiny_model(max_positions=1024):
    args = argparse.Namespace(layers=1, embed_dim=64, ffn_embed_dim=128, attention_heads=1, dropout=0.1, attention_dropout=0.1,
                              activation_dropout=0.1, max_positions=max_positions, embed_positions_msa=True,
                              embed_positions_msa_dim=64, max_tokens=2 ** 14, max_tokens_per_msa=2 ** 14)
    alphabet = esm.Alphabet.from_architecture("msa_transformer")
    return esm.MSATransformer(args, alphabet).eval(), alphabet


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
def test_msa_rows_workspace_query():
    h = make_msa()
    q = N.lib.esmk_msa_rows_workspace_bytes
    n, off, base = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    for B, R, C, n_sel in ((1, 8, 33, 1), (33, 8, 33, 33), (5, 6, 65, 11), (3, 7, 19, 400)):
        assert q(h, B, R, C, n_sel, ctypes.byref(n), ctypes.byref(off)) == 0, err()
        assert N.lib.esmk_msa_workspace_bytes(h, B, R, C, N.OUT_LOGITS, ctypes.byref(base)) == 0
        # behind (at least) the forward's own workspace; the tail holds the selected logits
        assert off.value >= base.value and n.value - off.value >= n_sel * 33 * 4 and off.value % 256 == 0
    assert q(h, 2, 8, 33, 4, ctypes.byref(n), None) == 0  # the offset is optional
    who = "esmk_msa_rows_workspace_bytes: "
    assert q(None, 2, 8, 33, 4, ctypes.byref(n), None) != 0 and who + "null" in err()
    assert q(h, 2, 8, 33, 4, None, None) != 0 and who + "null" in err()
    assert q(h, 2, 8, 33, 0, ctypes.byref(n), None) != 0 and who + "n_sel must be positive" in err()
    assert q(h, 0, 8, 33, 4, ctypes.byref(n), None) != 0 and who + "B, R, C must be positive" in err()
    assert q(h, 1 << 10, 1 << 10, 1 << 5, 4, ctypes.byref(n), None) != 0 and who + "B*R*C exceeds 2^24" in err()
    assert q(h, 1, 1025, 33, 4, ctypes.byref(n), None) != 0 and who + "MSA position embedding covers a depth of 1024" in err()
    assert q(h, 1, 8, 1025, 4, ctypes.byref(n), None) != 0 and who + "more than 1024 columns" in err()
    N.lib.esmk_destroy(h)


def test_msa_forward_rows_argument_checks():
    h = make_msa()
    need = ctypes.c_size_t()
    assert N.lib.esmk_msa_rows_workspace_bytes(h, 2, 8, 33, 5, ctypes.byref(need), None) == 0

    def call(handle=h, packed=FAKE, tokens=FAKE, B=2, R=8, C=33, sel=FAKE, n_sel=5, out=FAKE, ws=FAKE, ws_bytes=1 << 40):
        return N.lib.esmk_msa_forward_rows(handle, packed, tokens, B, R, C, sel, n_sel, out, ws, ctypes.c_size_t(ws_bytes), None)

    who = "esmk_msa_forward_rows: "
    for kw in (dict(handle=None), dict(packed=None), dict(tokens=None), dict(sel=None), dict(out=None), dict(ws=None)):
        assert call(**kw) != 0 and who + "null argument" in err(), kw
    assert call(n_sel=0) != 0 and who + "n_sel must be positive" in err()
    assert call(n_sel=-3) != 0 and who + "n_sel must be positive" in err()
    assert call(R=0) != 0 and who + "B, R, C must be positive" in err()
    assert call(B=1 << 10, R=1 << 10, C=1 << 5) != 0 and who + "B*R*C exceeds 2^24 rows" in err()
    assert call(R=1025) != 0 and who + "MSA position embedding covers a depth of 1024 alignments" in err()
    assert call(C=1025) != 0 and who + "more than 1024 columns are not supported" in err()
    assert call(ws_bytes=need.value - 1) != 0 and who + "workspace too small" in err()
    base = ctypes.c_size_t()
    assert N.lib.esmk_msa_workspace_bytes(h, 2, 8, 33, N.OUT_LOGITS, ctypes.byref(base)) == 0
    assert need.value > base.value and call(ws_bytes=base.value) != 0 and who + "workspace too small" in err()
    N.lib.esmk_destroy(h)
    short = make_msa(num_positions=40)  # a position table for 38 columns
    assert call(handle=short, C=39) != 0 and who + "sequence length above the maximum of the positional embedding" in err()
    N.lib.esmk_destroy(short)
    big = make_msa(vocab=65)
    assert call(handle=big) != 0 and who + "vocabulary above 64 entries" in err()
    N.lib.esmk_destroy(big)


def test_msa_forward_rows_refuses_a_single_sequence_handle_and_the_other_way_round():
    cfg = N.EsmkConfig(2, 128, 2, 512, 33, 1, 32, 0, 2, 1, 1, 1, N.dtype_code(torch.float16), 0, 0, 0)
    h = ctypes.c_void_p()
    assert N.lib.esmk_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    n = ctypes.c_size_t()
    assert N.lib.esmk_msa_rows_workspace_bytes(h, 1, 4, 16, 4, ctypes.byref(n), None) != 0
    assert "esmk_msa_rows_workspace_bytes: not an MSA model handle" in err()
    assert N.lib.esmk_msa_forward_rows(h, FAKE, FAKE, 1, 4, 16, FAKE, 4, FAKE, FAKE, ctypes.c_size_t(1 << 40), None) != 0
    assert "esmk_msa_forward_rows: not an MSA model handle" in err()
    N.lib.esmk_destroy(h)
    hm = make_msa()  # esmk_forward_rows keeps refusing MSA handles
    assert N.lib.esmk_forward_rows(hm, FAKE, FAKE, 1, 16, FAKE, 4, FAKE, FAKE, ctypes.c_size_t(1 << 40), None) != 0
    assert "esmk_forward_rows: MSA handle" in err()
    # esmk_msa_forward's own messages keep its name
    assert N.lib.esmk_msa_forward(hm, FAKE, FAKE, 1, 4, 1025, None, 0, None, N.OUT_LOGITS, FAKE, None, None, None, FAKE,
                                  ctypes.c_size_t(1 << 40), None) != 0
    assert err() == "esmk_msa_forward: more than 1024 columns are not supported"
    N.lib.esmk_destroy(hm)


def test_the_rows_entry_plans_the_slice_count_of_one_msa():
    """esmk_debug_msa_row_slices: esmk_msa_forward chooses the K slices of the tied-row score GEMM from B, the rows entry
    always takes the count of B = 1 — (8, 33) with two heads: 8 against 4 at B = 33; (6, 65): 6 against 2 at B = 65."""
    h = make_msa()
    s = ctypes.c_int32()

    def slices(B, R, C, rows_entry):
        assert N.lib.esmk_debug_msa_row_slices(h, B, R, C, rows_entry, ctypes.byref(s)) == 0, err()
        return s.value

    assert slices(1, 8, 33, 0) == 8 and slices(33, 8, 33, 0) == 4 and slices(33, 8, 33, 1) == 8
    assert slices(1, 6, 65, 0) == 6 and slices(65, 6, 65, 0) == 2 and slices(65, 6, 65, 1) == 6
    for B in (1, 2, 7, 33, 100):
        for R, C in ((8, 33), (6, 65), (7, 19), (400, 301), (16, 257)):
            assert slices(B, R, C, 1) == slices(1, R, C, 0) >= slices(B, R, C, 0)
    assert N.lib.esmk_debug_msa_row_slices(h, 0, 8, 33, 0, ctypes.byref(s)) != 0 and "must be positive" in err()
    N.lib.esmk_destroy(h)


# ---- read_msa ------------------------------------------------------------------------------------------------------------
def test_read_msa_removes_insertions_and_honours_nseq(tmp_path):
    a3m = tmp_path / "p.a3m"
    a3m.write_text("#a comment in front of the first record\n"
                   ">query some description\nMKTAY\nIAK\n"
                   ">hit1\nMK-AYabcIA.K*\n"
                   ">hit2\n-KTaAYIgg\nAK\n"
                   ">hit3\nMKTAYIAK\n")
    msa = esm_amd.read_msa(a3m, 3)
    assert msa == [("query some description", "MKTAYIAK"), ("hit1", "MK-AYIAK"), ("hit2", "-KTAYIAK")]
    assert len({len(s) for _, s in msa}) == 1
    assert len(esm_amd.read_msa(a3m, 400)) == 4 and esm_amd.read_msa(a3m, 1) == msa[:1] and esm_amd.read_msa(a3m, 0) == []
    # what the batch converter makes of it: [1, R, C] behind <cls>
    _, _, toks = esm.Alphabet.from_architecture("msa_transformer").get_batch_converter()(msa)
    assert tuple(toks.shape) == (1, 3, 9)


# ---- ValueErrors of the Python layer: raised before a device is asked for --------------------------------------------------
def test_bad_positions_rows_and_wild_types_raise():
    model, alphabet = tiny_model()
    toks = torch.randint(4, 24, (3, 9))
    toks[:, 0] = 0
    toks[2, :] = 1   # a pad row, as the batch converter appends to a shallower MSA of a ragged batch
    toks[:, 7:] = 1  # pad columns
    for bad in ([9], [-1], [3, 12]):
        with pytest.raises(ValueError, match="outside"):
            msa_scoring.msa_masked_marginals(model, toks, positions=bad)
    with pytest.raises(ValueError, match="<pad>"):
        msa_scoring.msa_masked_marginals(model, toks, positions=[7])
    with pytest.raises(ValueError, match="<pad>"):
        model.msa_masked_marginals(toks, positions=[2], row=2)
    for row in (3, -1):
        with pytest.raises(ValueError, match="row"):
            msa_scoring.msa_masked_marginals(model, toks, row=row)
        with pytest.raises(ValueError, match="row"):
            msa_scoring.msa_wt_marginals(model, toks, row=row)
        with pytest.raises(ValueError, match="row"):
            msa_scoring.msa_masked_joint(model, toks, [[1]], row=row)
    with pytest.raises(ValueError, match="empty"):
        msa_scoring.msa_masked_joint(model, toks, [[1, 2], []])
    with pytest.raises(ValueError, match="outside"):
        model.msa_masked_joint(toks, [[1, 9]])
    with pytest.raises(ValueError, match="<pad>"):
        msa_scoring.msa_masked_joint(model, toks, [[1, 8]])
    with pytest.raises(ValueError, match="chunk"):
        msa_scoring.msa_masked_joint(model, toks, [[1]], chunk=0)
    with pytest.raises(ValueError, match="one MSA"):
        msa_scoring.msa_masked_marginals(model, toks[None].repeat(2, 1, 1))
    msa = [("q", "MKTAYIAK"), ("h", "MK-AYIAK")]
    with pytest.raises(ValueError, match="wild type"):
        msa_scoring.msa_score_variants(model, alphabet, msa, ["A2G"], offset_idx=1)  # residue 2 is K
    with pytest.raises(ValueError, match="outside"):
        model.msa_score_variants(alphabet, msa, ["K9G"], offset_idx=1)
    with pytest.raises(ValueError, match="twice"):
        msa_scoring.msa_score_variants(model, alphabet, msa, ["K2G:K2A"], offset_idx=1)
    with pytest.raises(ValueError, match="strategy"):
        msa_scoring.msa_score_variants(model, alphabet, msa, ["K2G"], strategy="pseudo-ppl", offset_idx=1)
    with pytest.raises(ValueError, match="empty"):
        msa_scoring.msa_score_variants(model, alphabet, [], ["K2G"])
    # valid arguments reach the device check: the engine has no CPU path
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        msa_scoring.msa_masked_marginals(model, toks, positions=[1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        msa_scoring.msa_score_variants(model, alphabet, msa, ["K2G"], offset_idx=1)
    with pytest.raises(TypeError, match="MSATransformer"):
        msa_scoring.msa_masked_marginals(esm.ESM2(1, 128, 2), toks)
    short, _ = tiny_model(max_positions=8)
    with pytest.raises(ValueError, match="above maximum"):
        msa_scoring.msa_masked_marginals(short, toks)
    assert esm_amd.msa_masked_marginals is msa_scoring.msa_masked_marginals
    assert esm_amd.msa_score_variants is msa_scoring.msa_score_variants


# ---- python -m esm_amd.predict_msa -----------------------------------------------------------------------------------------
def test_cli_parser_and_table_round_trip(tmp_path):
    p = predict_msa.create_parser()
    a = p.parse_args(["--model-location", "m1.pt", "m2.pt", "--msa-path", "p.a3m", "--dms-input", "in.csv", "--mutation-col",
                      "mut", "--dms-output", "out.csv", "--offset-idx", "24", "--msa-samples", "64", "--mutation-sep", "/",
                      "--scoring-strategy", "wt-marginals", "--sequence", "MKT"])
    assert a.model_location == ["m1.pt", "m2.pt"] and str(a.msa_path) == "p.a3m" and a.msa_samples == 64
    assert str(a.dms_input) == "in.csv" and str(a.dms_output) == "out.csv" and a.mutation_col == "mut"
    assert a.offset_idx == 24 and a.mutation_sep == "/" and a.scoring_strategy == "wt-marginals" and a.sequence == "MKT"
    d = p.parse_args(["--model-location", "m", "--msa-path", "p.a3m", "--dms-input", "i", "--dms-output", "o"])
    assert d.msa_samples == 400 and d.scoring_strategy == "masked-marginals" and d.sequence is None
    assert d.mutation_col == "mutant" and d.offset_idx == 0 and d.mutation_sep == ":"
    for bad in (["--scoring-strategy", "pseudo-ppl"], ["--scoring-strategy", "something-else"]):
        with pytest.raises(SystemExit):
            p.parse_args(["--model-location", "m", "--msa-path", "p.a3m", "--dms-input", "i", "--dms-output", "o"] + bad)
    with pytest.raises(SystemExit):  # the MSA is not optional here
        p.parse_args(["--model-location", "m", "--dms-input", "i", "--dms-output", "o"])

    a3m = tmp_path / "p.a3m"
    a3m.write_text(">q\nMKTAY\n>h\nMK-AYgg\n")
    assert predict_msa.load_msa(a3m, 400) == [("q", "MKTAY"), ("h", "MK-AY")]
    assert predict_msa.load_msa(a3m, 1, "MKTAY") == [("q", "MKTAY")]
    with pytest.raises(SystemExit, match="first row"):
        predict_msa.load_msa(a3m, 400, "MKTAW")
    with pytest.raises(SystemExit, match="no sequence"):
        predict_msa.load_msa(a3m, 0)
    src = tmp_path / "scan.csv"
    src.write_text("mutant,fitness\nK2G,0.5\nT3C:A4W,-1.25\n")
    out = tmp_path / "scored.csv"
    with pytest.raises(SystemExit, match="first row"):  # refused before a model is loaded
        predict_msa.main(["--model-location", "m", "--msa-path", str(a3m), "--dms-input", str(src), "--dms-output", str(out),
                          "--sequence", "MKTAW"])
    # the table format is esm_amd.predict's
    fields, rows = predict_msa.read_table(src, "mutant")
    for r, s in zip(rows, (0.25, -3.0)):
        r["model"] = repr(s)
    predict_msa.write_table(out, fields + ["model"], rows)
    assert out.read_text().splitlines() == [",mutant,fitness,model", "0,K2G,0.5,0.25", "1,T3C:A4W,-1.25,-3.0"]
    assert predict_msa.read_table is predict.read_table and predict_msa.write_table is predict.write_table


def test_the_single_sequence_names_keep_refusing_the_msa_transformer(tmp_path):
    model, alphabet = tiny_model()
    assert model.supports_scoring is False
    toks = torch.zeros((1, 2, 8), dtype=torch.int64)
    for call in (model.masked_marginals, model.wt_marginals, model.pseudo_log_likelihood):
        with pytest.raises(NotImplementedError, match="MSA Transformer"):
            call(toks)
    for call in (model.masked_joint, model.score_variants):
        with pytest.raises(NotImplementedError, match="MSA Transformer"):
            call(toks, [[1]])
    with pytest.raises(NotImplementedError, match="MSA Transformer"):
        scoring._refuse_msa(model)
    with pytest.raises(NotImplementedError, match="MSA Transformer"):
        predict.score_table(model, alphabet, "MKTAY", ["K2G"], "masked-marginals", 1)
    src = tmp_path / "scan.csv"
    src.write_text("mutant\nK2G\n")
    with pytest.raises(SystemExit, match="MSA Transformer"):
        predict.main(["--model-location", "m", "--sequence", "MK", "--dms-input", str(src), "--dms-output",
                      str(tmp_path / "o.csv"), "--msa-path", str(tmp_path / "x.a3m")])


# ---- the oracle against the reference's recorded MSA loop -------------------------------------------------------------------
def test_oracle_reproduces_the_recorded_masked_marginal_table():
    """tests/golden/msa_scoring_tiny.pt: the reference's loop (predict.py:167-178) and label_row scores; the oracle's loop on
    the regenerated weights must give the same table within the bound tests/test_oracle.py holds the oracle's logits to."""
    from esm_amd.synth import synth_msa_state_dict
    from oracle.msa_oracle import msa_forward

    fix = torch.load(GOLDEN, weights_only=False)
    d = fix["dims"]
    alphabet = esm.Alphabet.from_architecture("msa_transformer")
    sd = synth_msa_state_dict(d["L"], d["E"], d["H"], d["F"], seed=d["seed"])
    chk = float(sum(v.double().sum() for k, v in sd.items() if k != "lm_head.weight"))
    assert abs(chk - fix["weights_checksum"]) < 1e-6 * max(1.0, abs(chk)), "synthetic weight generator drifted"
    _, _, toks = alphabet.get_batch_converter()(fix["msa"])
    assert torch.equal(toks, fix["tokens"]) and tuple(toks.shape) == (1, 8, 33)  # this tokeniser gives the reference's tokens
    table = []
    for i in range(toks.size(2)):
        masked = toks.clone()
        masked[0, 0, i] = alphabet.mask_idx
        table.append(torch.log_softmax(msa_forward(sd, masked, d["L"], d["H"])["logits"], dim=-1)[0, 0, i])
    table = torch.stack(table)
    assert table.shape == fix["masked_marginals"].shape == (33, len(alphabet))
    assert (table - fix["masked_marginals"]).abs().max() < 2e-5
    got = scoring.score_mutations(table, fix["msa"][0][1], fix["mutations"], alphabet, fix["offset_idx"])
    assert len(got) == len(fix["scores"]) >= 5
    for g, s in zip(got, fix["scores"]):
        assert abs(g - s) < 4e-5  # a difference of two table entries
    # the recorded scores are the recorded table's: label_row is score_mutations
    assert scoring.score_mutations(fix["masked_marginals"], fix["msa"][0][1], fix["mutations"], alphabet, fix["offset_idx"]) == fix["scores"]
