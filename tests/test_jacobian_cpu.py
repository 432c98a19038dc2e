"""The host side of the categorical Jacobian without a GPU: the argument checks of the five C entries (refused before any HIP
call, on fake pointers as in tests/test_c_abi_validation_cpu.py), the fp64 references of tests/_jacobian_ref.py against closed
forms, the candidate list, the refusals of the Python layer and the command line."""
import argparse
import ctypes

import pytest
import torch

import _jacobian_ref as R
import esm
from esm_amd import _native as N
from esm_amd import jacobian

FAKE = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused first


def err():
    return N.lib.esmk_last_error().decode()


# ---- the C entries refuse bad arguments before any HIP call -----------------------------------------------------------------
def test_substitute_rows_argument_checks():
    def s(tokens=FAKE, src=None, pos=FAKE, tok=FAKE, out=FAKE, B=1, T=25, n=7, V=33):
        return N.lib.esmk_op_substitute_rows(tokens, src, pos, tok, out, B, T, n, V, None)

    for kw in (dict(tokens=None), dict(pos=None), dict(tok=None), dict(out=None)):
        assert s(**kw) != 0 and err() == "esmk_op_substitute_rows: null argument", kw
    for kw in (dict(B=0), dict(T=0), dict(n=0), dict(V=0), dict(n=-3), dict(V=-1)):
        assert s(**kw) != 0 and "esmk_op_substitute_rows: B, T, n and V must be positive" in err(), kw
    for kw in (dict(B=2 ** 12, T=2 ** 13), dict(n=2 ** 14, T=1025)):
        assert s(**kw) != 0 and "2^24" in err(), kw


def test_jacobian_scatter_argument_checks():
    def s(logits=FAKE, wt=FAKE, cols=FAKE, out=FAKE, n=7, L=23, nA=20, V=33):
        return N.lib.esmk_op_jacobian_scatter(logits, wt, cols, out, n, L, nA, V, None)

    for kw in (dict(logits=None), dict(wt=None), dict(cols=None), dict(out=None)):
        assert s(**kw) != 0 and err() == "esmk_op_jacobian_scatter: null argument", kw
    for kw in (dict(n=0), dict(V=0), dict(n=-1)):
        assert s(**kw) != 0 and "n_copies and V must be positive" in err(), kw
    for kw in (dict(L=0), dict(nA=0), dict(L=-2)):
        assert s(**kw) != 0 and "L and nA must be positive" in err(), kw
    assert s(nA=33) != 0 and "nA must be in 1 .. 32" in err()
    assert s(n=461) != 0 and "more copies than L*nA" in err()
    assert s(L=2 ** 20, nA=1) != 0 and "2^40" in err()  # L*nA*L*nA = 2^40
    assert s(L=2 ** 20, nA=32) != 0 and "2^24 copies" in err()
    assert s(n=2 ** 12, L=2 ** 13, nA=1) != 0 and "n_copies*L exceeds 2^24 rows" in err()


def test_center_contacts_and_apc_argument_checks():
    center, contacts, apc = N.lib.esmk_op_jacobian_center, N.lib.esmk_op_jacobian_contacts, N.lib.esmk_op_apc
    assert center(None, 23, 20, None) != 0 and err() == "esmk_op_jacobian_center: null argument"
    for a, b in ((None, FAKE), (FAKE, None)):
        assert contacts(a, b, 23, 20, None) != 0 and err() == "esmk_op_jacobian_contacts: null argument"
        assert apc(a, b, 23, None) != 0 and err() == "esmk_op_apc: null argument"
    for name, call in (("esmk_op_jacobian_center", lambda L, nA: center(FAKE, L, nA, None)),
                       ("esmk_op_jacobian_contacts", lambda L, nA: contacts(FAKE, FAKE, L, nA, None))):
        for L, nA, msg in ((0, 20, "L and nA must be positive"), (23, 0, "L and nA must be positive"), (-1, 20, "must be positive"),
                           (23, 33, "nA must be in 1 .. 32"), (2 ** 20, 1, "2^40"), (2 ** 15, 32, "2^40"),
                           (2 ** 24, 2, "2^24 copies")):
            assert call(L, nA) != 0 and err().startswith(name) and msg in err(), (name, L, nA, err())
    for L in (0, -5):
        assert apc(FAKE, FAKE, L, None) != 0 and "esmk_op_apc: L must be positive" in err()
    assert apc(FAKE, FAKE, 2 ** 24 + 1, None) != 0 and "2^24" in err()


# ---- the references ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,nA", [(1, 1), (1, 20), (5, 1), (7, 3), (11, 20)])
def test_sequential_centring_equals_the_projection(L, nA):
    J = torch.randn((L, nA, L, nA), generator=torch.Generator().manual_seed(L + nA), dtype=torch.float32) + 10.0
    seq, ms = R.center_ref(J)
    closed = R.center_closed_form(J)
    scale = J.double().abs().max().item()
    assert (seq - closed).abs().max().item() <= 64 * 2.0 ** -52 * scale  # fp64 round-off of two orders of the same sums
    assert len(ms) == 4 and all(m >= 0 for m in ms)
    for axis in range(4):  # a projection: every mean is gone, and doing it again changes nothing
        assert seq.mean(dim=axis).abs().max().item() <= 64 * 2.0 ** -52 * scale
    again, _ = R.center_ref(seq)
    assert (again - seq).abs().max().item() <= 64 * 2.0 ** -52 * scale
    assert R.center_bound([1.0, 1.0, 1.0, 1.0]) == 15 * 2.0 ** -24


def test_contact_references_on_known_answers():
    L, nA = 3, 2
    J = torch.zeros((L, nA, L, nA), dtype=torch.float64)
    J[0, :, 1, :] = torch.tensor([[3.0, 0.0], [0.0, 0.0]])
    J[1, :, 0, :] = torch.tensor([[5.0, 0.0], [0.0, 0.0]])  # the block of (1, 0), transposed, meets the one of (0, 1)
    J[0, 1, 2, 0] = 2.0                                     # pairs with J[2, 0, 0, 1] = 0
    S = R.contacts_ref(J)
    assert torch.equal(S, S.t())
    assert S[0, 1].item() == 4.0 and S[0, 2].item() == 1.0 and S[1, 2].item() == 0.0
    C = R.apc_ref(S)
    r = torch.tensor([5.0, 4.0, 1.0], dtype=torch.float64)
    want = torch.tensor([[0.0, 4.0, 1.0], [4.0, 0.0, 0.0], [1.0, 0.0, 0.0]], dtype=torch.float64) - r[:, None] * r[None, :] / 10.0
    want.fill_diagonal_(0.0)
    assert torch.allclose(C, want, rtol=0, atol=1e-15)
    zero = R.apc_ref(torch.zeros((4, 4)))
    assert bool((zero == 0).all())  # s == 0: no 0 / 0


# ---- the Python layer -------------------------------------------------------------------------------------------------------
def test_candidate_columns():
    model = esm.ESM2(1, 128, 2)
    a = model.alphabet
    std = jacobian.candidate_columns(model)
    assert std == [a.get_idx(r) for r in "ACDEFGHIKLMNPQRSTVWY"] and len(set(std)) == 20
    assert jacobian.candidate_columns(model, "VGA") == [a.get_idx("V"), a.get_idx("G"), a.get_idx("A")]  # the order given
    assert jacobian.candidate_columns(model, [5, 7]) == [5, 7]
    assert len(jacobian.candidate_columns(model, range(32))) == 32
    for bad in ("", [], "A?", [99], [-1], "AGA", [5, 5], range(33)):
        with pytest.raises(ValueError):
            jacobian.candidate_columns(model, bad)


def test_refusals_without_a_gpu():
    args = argparse.Namespace(layers=1, embed_dim=64, ffn_embed_dim=128, attention_heads=2, dropout=0.1, attention_dropout=0.1,
                              activation_dropout=0.1, max_positions=1024, embed_positions_msa=True, embed_positions_msa_dim=64,
                              max_tokens=2 ** 14, max_tokens_per_msa=2 ** 14)
    msa = esm.MSATransformer(args, esm.Alphabet.from_architecture("msa_transformer"))
    toks = torch.zeros((1, 2, 8), dtype=torch.int64)
    for call in (lambda: msa.categorical_jacobian(toks), lambda: msa.jacobian_contacts(toks),
                 lambda: jacobian.categorical_jacobian(msa, toks), lambda: jacobian.jacobian_contacts(msa, toks)):
        with pytest.raises(NotImplementedError, match="MSA Transformer"):
            call()
    model = esm.ESM2(1, 128, 2)
    with pytest.raises(ValueError, match="ONE sequence"):
        model.categorical_jacobian(torch.tensor([[0, 5, 2], [0, 6, 2]]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.categorical_jacobian(torch.tensor([[0, 5, 2]]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.jacobian_contacts(torch.tensor([0, 5, 2]))
    import esm_amd

    assert esm_amd.categorical_jacobian is jacobian.categorical_jacobian
    assert callable(esm_amd.jacobian_contacts)


# ---- the command line -------------------------------------------------------------------------------------------------------
def test_cli_parsing_and_output_names(tmp_path):
    import importlib

    import esm_amd

    cli = importlib.import_module("esm_amd.jacobian_contacts")  # the module (it forwards calls to the function of that name)
    a = cli.parse_args(["--model-location", "m.pt", "--sequence", "MKTAY", "--output-dir", str(tmp_path)])
    assert (a.sequence, a.fasta, a.save_jacobian, a.allowed, a.chunk) == ("MKTAY", None, False, None, None)
    assert cli.read_records(a) == [("sequence", "MKTAY")]
    a = cli.parse_args(["--model-location", "m.pt", "--fasta", "in.fasta", "--output-dir", "out", "--save-jacobian", "--allowed",
                        "AGV", "--chunk", "7"])
    assert (str(a.fasta), str(a.output_dir), a.save_jacobian, a.allowed, a.chunk) == ("in.fasta", "out", True, "AGV", 7)
    base = ["--model-location", "m.pt", "--output-dir", "out"]
    for bad in (base, base + ["--sequence", "MK", "--fasta", "x"], base + ["--sequence", "MK", "--allowed", ""],
                base + ["--sequence", "MK", "--allowed", "AGA"], base + ["--sequence", "MK", "--chunk", "0"],
                ["--model-location", "m.pt", "--sequence", "MK"], ["--sequence", "MK", "--output-dir", "out"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    contacts, jac = cli.output_paths(tmp_path, "sp|P12345|NAME some description", save_jacobian=True)
    assert contacts == tmp_path / "sp_P12345_NAME.contacts.npy" and jac == tmp_path / "sp_P12345_NAME.jacobian.npy"
    assert cli.output_paths("out", "protein-1.a")[0].name == "protein-1.a.contacts.npy" and cli.output_paths("out", "x")[1] is None
    assert cli.output_paths("out", "")[0].name == "sequence.contacts.npy"
    fasta = tmp_path / "in.fasta"
    fasta.write_text(">a first\nMKT\nAY\n>b\nGG\n")
    a = cli.parse_args(["--model-location", "m.pt", "--fasta", str(fasta), "--output-dir", str(tmp_path)])
    assert [(label.split()[0], seq) for label, seq in cli.read_records(a)] == [("a", "MKTAY"), ("b", "GG")]
    # importing the module rebinds the package attribute; calls still reach the function
    assert callable(esm_amd.jacobian_contacts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        esm_amd.jacobian_contacts(esm.ESM2(1, 128, 2), torch.tensor([[0, 5, 2]]))


def test_cli_refuses_an_msa_model(tmp_path, monkeypatch):
    import importlib

    from esm_amd import pretrained

    cli = importlib.import_module("esm_amd.jacobian_contacts")
    args = argparse.Namespace(layers=1, embed_dim=64, ffn_embed_dim=128, attention_heads=2, dropout=0.1, attention_dropout=0.1,
                              activation_dropout=0.1, max_positions=1024, embed_positions_msa=True, embed_positions_msa_dim=64,
                              max_tokens=2 ** 14, max_tokens_per_msa=2 ** 14)
    alphabet = esm.Alphabet.from_architecture("msa_transformer")
    monkeypatch.setattr(pretrained, "load_model_and_alphabet", lambda location: (esm.MSATransformer(args, alphabet), alphabet))
    with pytest.raises(SystemExit, match="MSA Transformer"):
        cli.main(["--model-location", "msa.pt", "--sequence", "MKTAY", "--output-dir", str(tmp_path / "out")])
    assert not (tmp_path / "out").exists()
