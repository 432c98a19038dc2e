"""Differential tests against the reference implementation itself, through the committed fixture
tests/golden/reference_probe.pt: tests/_reference_probe.py runs inside the reference (its package is also called
``esm``) and records what it computes for seeded random inputs — tokenisation, batching, FASTA parsing, model
forwards, checkpoint loading, module surfaces, and the result files of its unmodified scripts/extract.py.  Regenerate
the fixture with that script where a checkout of the reference exists; these tests need only the repository.
This process then compares
  * the host side (esm_amd.Alphabet / BatchConverter / MSABatchConverter / FastaBatchedDataset.get_batch_indices /
    read_fasta) — integer work, bit-exact — with reference esm/data.py:19-378;
  * the oracles (oracle/esm2_oracle.py, esm1b_oracle.py, msa_oracle.py) with reference ESM2 / ProteinBertModel /
    MSATransformer forwards on synthetic weights at dims and seeds that are NOT among the committed fixtures
    (head dims 24 / 32 / 128, other depths), to <= 2e-5: a second pin of the oracle, independent of the fixtures
    the model tests use.
"""
import os
import subprocess
import sys

import pytest
import torch

import _reference_probe as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(P.FIXTURE), f"{P.FIXTURE} missing: regenerate with tests/_reference_probe.py"
    return torch.load(P.FIXTURE, weights_only=False)


def test_tokenizer_and_batch_converter_bit_exact(probe):
    import esm

    for arch, cases in probe["alphabet"].items():
        a = esm.Alphabet.from_architecture(arch)
        assert a.all_toks == cases["all_toks"], arch
        assert (a.padding_idx, a.cls_idx, a.eos_idx, a.unk_idx, a.mask_idx) == cases["ids"], arch
        assert (a.prepend_bos, a.append_eos) == cases["bos_eos"], arch
        for s, want in cases["encode"]:
            assert a.encode(s) == want, (arch, s)
        for s, want in cases["tokenize"]:
            assert a.tokenize(s) == want, (arch, s)
        for trunc, batch, (labels, strs, toks) in cases["batches"]:
            got = a.get_batch_converter(trunc)(batch)
            assert got[0] == labels and got[1] == strs, (arch, trunc)
            assert got[2].dtype == torch.int64 and torch.equal(got[2], toks), (arch, trunc)
        for s in cases["raises"]:
            with pytest.raises(KeyError):
                a.encode(s)


def test_msa_batch_converter_bit_exact(probe):
    import esm

    a = esm.Alphabet.from_architecture("msa_transformer")
    conv = a.get_batch_converter()
    for inp, (labels, strs, toks) in probe["msa_batches"]:
        got = conv(inp)
        assert got[0] == labels and got[1] == strs and torch.equal(got[2], toks)
    with pytest.raises(RuntimeError, match="unaligned"):
        conv([("a", "MKT"), ("b", "MK")])


def test_fasta_dataset_and_batching_bit_exact(probe, tmp_path):
    import esm

    for text, toks_per_batch, extra, (labels, seqs, batches) in probe["fasta"]:
        f = tmp_path / "x.fasta"
        f.write_text(text)
        ds = esm.FastaBatchedDataset.from_file(f)
        assert list(ds.sequence_labels) == labels and list(ds.sequence_strs) == seqs
        assert ds.get_batch_indices(toks_per_batch, extra_toks_per_seq=extra) == batches
    for text, kw, rows in probe["read_fasta"]:
        f = tmp_path / "x.a3m"
        f.write_text(text)
        assert list(esm.data.read_fasta(str(f), **kw))[:len(rows)] == rows, kw


def _close(a, b, tol, mask=None):
    d = (a - b).abs()
    if mask is not None:
        d = d[mask]
    return d.numel() == 0 or d.max().item() <= tol


def test_esm2_oracle_matches_live_reference(probe):
    from esm_amd.synth import synth_esm2_state_dict
    from oracle.esm2_oracle import esm2_forward

    for c in probe["esm2"]:
        sd = synth_esm2_state_dict(c["L"], c["E"], c["H"], seed=c["seed"])
        out = esm2_forward(sd, c["tokens"], c["L"], c["H"], repr_layers=range(c["L"] + 1), return_contacts=True)
        nonpad = c["tokens"].ne(1)
        tag = (c["L"], c["E"], c["H"])
        assert _close(out["logits"], c["logits"], 2e-5, nonpad), tag
        for l, ref in c["representations"].items():
            assert _close(out["representations"][l], ref, 2e-5, nonpad), (tag, l)
        assert _close(out["attentions"], c["attentions"], 2e-6), tag
        assert _close(out["contacts"], c["contacts"], 2e-5), tag


def test_esm1b_oracle_matches_live_reference(probe):
    from esm_amd.synth import synth_esm1b_state_dict
    from oracle.esm1b_oracle import esm1b_forward

    for c in probe["esm1b"]:
        sd = synth_esm1b_state_dict(c["L"], c["E"], c["H"], seed=c["seed"], ln_before=c["ln_before"])
        out = esm1b_forward(sd, c["tokens"], c["L"], c["H"], repr_layers=range(c["L"] + 1))
        nonpad = c["tokens"].ne(1)
        assert _close(out["logits"], c["logits"], 2e-5, nonpad)
        for l, ref in c["representations"].items():
            assert _close(out["representations"][l], ref, 2e-5, nonpad), l


def test_msa_oracle_matches_live_reference(probe):
    from esm_amd.synth import synth_msa_state_dict
    from oracle.msa_oracle import msa_forward

    for c in probe["msa"]:
        sd = synth_msa_state_dict(c["L"], c["E"], c["H"], c["F"], seed=c["seed"])
        out = msa_forward(sd, c["tokens"], c["L"], c["H"], repr_layers=range(c["L"] + 1), return_contacts=True)
        nonpad = c["tokens"].ne(1)
        assert _close(out["logits"], c["logits"], 5e-5, nonpad)
        for l, ref in c["representations"].items():
            assert _close(out["representations"][l], ref, 5e-5, nonpad), l
        assert _close(out["row_attentions"], c["row_attentions"], 5e-6)
        assert _close(out["contacts"], c["contacts"], 5e-5)


def _check_result_file(got, ref, layers, tol, tag):
    """A result file written here against the reference's, as the fixture stores it (tests/_reference_probe.py
    slim_result_file): label and keys; mean and <bos> representations whole; per-token representations and the contact map
    by shape and dtype, their values on the rows per_tok_rows() keeps."""
    assert got["label"] == ref["label"] and sorted(got) == ref["keys"], tag
    for key in ("mean_representations", "bos_representations"):
        assert sorted(got[key]) == sorted(ref[key]) == layers, (tag, key)
        for l in ref[key]:
            assert got[key][l].shape == ref[key][l].shape and got[key][l].dtype == ref[key][l].dtype, (tag, key, l)
            assert (got[key][l] - ref[key][l]).abs().max().item() < tol, (tag, key, l)
    assert sorted(got["representations"]) == sorted(ref["per_tok_shape"]) == layers, tag
    for l, t in got["representations"].items():
        assert tuple(t.shape) == ref["per_tok_shape"][l] and t.dtype == ref["per_tok_dtype"][l], (tag, l)
        assert (t[P.per_tok_rows(t.shape[0])] - ref["per_tok_rows"][l]).abs().max().item() < tol, (tag, l)
    c = got["contacts"]
    assert tuple(c.shape) == ref["contacts_shape"] and c.dtype == ref["contacts_dtype"], tag
    assert (c[P.per_tok_rows(c.shape[0])] - ref["contacts_rows"]).abs().max().item() < tol, tag


def test_reference_extract_script_runs_unmodified_against_the_shim(probe, tmp_path):
    """BASELINE configs[0]: the result files of the reference's unmodified scripts/extract.py (8M dims, the reference's
    examples FASTA, --nogpu), recorded in the fixture (per-token and contact-map rows at a stride), against the same call
    sequence on this repo's ``esm`` package (tests/_extract_replay.py, each step citing the script's line).  The shim run
    has the engine replaced by the oracle inside the test launcher only (tests/_run_reference_script.py): the product has
    no CPU path.  Same files, same labels, same keys, shapes and dtypes, values to oracle precision."""
    from esm_amd.synth import write_esm2_checkpoint

    case, rec = P.EXTRACT_CASES["few_proteins_8M"], probe["extract"]["few_proteins_8M"]
    name, L, E, H, seed = case["ckpt"]
    ckpt = write_esm2_checkpoint(str(tmp_path), name, L, E, H, seed=seed)
    fasta = tmp_path / "few_proteins.fasta"
    fasta.write_text(rec["fasta"])
    out_dir = tmp_path / "shim"
    cmd = [sys.executable, os.path.join(ROOT, "tests", "_run_reference_script.py"), os.path.join(ROOT, "tests", "_extract_replay.py"),
           ckpt, str(fasta), str(out_dir)] + case["args"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=900,
                       env=dict(os.environ, PYTHONPATH=ROOT, TORCH_FORCE_NO_WEIGHTS_ONLY_LOAD="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    outs = {"ref": rec["files"],
            "shim": {str(p.relative_to(out_dir)): torch.load(p, weights_only=False) for p in sorted(out_dir.rglob("*.pt"))}}
    assert outs["ref"] and sorted(outs["ref"]) == sorted(outs["shim"])
    for name, ref in outs["ref"].items():
        _check_result_file(outs["shim"][name], ref, [0, 5, 6], 5e-5, name)


def test_reference_own_alphabet_tests_pass_on_our_alphabets(probe):
    """The batches of the reference's OWN alphabet tests (tests/test_alphabet.py:6-45, plain and truncated at 10) through
    this repo's Alphabet objects give what the reference's alphabets gave (recorded in the fixture); their public
    wrappers download checkpoints just to get an alphabet, which ``Alphabet.from_architecture`` provides offline
    (esm/pretrained.py:87-127 picks the same names)."""
    import esm

    for arch in ("ESM-1b", "roberta_large"):  # esm1b_t33_650M_UR50S / esm1v_t33_650M_UR90S_* use this alphabet
        a = esm.Alphabet.from_architecture(arch)
        cases = probe["alphabet_tests"][arch]
        assert [(t, b) for t, b, _ in cases] == P.ALPHABET_TEST_BATCHES
        for trunc, batch, (labels, strs, toks) in cases:
            got = a.get_batch_converter(trunc)(batch)
            assert got[0] == labels and got[1] == strs, (arch, trunc)
            assert got[2].dtype == toks.dtype and torch.equal(got[2], toks), (arch, trunc)


def test_checkpoint_loading_matches_reference(probe, tmp_path):
    """esm.pretrained.load_model_and_alphabet on checkpoint FILES in the released formats (ESM-2 cfg format;
    ESM-1b / MSA Transformer fairseq-args formats with encoder_* argument names, encoder.sentence_encoder.* key
    prefixes, the row/column key swap of the MSA files, sibling -contact-regression.pt): same model class name, same
    alphabet, same state-dict keys, bit-identical tensors (dtype, shape, SHA-256 of the bytes) as the reference's loader
    (esm/pretrained.py:52-221) produced from the same files."""
    import esm
    from esm_amd import synth

    paths = P.write_checkpoints(str(tmp_path / "ckpt"), synth)
    assert [os.path.basename(p) for p in paths] == [c["name"] for c in probe["checkpoints"]] and len(paths) == 3
    for path, c in zip(paths, probe["checkpoints"]):
        model, alphabet = esm.pretrained.load_model_and_alphabet(path)
        assert type(model).__name__ == c["cls"], c["name"]
        assert list(alphabet.all_toks) == c["all_toks"] and model.num_layers == c["num_layers"]
        got = model.state_dict()
        assert sorted(got) == sorted(c["state"]), set(got) ^ set(c["state"])
        for k, v in c["state"].items():
            assert P.tensor_digest(got[k]) == v, (c["name"], k)


def test_module_surface_matches_reference(probe):
    """What callers poke at on the nn.Module (scripts/extract.py:65-84, esmfold.py:61-67, the FSDP example wrapping
    ``model.layers``): child-module names and order, state-dict key order and shapes, parameter / buffer names,
    parameter count, the scalar attributes — identical to a freshly constructed reference ESM2 (esm2.py:15-75)."""
    import esm

    ref = probe["surface"]["esm2_8M"]
    m = esm.ESM2(6, 320, 20)
    assert [n for n, _ in m.named_children()] == ref["children"]
    assert list(m.state_dict().keys()) == ref["state_keys"]
    assert [n for n, _ in m.named_parameters()] == ref["param_names"]
    assert [n for n, _ in m.named_buffers()] == ref["buffer_names"]
    assert sum(p.numel() for p in m.parameters()) == ref["n_params"]
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == ref["shapes"]
    assert [n for n, _ in m.layers[0].named_children()] == ref["layer_children"]
    for a, v in ref["attrs"].items():
        assert getattr(m, a) == v, a
    d = esm.ESM2(num_layers=1)
    for a, v in probe["surface"]["esm2_default"]["attrs"].items():
        assert getattr(d, a) == v, a


def _check_surface(m, ref):
    assert [n for n, _ in m.named_children()] == ref["children"]
    assert list(m.state_dict().keys()) == ref["state_keys"]
    assert [n for n, _ in m.named_parameters()] == ref["param_names"]
    assert [n for n, _ in m.named_buffers()] == ref["buffer_names"]
    assert sum(p.numel() for p in m.parameters()) == ref["n_params"]
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == ref["shapes"]
    assert [n for n, _ in m.layers[0].named_children()] == ref["layer_children"]
    for a, v in ref["attrs"].items():
        assert getattr(m, a) == v, a


def test_msa_and_esm1b_module_surface_matches_reference(probe):
    """Same check for MSATransformer (msa_transformer.py:20-144) and ProteinBertModel / ESM-1b (esm1.py:20-115)."""
    import argparse

    import esm

    msa_args = argparse.Namespace(layers=2, embed_dim=96, ffn_embed_dim=192, attention_heads=3, dropout=0.1,
                                  attention_dropout=0.1, activation_dropout=0.1, max_positions=1024,
                                  embed_positions_msa=True, embed_positions_msa_dim=96, max_tokens=2 ** 14,
                                  max_tokens_per_msa=2 ** 14)
    _check_surface(esm.MSATransformer(msa_args, esm.Alphabet.from_architecture("msa_transformer")), probe["surface"]["msa"])
    b_args = argparse.Namespace(arch="roberta_large", layers=2, embed_dim=96, ffn_embed_dim=384, attention_heads=3,
                                max_positions=1024, token_dropout=True, emb_layer_norm_before=True)
    _check_surface(esm.ProteinBertModel(b_args, esm.Alphabet.from_architecture("roberta_large")), probe["surface"]["esm1b"])


def test_alphabet_object_and_dataset_edge_cases(probe, tmp_path):
    """Attributes and small methods of Alphabet for all five architectures the reference names (data.py:91-176), the
    error for an unknown architecture, FastaBatchedDataset indexing, the duplicate-label check of from_file
    (data.py:52-55) and a batch holding an empty string."""
    import esm

    for arch, ref in probe["alphabet_surface"].items():
        if arch == "_invalid":
            continue
        a = esm.Alphabet.from_architecture(arch)
        for f, v in ref["fields"].items():
            assert getattr(a, f) == v, (arch, f)
        assert len(a) == ref["length"] and a.to_dict() == ref["to_dict"]
        assert [(t, a.get_idx(t)) for t, _ in ref["get_idx"]] == ref["get_idx"], arch
        assert [(i, a.get_tok(i)) for i, _ in ref["get_tok"]] == ref["get_tok"], arch
        assert type(a.get_batch_converter()).__name__ == ref["converter"], arch
    with pytest.raises(Exception) as ei:
        esm.Alphabet.from_architecture("no_such_arch")
    assert type(ei.value).__name__ == probe["alphabet_surface"]["_invalid"]
    ds = esm.FastaBatchedDataset(["a", "b", "c"], ["MKT", "MKTVRQG", "M"])
    ref = probe["dataset"]
    assert len(ds) == ref["length"] and [ds[i] for i in range(3)] == ref["items"]
    assert ds.get_batch_indices(8, 1) == ref["batches"]
    f = tmp_path / "dup.fasta"
    f.write_text(">x\nMK\n>x\nMKT\n")
    with pytest.raises(Exception) as ei:
        esm.FastaBatchedDataset.from_file(f)
    assert (type(ei.value).__name__, str(ei.value)) == ref["duplicate_labels"]
    a = esm.Alphabet.from_architecture("ESM-1b")
    labels, strs, toks = a.get_batch_converter()([("e", ""), ("f", "MK")])
    assert (labels, strs) == ref["empty_string_batch"][:2] and torch.equal(toks, ref["empty_string_batch"][2])


def test_binding_stub_reads_the_real_reference_class(probe):
    """examples/reference_binding/_esmk.py configured from the attributes an instance of the REFERENCE's ESM2 carries
    (esm2.py:24-38, recorded in the fixture): esmk_create accepts it and plans the same packed image as for this repo's
    class."""
    import ctypes
    import importlib.util
    import types

    import esm
    from esm_amd import _native

    spec = importlib.util.spec_from_file_location("ref_esmk_stub", os.path.join(ROOT, "examples", "reference_binding", "_esmk.py"))
    stub = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(stub)
    L_ = stub.lib(_native.LIB_PATH)
    ref = probe["binding_attrs"]
    scfg = stub.config_for(types.SimpleNamespace(**ref["attrs"]))  # reads the attributes the reference's ESM2.__init__ sets
    h, n_ref = ctypes.c_void_p(), ctypes.c_size_t()
    assert L_.esmk_create(ctypes.byref(scfg), ctypes.byref(h)) == 0
    L_.esmk_packed_bytes(h, ctypes.byref(n_ref))
    L_.esmk_destroy(h)
    m = esm.ESM2(6, 320, 20)
    cfg = _native.EsmkConfig(6, 320, 20, 1280, m.alphabet_size, m.padding_idx, m.mask_idx, m.cls_idx, m.eos_idx, 1, 1, 1,
                             _native.dtype_code(torch.float16), 0, 0, 0)
    assert [getattr(scfg, f[0]) for f in stub.Config._fields_] == [getattr(cfg, f[0]) for f in _native.EsmkConfig._fields_]
    h, n = ctypes.c_void_p(), ctypes.c_size_t()
    _native.check(_native.lib.esmk_create(ctypes.byref(cfg), ctypes.byref(h)))
    _native.check(_native.lib.esmk_packed_bytes(h, ctypes.byref(n)))
    _native.lib.esmk_destroy(h)
    assert n.value == n_ref.value
    assert ref["state_keys"] == list(m.state_dict())  # every key esmk_pack_weight will be handed


def test_extraction_driver_writes_the_files_the_reference_script_writes(probe, tmp_path):
    """esm_amd.extract.extract (the sharded driver; here one rank on CPU with the oracle as its embed_fn — test
    infrastructure, the product's embed_fn is the engine) against the result files of the reference's scripts/extract.py
    run on a checkpoint with the same weights and the same FASTA (recorded in the fixture, rows at a stride as above): the
    same set of <label>.pt files, the same keys, dtypes and shapes, truncation at --truncation_seq_length, values to
    oracle precision."""
    import pathlib

    import esm
    from esm_amd.extract import extract
    from esm_amd.synth import synth_esm2_state_dict
    from oracle.esm2_oracle import esm2_forward

    case, rec = P.EXTRACT_CASES["tiny_truncated"], probe["extract"]["tiny_truncated"]
    _, L, E, H, seed = case["ckpt"]
    assert (L, E, H, seed) == (3, 128, 2, 17) and "--truncation_seq_length" in case["args"]
    assert rec["fasta"] == P.tiny_truncated_fasta()
    fasta = tmp_path / "in.fasta"
    fasta.write_text(rec["fasta"])

    sd = synth_esm2_state_dict(L, E, H, seed=seed)
    alphabet = esm.Alphabet.from_architecture("ESM-1b")
    ds = esm.FastaBatchedDataset.from_file(fasta)

    def embed_fn(toks, layers, return_contacts):
        return esm2_forward(sd, toks, L, H, repr_layers=layers, return_contacts=return_contacts)

    extract(ds, alphabet, embed_fn, L, E, [-1, 1], ["mean", "per_tok", "bos", "contacts"],
            output_dir=pathlib.Path(tmp_path / "ours"), toks_per_batch=150, truncation_seq_length=40, device=None,
            gather_mean=False, log=lambda s: None)
    ref_files = sorted(rec["files"])
    our_files = sorted(str(p.relative_to(tmp_path / "ours")) for p in (tmp_path / "ours").rglob("*.pt"))
    assert ref_files == our_files and len(ref_files) == 5
    for rel in ref_files:
        _check_result_file(torch.load(tmp_path / "ours" / rel, weights_only=False), rec["files"][rel], [1, L], 5e-5, rel)
