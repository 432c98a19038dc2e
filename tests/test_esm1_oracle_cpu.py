"""ESM-1 (arch "protein_bert_base") without a GPU: the CPU restatement tests/_esm1_oracle.py against the fixtures the
reference produced (tests/golden/make_golden_esm1.py), the module tree's state-dict keys against the reference's recorded
list, the checkpoint round trip through ``esm.pretrained``, and — where the reference package is present — a live
comparison against it."""
import os
import sys

import pytest
import torch

import esm
from _esm1_oracle import esm1_forward
from esm_amd.synth import esm1_args, synth_esm1_state_dict, write_esm1_checkpoint

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["tiny_d64", "mid_d64", "edges_d64"]
REFERENCE = "/root/reference"


def load_fixture(name):
    fix = torch.load(os.path.join(HERE, "golden", f"esm1_{name}.pt"), weights_only=False)
    fix["attentions"] = torch.load(os.path.join(HERE, "golden", f"esm1_{name}_attn.pt"), weights_only=False)["attentions"]
    return fix


def fixture_model_inputs(fix):
    d = fix["dims"]
    sd = synth_esm1_state_dict(d["L"], d["E"], d["H"], seed=d["seed"], final_bias=d["final_bias"])
    chk = float(sum(v.double().sum() for v in sd.values()))
    assert abs(chk - fix["weights_checksum"]) < 1e-6 * max(1.0, abs(chk)), "synthetic weight generator drifted"
    return d, sd


def test_fixtures_present_and_null_key_matters():
    for name in CASES:
        fix = load_fixture(name)
        assert fix["null_mass"] >= 0.05 and fix["null_removed_rel_l2"] >= 1e-2, name
    lens = load_fixture("edges_d64")["lengths"]
    assert lens == [64, 65, 128, 130]


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference_fixture(name):
    """The bounds tests/test_oracle.py holds the other restatements to."""
    fix = load_fixture(name)
    d, sd = fixture_model_inputs(fix)
    toks = fix["tokens"]
    out = esm1_forward(sd, toks, d["L"], d["H"], repr_layers=range(d["L"] + 1), return_contacts=True,
                       token_dropout=d["token_dropout"])
    real = toks.ne(1)
    assert (out["logits"][real] - fix["logits"]).abs().max() < 2e-5
    for layer, ref in fix["representations"].items():
        assert (out["representations"][layer][real] - ref).abs().max() < 2e-5, layer
    for b, n in enumerate(fix["lengths"]):
        assert (out["attentions"][b, :, :, :n, :n] - fix["attentions"][b]).abs().max() < 1e-6
        assert (out["contacts"][b, :n - 1, :n - 1] - fix["contacts"][b]).abs().max() < 2e-5
    # the recorded figure: without the null key the restatement is far from the reference
    off = esm1_forward(sd, toks, d["L"], d["H"], repr_layers=[d["L"]], token_dropout=d["token_dropout"], null_key=False)
    refL = fix["representations"][d["L"]]
    rel = ((off["representations"][d["L"]][real] - refL).norm() / refL.norm()).item()
    assert rel >= 1e-2 and abs(rel - fix["null_removed_rel_l2"]) < 1e-3 * rel


@pytest.mark.parametrize("name", CASES)
def test_module_tree_has_the_reference_state_dict_keys(name):
    fix = load_fixture(name)
    d, sd = fixture_model_inputs(fix)
    alphabet = esm.Alphabet.from_architecture("protein_bert_base")
    model = esm.ProteinBertModel(esm1_args(d["L"], d["E"], d["H"], d["final_bias"], d["token_dropout"]), alphabet)
    assert sorted(model.state_dict().keys()) == fix["state_dict_keys"]
    model.load_state_dict(sd, strict=True)
    assert model.model_version == "ESM-1" and model.num_layers == d["L"]
    assert model.embed_scale == d["E"] ** 0.5
    assert (model.embed_out_bias is not None) == d["final_bias"]
    assert (len(alphabet), alphabet.prepend_bos, alphabet.append_eos) == (35, True, False)


def test_checkpoint_round_trip_through_pretrained(tmp_path):
    path = write_esm1_checkpoint(str(tmp_path), "esm1_synth_t2", 2, 128, 2, seed=9, final_bias=True)
    model, alphabet = esm.pretrained.load_model_and_alphabet(path)
    assert isinstance(model, esm.ProteinBertModel) and model.model_version == "ESM-1"
    sd = synth_esm1_state_dict(2, 128, 2, seed=9, final_bias=True)
    got = model.state_dict()
    assert set(got) == set(sd)
    for k, v in sd.items():
        assert torch.equal(got[k], v), k
    assert len(alphabet) == 35
    for name in ("esm1_t34_670M_UR50S", "esm1_t34_670M_UR50D", "esm1_t34_670M_UR100", "esm1_t12_85M_UR50S", "esm1_t6_43M_UR50S"):
        assert callable(getattr(esm.pretrained, name))


def test_split_operand_modes_are_refused_in_python(monkeypatch):
    """ESM_AMD_OPERAND=f16x2* / f16x3 with an ESM-1 model: a Python error before esmk_create (no GPU involved)."""
    from esm_amd.esm2 import _Engine

    model = esm.ProteinBertModel(esm1_args(1, 128, 2), esm.Alphabet.from_architecture("protein_bert_base"))
    for mode, split in (("f16x2", 1), ("f16x2a", 2), ("f16x3", 4)):
        monkeypatch.setenv("ESM_AMD_OPERAND", mode)
        with pytest.raises(RuntimeError, match="ESM-1"):
            _Engine(model, torch.device("cpu"), torch.float16, split)
    monkeypatch.setenv("ESM_AMD_LN_FOLD", "1")
    assert model._fold_setting() == -1  # no LayerNorm fold for this family, whatever the environment asks


def test_c_abi_refuses_what_esm1_does_not_have():
    """esmk_create / the packed entries fail before any HIP call, naming ESM-1."""
    import ctypes

    from esm_amd import _native as N

    def create(**kw):
        f = dict(num_layers=2, embed_dim=128, num_heads=2, ffn_dim=512, vocab=35, pad_idx=1, mask_idx=33, cls_idx=32, eos_idx=2,
                 prepend_bos=1, operand_dtype=N.F16, no_rope=N.ESM1, ln_fold=-1)
        f.update(kw)
        h = ctypes.c_void_p()
        rc = N.lib.esmk_create(ctypes.byref(N.EsmkConfig(**f)), ctypes.byref(h))
        return rc, h, N.lib.esmk_last_error().decode()

    for kw, word in ((dict(ln_fold=1), "LayerNorm fold"), (dict(weight_split=1), "weight_split"), (dict(weight_split=4), "weight_split"),
                     (dict(num_heads=4), "head_dim 64"), (dict(num_positions=1026), "sinusoidal")):
        rc, h, msg = create(**kw)
        assert rc != 0 and "ESM-1" in msg and word in msg, (kw, msg)
    for bad in (N.ESM1_FINAL_BIAS, N.ESM1_FINAL_BIAS | 1, 3, 8, -1):  # final_bias without ESM-1, unknown values
        rc, _, msg = create(no_rope=bad)
        assert rc != 0 and "no_rope" in msg and "ESM-1" in msg, (bad, msg)
    rc, h, msg = create(no_rope=N.ESM1 | N.ESM1_FINAL_BIAS)
    assert rc == 0, msg
    N.lib.esmk_destroy(h)
    assert ctypes.sizeof(N.EsmkConfig) == 72  # the struct did not grow: the architecture rides in no_rope
    rc, h, msg = create(ln_fold=0)  # "the library's default" resolves to off
    assert rc == 0, msg
    try:
        assert N.lib.esmk_ln_fold_enabled(h) == 0
        plain, nbytes = ctypes.c_size_t(), ctypes.c_size_t()
        N.check(N.lib.esmk_packed_bytes(h, ctypes.byref(nbytes)))
        rc2, h2, _ = create(no_rope=1, ln_fold=-1)
        N.check(N.lib.esmk_packed_bytes(h2, ctypes.byref(plain)))
        N.lib.esmk_destroy(h2)
        # bias_k | bias_v per layer, embed_out and embed_out_bias (256-byte aligned carving)
        assert nbytes.value == plain.value + 2 * 512 + (35 * 128 * 2 + 255) // 256 * 256 + 256
        need = ctypes.c_size_t()
        seg = (ctypes.c_int32 * 2)(0, 64)
        assert N.lib.esmk_packed_workspace_bytes(h, 1, 64, 1, ctypes.byref(need)) != 0
        assert "ESM-1" in N.lib.esmk_last_error().decode()
        assert N.lib.esmk_packed_workspace_bytes_ex(h, seg, 1, 64, 1, ctypes.byref(need)) != 0
        assert "ESM-1" in N.lib.esmk_last_error().decode()
        one = ctypes.c_void_p(1)  # never dereferenced: the entry fails on the handle first
        assert N.lib.esmk_forward_packed(h, one, one, seg, 1, 64, None, 0, None, 1, one, one, 0, None) != 0
        assert "ESM-1" in N.lib.esmk_last_error().decode()
        assert N.lib.esmk_forward_packed_ex(h, one, one, seg, 1, 64, None, 0, None, 1, one, None, one, 0, None) != 0
        assert "ESM-1" in N.lib.esmk_last_error().decode()
    finally:
        N.lib.esmk_destroy(h)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "esm")), reason="the reference package is not on this machine")
def test_live_against_the_reference(tmp_path):
    """In a child process (the reference package has this package's import name): the reference's own ProteinBertModel on
    the synthetic weights against the restatement, its state-dict keys against the recorded list, and its loader on a
    checkpoint written by write_esm1_checkpoint."""
    import subprocess

    root = os.path.dirname(HERE)
    path = write_esm1_checkpoint(str(tmp_path), "esm1_synth_live", 2, 128, 2, seed=17, final_bias=True, token_dropout=True)
    code = f"""
import sys, torch
sys.path[:0] = [{REFERENCE!r}, {HERE!r}, {root!r}]
import esm
assert esm.__file__.startswith({REFERENCE!r}), esm.__file__
from _esm1_oracle import esm1_forward
from esm_amd.synth import synth_esm1_state_dict, synth_tokens
model, alphabet = esm.pretrained.load_model_and_alphabet({path!r})
model.eval()
assert type(model).__name__ == "ProteinBertModel" and model.model_version == "ESM-1"
fix = torch.load({os.path.join(HERE, 'golden', 'esm1_tiny_d64.pt')!r}, weights_only=False)
args = model.args
assert args.final_bias and args.token_dropout
sd = synth_esm1_state_dict(2, 128, 2, seed=17, final_bias=True)
assert sorted(model.state_dict().keys()) == sorted(set(fix["state_dict_keys"]) | {{"embed_out_bias"}})
toks = synth_tokens(3, 40, seed=4) + 0
toks[:, 0] = 32; toks[:, -1] = 5; toks[1, 30:] = 1; toks[0, 4] = 33
with torch.no_grad():
    ref = model(toks, repr_layers=[0, 1, 2], return_contacts=True)
out = esm1_forward(sd, toks, 2, 2, repr_layers=[0, 1, 2], return_contacts=True, token_dropout=True)
real = toks.ne(1)
assert (out["logits"] - ref["logits"])[real].abs().max() < 2e-5
for l in (0, 1, 2):
    assert (out["representations"][l] - ref["representations"][l])[real].abs().max() < 2e-5, l
assert (out["attentions"] - ref["attentions"]).abs().max() < 1e-6
assert (out["contacts"] - ref["contacts"]).abs().max() < 2e-5
print("live ok")
"""
    env = dict(os.environ, TORCH_FORCE_NO_WEIGHTS_ONLY_LOAD="1")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0 and "live ok" in r.stdout, r.stdout + r.stderr
