"""The original ESM-1 models (esm.ProteinBertModel, arch "protein_bert_base": sinusoidal positions, bias_kv attention,
untied output projection) on the MI355X engine: parity against fixtures produced by the reference
(tests/golden/make_golden_esm1.py) and against the CPU restatement (tests/_esm1_oracle.py) at the t34 dimensions.
Mirrors tests/test_esm1b_gpu.py; bounds as there: representation 0 within 1e-5 relative, every other representation and
the logits under the one contract (tests/_contract.py) against the plain-form fp16 floor, attentions 3e-3, contacts 5e-3."""
import pytest
import torch

import _contract as C
import esm
from _esm1_oracle import esm1_forward
from esm_amd.synth import esm1_args, synth_esm1_state_dict, synth_tokens
from test_esm1_oracle_cpu import CASES, fixture_model_inputs, load_fixture

pytestmark = pytest.mark.gpu
PAD, CLS, MASK = 1, 32, 33


def rel_err(a, b, mask=None):
    if mask is not None:
        a, b = a[mask], b[mask]
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def build(L, E, H, seed, final_bias=False, token_dropout=False):
    sd = synth_esm1_state_dict(L, E, H, seed=seed, final_bias=final_bias)
    model = esm.ProteinBertModel(esm1_args(L, E, H, final_bias, token_dropout),
                                 esm.Alphabet.from_architecture("protein_bert_base")).eval()
    model.load_state_dict(sd, strict=True)
    return model.cuda(), sd


def floor_of(model, sd, toks, L, H, **kw):
    """The fp16 / bf16 operand floor in the plain form (ESM-1 has no LayerNorm fold; C.floor_forward asks the model)."""
    assert model.ln_fold_active() is False
    return C.floor_forward(sd, toks, L, H, model=model, forward=esm1_forward, **kw)


@pytest.mark.parametrize("name", CASES)
def test_esm1_engine_matches_reference_fixture(name):
    fix = load_fixture(name)
    d, sd = fixture_model_inputs(fix)
    L, H = d["L"], d["H"]
    model, _ = build(L, d["E"], H, d["seed"], d["final_bias"], d["token_dropout"])
    toks = fix["tokens"]
    with torch.no_grad():
        out = model(toks.cuda(), repr_layers=list(range(L + 1)), return_contacts=True)
    real = toks.ne(PAD)
    floor = floor_of(model, sd, toks, L, H, repr_layers=list(range(L + 1)), token_dropout=d["token_dropout"])
    for layer, ref in fix["representations"].items():
        got = out["representations"][layer].cpu()[real]
        if layer == 0:
            assert rel_err(got, ref) < 1e-5
            continue
        C.check_tensors(f"esm1_{name} repr[{layer}]", got, ref, floor["representations"][layer][real])
    C.check_tensors(f"esm1_{name} logits", out["logits"].cpu()[real], fix["logits"], floor["logits"][real])
    attn, contacts = out["attentions"].cpu(), out["contacts"].cpu()
    assert attn.shape == (toks.shape[0], L, H, toks.shape[1], toks.shape[1])
    assert contacts.shape == (toks.shape[0], toks.shape[1] - 1, toks.shape[1] - 1)  # the (1, 0) crop: BOS only
    for b, n in enumerate(fix["lengths"]):
        print(f"\nesm1_{name} seq {b}: attentions max err {(attn[b, :, :, :n, :n] - fix['attentions'][b]).abs().max().item():.2e}, "
              f"contacts max err {(contacts[b, :n - 1, :n - 1] - fix['contacts'][b]).abs().max().item():.2e}")
        assert (attn[b, :, :, :n, :n] - fix["attentions"][b]).abs().max().item() < 3e-3
        assert (contacts[b, :n - 1, :n - 1] - fix["contacts"][b]).abs().max().item() < 5e-3
    # maps: exactly 0 on pad rows and columns; the null key's column is gone, so real rows sum to 1 - (its mass) < 1
    keep = real[:, None, None, :, None] & real[:, None, None, None, :]
    assert (attn[~keep.expand_as(attn)] == 0).all()
    mass = (1 - attn.sum(-1)).permute(0, 3, 1, 2)[real]
    assert abs(mass.mean().item() - fix["null_mass"]) < 3e-3 and mass.min().item() > 0
    # predict_contacts (fused: no attention tensor) against the materialised path, the existing fused-vs-materialised bound
    with torch.no_grad():
        fused = model.predict_contacts(toks.cuda()).cpu()
    for b, n in enumerate(fix["lengths"]):
        assert (fused[b, :n - 1, :n - 1] - contacts[b, :n - 1, :n - 1]).abs().max().item() < 2e-5


def test_esm1_t34_dims_against_restatement():
    L, E, H = 3, 1280, 20
    model, sd = build(L, E, H, seed=34, final_bias=True)
    toks = synth_tokens(2, 508, seed=12)  # T = 510
    toks[:, 0] = CLS
    toks[:, -1] = 7
    toks[1, 400:] = PAD
    toks[0, 17] = MASK
    with torch.no_grad():
        out = model(toks.cuda(), repr_layers=[0, L])
    ref = esm1_forward(sd, toks, L, H, repr_layers=[0, L])
    real = toks.ne(PAD)
    assert rel_err(out["representations"][0].cpu(), ref["representations"][0], real) < 1e-5  # fp32 embedding + positions
    floor = floor_of(model, sd, toks, L, H, repr_layers=[L])
    C.check_tensors("ESM-1 t34-dims repr", out["representations"][L].cpu(), ref["representations"][L], floor["representations"][L], real)
    C.check_tensors("ESM-1 t34-dims logits", out["logits"].cpu(), ref["logits"], floor["logits"], real)
    assert out["logits"].shape == (2, 510, 35)
    assert isinstance(model, esm.ProteinBertModel) and model.model_version == "ESM-1" and model.num_layers == L


def test_esm1_long_sequence_positions():
    """Positions up to 1 + 1 + 1023: representation 0 (sqrt(E) x embedding + sinusoidal table, fp32) at the released models'
    longest input."""
    model, sd = build(1, 128, 2, seed=5)
    toks = synth_tokens(1, 1022, seed=3)
    toks[:, 0] = CLS
    with torch.no_grad():
        out = model(toks.cuda(), repr_layers=[0])
    ref = esm1_forward(sd, toks, 1, 2, repr_layers=[0])
    assert rel_err(out["representations"][0].cpu(), ref["representations"][0]) < 1e-5


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_esm1_low_precision_models_return_their_dtype(dt):
    fix = load_fixture("tiny_d64")
    d, sd = fixture_model_inputs(fix)
    L, H = d["L"], d["H"]
    model, _ = build(L, d["E"], H, d["seed"])
    model = model.to(dt)
    toks = fix["tokens"]
    with torch.no_grad():
        out = model(toks.cuda(), repr_layers=[0, L], need_head_weights=True)
    assert out["logits"].dtype == dt and out["attentions"].dtype == dt
    assert all(r.dtype == dt for r in out["representations"].values())
    # against the restatement on the model's own (rounded) parameters, with that dtype's operand floor
    sd_lp = {k: v.to(dt).float() for k, v in sd.items()}
    ref = esm1_forward(sd_lp, toks, L, H, repr_layers=[L])
    floor = C.floor_forward(sd_lp, toks, L, H, dtype=dt, forward=esm1_forward, repr_layers=[L])
    real = toks.ne(PAD)
    l2, mx = C.errors(out["representations"][L].float().cpu(), ref["representations"][L], real)
    f_l2, f_mx = C.errors(floor["representations"][L], ref["representations"][L], real)
    eps = 2.0 ** -11 if dt == torch.float16 else 2.0 ** -8  # the output's own rounding on top of the operand floor
    print(f"\nesm1 {dt} repr[{L}]: L2 {l2:.2e} (floor {f_l2:.2e}), max {mx:.2e} (floor {f_mx:.2e})")
    assert l2 <= max(C.CONTRACT, C.SLACK_L2 * f_l2) + eps and mx <= max(C.CONTRACT, C.SLACK_TOY * f_mx) + eps


def test_esm1_forward_varlen_is_forward_on_real_positions():
    fix = load_fixture("mid_d64")
    d, _ = fixture_model_inputs(fix)
    L = d["L"]
    model, _ = build(L, d["E"], d["H"], d["seed"], d["final_bias"], d["token_dropout"])
    toks = fix["tokens"].cuda()
    with torch.no_grad():
        a = model(toks, repr_layers=[0, L])
        b = model.forward_varlen(toks, repr_layers=[0, L], min_saving=None)
        c = model.forward_varlen(toks.cpu(), repr_layers=[L], contacts_only=True)
        ct = model.predict_contacts(toks)
    real = toks.ne(PAD)
    assert torch.equal(a["logits"][real], b["logits"][real])
    for l in (0, L):
        assert torch.equal(a["representations"][l][real], b["representations"][l][real])
    assert torch.equal(c["contacts"], ct) and "logits" not in c


def test_esm1_refusals(monkeypatch):
    """No LayerNorm fold, no split-operand modes, no token-packed batches: each refused with a message naming ESM-1."""
    model, _ = build(1, 128, 2, seed=2)
    toks = synth_tokens(2, 30, seed=1).cuda()
    toks[:, 0] = CLS
    monkeypatch.setenv("ESM_AMD_LN_FOLD", "1")  # the package never asks the library for the fold on this family
    with torch.no_grad():
        model(toks)
    assert model.ln_fold_active() is False
    monkeypatch.delenv("ESM_AMD_LN_FOLD")
    for mode in ("f16x2", "f16x2v", "f16x3"):
        monkeypatch.setenv("ESM_AMD_OPERAND", mode)
        with pytest.raises(RuntimeError, match="ESM-1"), torch.no_grad():
            model(toks)
    monkeypatch.delenv("ESM_AMD_OPERAND")
    from esm_amd import _native as N

    with pytest.raises(N.EsmkError, match="ESM-1"), torch.no_grad():
        model.forward_varlen(toks, unpack=False)
    with torch.no_grad():
        assert torch.isfinite(model(toks)["logits"]).all()  # the model still runs after the refused calls
