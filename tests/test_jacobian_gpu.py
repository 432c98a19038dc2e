"""The categorical Jacobian through the model (esm_amd/jacobian.py): the raw tensor bit for bit against the definition run on
this model's own ``forward`` at B = 1 (tests/_jacobian_ref.loop_jacobian), whatever the chunking, the candidate list and the
padding; the contact map against the fp64 pipeline on the engine's own raw tensor inside the derived bound.  Synthetic models
of esm_amd/synth.py, L = 2 layers, E = 128, H = 2 (one with head_dim 128: E = 256, H = 2)."""
import argparse
import functools

import pytest
import torch

import _jacobian_ref as R
import esm
from esm_amd import jacobian, ops
from esm_amd.sampling import STANDARD_RESIDUES
from esm_amd.synth import synth_esm1b_state_dict, synth_esm2_state_dict, synth_tokens

pytestmark = pytest.mark.gpu
LAYERS = 2


def esm2_model(E=128, H=2, seed=3):
    model = esm.ESM2(LAYERS, E, H).eval()
    model.load_state_dict(synth_esm2_state_dict(LAYERS, E, H, seed=seed))
    return model.cuda()


def esm1b_model():
    args = argparse.Namespace(arch="roberta_large", layers=LAYERS, embed_dim=128, ffn_embed_dim=512, attention_heads=2,
                              max_positions=1024, token_dropout=True, emb_layer_norm_before=True)
    model = esm.ProteinBertModel(args, esm.Alphabet.from_architecture("roberta_large")).eval()
    model.load_state_dict(synth_esm1b_state_dict(LAYERS, 128, 2, seed=5), strict=True)
    return model.cuda()


CASES = {"esm2": (esm2_model, 23), "esm1b": (esm1b_model, 11), "head_dim128": (lambda: esm2_model(E=256, H=2), 11)}


@functools.lru_cache(maxsize=None)
def loop_case(kind):
    """(model, tokens [1, T], the loop's raw tensor): computed once per model kind and left unchanged."""
    make, n_res = CASES[kind]
    model = make()
    toks = synth_tokens(1, n_res, seed=n_res).cuda()
    cols = [model.alphabet.get_idx(a) for a in STANDARD_RESIDUES]
    return model, toks, R.loop_jacobian(model, toks, cols)


@pytest.mark.parametrize("kind", list(CASES))
def test_raw_tensor_equals_the_loop(kind):
    model, toks, loop = loop_case(kind)
    L = CASES[kind][1]
    assert toks.shape[1] == L + 2 and bool(loop.ne(0).any())
    small = model.categorical_jacobian(toks, chunk=7)  # 7 is no multiple of 20: a position's copies straddle chunks
    assert small.dtype == torch.float32 and tuple(small.shape) == (L, 20, L, 20) and small.is_cuda
    print(f"\ncategorical_jacobian {kind}: max |engine - loop| = {(small - loop).abs().max().item():.3e}")
    assert torch.equal(small, loop), f"{kind}: chunk=7 differs from the B = 1 loop"
    default = jacobian.categorical_jacobian(model, toks[0])  # [T]; all copies in one chunk
    assert torch.equal(default, loop), f"{kind}: the default chunk differs from the B = 1 loop"
    assert torch.equal(default, small)


def test_raw_tensor_bf16_operands(monkeypatch):
    monkeypatch.setenv("ESM_AMD_OPERAND", "bf16")
    model = esm2_model()
    toks = synth_tokens(1, 11, seed=11).cuda()
    loop = R.loop_jacobian(model, toks, [model.alphabet.get_idx(a) for a in STANDARD_RESIDUES])
    got = model.categorical_jacobian(toks, chunk=7)
    print(f"\ncategorical_jacobian bf16: max |engine - loop| = {(got - loop).abs().max().item():.3e}")
    assert torch.equal(got, loop) and torch.equal(model.categorical_jacobian(toks), loop)


def test_restricted_candidates_and_trailing_padding():
    model, toks, loop = loop_case("esm2")
    idx = torch.tensor([STANDARD_RESIDUES.index(a) for a in "AGV"]).cuda()
    agv = model.categorical_jacobian(toks, allowed="AGV", chunk=7)
    assert tuple(agv.shape) == (23, 3, 23, 3)
    assert torch.equal(agv, loop[:, idx][:, :, :, idx])  # the same copies, the same columns
    by_index = model.categorical_jacobian(toks, allowed=[model.alphabet.get_idx(a) for a in "AGV"])
    assert torch.equal(by_index, agv)
    padded = torch.full((1, toks.shape[1] + 9), model.padding_idx, dtype=torch.int64).cuda()
    padded[0, :toks.shape[1]] = toks[0]
    assert torch.equal(model.categorical_jacobian(padded, chunk=7), loop)
    assert torch.equal(model.categorical_jacobian(padded), loop)


@pytest.mark.parametrize("kind", ["esm2", "esm1b"])
def test_contact_map_against_fp64(kind):
    model, toks, loop = loop_case(kind)
    L = CASES[kind][1]
    raw = model.categorical_jacobian(toks)
    C, Jc = model.jacobian_contacts(toks, chunk=7, return_jacobian=True)
    assert C.dtype == torch.float32 and tuple(C.shape) == (L, L) and torch.isfinite(C).all()
    assert torch.equal(Jc, ops.jacobian_center(raw.clone()))
    assert torch.equal(model.categorical_jacobian(toks, center=True), Jc)
    ref, bound = R.contact_map_ref_and_bound(raw)
    R.report(f"jacobian_contacts {kind}", (C.double() - ref).abs().cpu(), bound.cpu())
    assert bool((C.diagonal() == 0).all()) and bool(C.abs().max() > 0)
    assert torch.equal(jacobian.jacobian_contacts(model, toks), C)  # another chunking, no tensor returned: the same map


def test_refusals():
    model = esm2_model()
    toks = synth_tokens(1, 11, seed=1).cuda()
    with pytest.raises(ValueError, match="ONE sequence"):
        model.categorical_jacobian(synth_tokens(2, 11, seed=1).cuda())
    with pytest.raises(ValueError, match="max_bytes"):
        model.categorical_jacobian(toks, max_bytes=11 * 11 * 400 * 4 - 1)
    assert model.categorical_jacobian(toks, max_bytes=11 * 11 * 400 * 4).numel() == 11 * 11 * 400
    for bad in ("", [], "A?", [99], "AA", range(33)):
        with pytest.raises(ValueError):
            model.categorical_jacobian(toks, allowed=bad)
    with pytest.raises(ValueError, match="no residues"):
        model.jacobian_contacts(torch.tensor([[0, 2]]).cuda())
    with pytest.raises(ValueError, match="chunk"):
        model.categorical_jacobian(toks, chunk=0)
    margs = argparse.Namespace(layers=1, embed_dim=64, ffn_embed_dim=128, attention_heads=2, dropout=0.1, attention_dropout=0.1,
                               activation_dropout=0.1, max_positions=1024, embed_positions_msa=True, embed_positions_msa_dim=64,
                               max_tokens=2 ** 14, max_tokens_per_msa=2 ** 14)
    msa = esm.MSATransformer(margs, esm.Alphabet.from_architecture("msa_transformer")).cuda()
    msa_toks = torch.zeros((1, 2, 8), dtype=torch.int64).cuda()
    for call in (lambda: msa.categorical_jacobian(msa_toks), lambda: msa.jacobian_contacts(msa_toks),
                 lambda: jacobian.categorical_jacobian(msa, msa_toks), lambda: jacobian.jacobian_contacts(msa, msa_toks)):
        with pytest.raises(NotImplementedError, match="MSA Transformer"):
            call()
