"""Contact maps of token-packed batches (esmk_forward_packed_ex / ESM2.forward_varlen(contacts_only=True)) on the MI355X.

Each segment's contacts are accumulated in its own [len, len] scratch with the chunk and block boundaries of the sequence
run alone, so a segment's map equals predict_contacts on that sequence wherever the head grouping G is the same (one
segment; B equal, pad-free lengths) and differs only by the fp32 order of the head-group sum otherwise."""
import argparse
import os
import subprocess
import sys

import pytest
import torch

import esm
from esm_amd.synth import synth_esm1b_state_dict, synth_esm2_state_dict
from oracle.esm2_oracle import esm2_forward

import _contract as C

pytestmark = pytest.mark.gpu
PAD, MASK, CLS, EOS = 1, 32, 0, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(L, E, H, seed, dtype=torch.float16):
    sd = synth_esm2_state_dict(L, E, H, seed=seed)
    m = esm.ESM2(L, E, H).eval()
    m.load_state_dict(sd)
    m = m.cuda()
    if dtype == torch.bfloat16:
        m = m.to(torch.bfloat16)
    return m, sd


def ragged_batch(lengths, seed, masks=(), interior_pad=()):
    g = torch.Generator().manual_seed(seed)
    toks = torch.full((len(lengths), max(lengths)), PAD, dtype=torch.int64)
    for b, n in enumerate(lengths):
        toks[b, 0] = CLS
        if n > 2:
            toks[b, 1:n - 1] = torch.randint(4, 24, (n - 2,), generator=g)
        toks[b, n - 1] = EOS
    for b, t in masks:
        toks[b, t] = MASK
    for b, t in interior_pad:
        toks[b, t] = PAD
    return toks


def off_block(m, S):
    """the entries of an unpacked [T-2, T-2] map outside its sequence's top-left [S, S] block"""
    keep = torch.ones_like(m, dtype=torch.bool)
    keep[:S, :S] = False
    return m[keep] if bool(keep.any()) else m.new_zeros(1)


def alone(model, toks, b, n):
    return model.predict_contacts(toks[b:b + 1, :n].cuda())[0]


ONE_LENGTHS = [3, 4, 63, 64, 65, 66, 127, 128, 129, 130, 255, 256, 257, 258, 1022]


@pytest.mark.parametrize("dims,dtype", [((2, 128, 2), torch.float16), ((2, 256, 2), torch.float16),
                                        ((2, 128, 2), torch.bfloat16), ((2, 256, 2), torch.bfloat16)],
                         ids=["d64_f16", "d128_f16", "d64_bf16", "d128_bf16"])
def test_one_segment_equals_alone(dims, dtype):
    L, E, H = dims
    model, _ = build(L, E, H, seed=21, dtype=dtype)
    with torch.no_grad():
        for n in ONE_LENGTHS:
            toks = ragged_batch([n], seed=n)
            got = model.forward_varlen(toks, repr_layers=[L], min_saving=None, contacts_only=True)["contacts"][0]
            ref = alone(model, toks, 0, n)
            assert got.shape == ref.shape == (n - 2, n - 2)
            assert torch.equal(got, ref), (n, (got.float() - ref.float()).abs().max().item())


@pytest.mark.parametrize("dims", [(2, 128, 2), (2, 256, 2)], ids=["d64", "d128"])
@pytest.mark.parametrize("n", [64, 130, 300])
def test_equal_lengths_equal_padded(dims, n):
    L, E, H = dims
    model, _ = build(L, E, H, seed=4)
    toks = ragged_batch([n] * 4, seed=n + 1)
    with torch.no_grad():
        got = model.forward_varlen(toks, repr_layers=[L], min_saving=None, contacts_only=True)["contacts"]
        ref = model.predict_contacts(toks.cuda())
    assert torch.equal(got, ref)


MIXED = [2, 3, 50, 127, 128, 129, 200, 17, 256, 257, 33, 300]


@pytest.mark.parametrize("dims", [(3, 128, 4), (2, 256, 2)], ids=["d64", "d128"])
def test_mixed_lengths(dims):
    L, E, H = dims
    model, sd = build(L, E, H, seed=5)
    toks = ragged_batch(MIXED, seed=7, masks=[(4, 5), (6, 100)], interior_pad=[(6, 20), (11, 150)])
    with torch.no_grad():
        a = model.forward_varlen(toks, repr_layers=[L], min_saving=None, contacts_only=True)
        model._engine.workspace.fill_(255)  # nothing may be read before it is written
        b = model.forward_varlen(toks, repr_layers=[L], min_saving=None, contacts_only=True)
        plain = model.forward_varlen(toks, repr_layers=[L], min_saving=None)
    assert torch.equal(a["contacts"], b["contacts"])
    assert torch.equal(a["representations"][L], plain["representations"][L])
    ref = esm2_forward(sd, toks, L, H, repr_layers=[L], return_contacts=True)["contacts"]
    floor = C.floor_forward(sd, toks, L, H, model=model, repr_layers=[L], return_contacts=True)["contacts"]
    got_all, ref_all, floor_all = [], [], []
    for i, n in enumerate(MIXED):
        S = max(n - 2, 0)
        got = a["contacts"][i, :S, :S]
        assert off_block(a["contacts"][i], S).abs().max().item() == 0  # zero outside the sequence's block
        if S == 0:
            continue
        with torch.no_grad():
            one = alone(model, toks, i, n)
        assert (got - one).abs().max().item() <= 1e-6, (n, (got - one).abs().max().item())
        got_all.append(got.flatten().cpu())
        ref_all.append(ref[i, :S, :S].flatten())
        floor_all.append(floor[i, :S, :S].flatten())
    # the parity contract (tests/_contract.py) on the contact logits of all segments, against the floor on the same inputs
    _, rel = C.contact_logit_errors(torch.cat(got_all), torch.cat(ref_all))
    _, rel_f = C.contact_logit_errors(torch.cat(floor_all), torch.cat(ref_all))
    print(f"\ncontract packed contacts: rel max {rel:.2e} (floor {rel_f:.2e})")
    assert rel <= max(C.CONTRACT, C.SLACK_TOY * rel_f), (rel, rel_f)


def test_python_shapes_and_logits():
    L, E, H = 2, 128, 2
    model, _ = build(L, E, H, seed=8)
    lengths = [40, 2, 131, 77]
    toks = ragged_batch(lengths, seed=3)
    with torch.no_grad():
        pad = model(toks.cuda(), repr_layers=[L], contacts_only=True)
        un = model.forward_varlen(toks, repr_layers=[L], min_saving=None, contacts_only=True)
        raw = model.forward_varlen(toks, repr_layers=[L], min_saving=None, contacts_only=True, unpack=False)
        both = model.forward_varlen(toks, repr_layers=[L], min_saving=None, return_contacts=True)
        plain = model.forward_varlen(toks, repr_layers=[L], min_saving=None)
        fb = model.forward_varlen(toks, repr_layers=[L], contacts_only=True, min_saving=0.99)  # padded fallback
    assert un["contacts"].shape == pad["contacts"].shape and un["contacts"].dtype == pad["contacts"].dtype
    assert "logits" not in un
    # (the padded map of the 2-token sequence is 0/0 like the reference's apc: NaN == NaN here)
    assert torch.allclose(fb["contacts"], pad["contacts"], rtol=0, atol=0, equal_nan=True)
    assert len(raw["contacts"]) == len(lengths)
    for b, n in enumerate(lengths):
        S = max(n - 2, 0)
        assert raw["contacts"][b].shape == (S, S)
        assert torch.equal(raw["contacts"][b], un["contacts"][b, :S, :S])
        assert off_block(un["contacts"][b], S).abs().max().item() == 0
    assert torch.equal(both["logits"], plain["logits"])
    assert torch.equal(both["contacts"], un["contacts"])


def test_all_segments_empty():
    model, _ = build(2, 128, 2, seed=9)
    toks = ragged_batch([2, 2, 2], seed=1)
    with torch.no_grad():
        out = model.forward_varlen(toks, repr_layers=[2], min_saving=None, contacts_only=True)
    assert out["contacts"].shape == (3, 0, 0)


def test_esm1b_segments_equal_alone():
    L, E, H = 2, 128, 2
    args = argparse.Namespace(arch="roberta_large", layers=L, embed_dim=E, ffn_embed_dim=4 * E, attention_heads=H,
                              max_positions=1024, token_dropout=True, emb_layer_norm_before=True)
    model = esm.ProteinBertModel(args, esm.Alphabet.from_architecture("roberta_large")).eval()
    model.load_state_dict(synth_esm1b_state_dict(L, E, H, seed=8, ln_before=True), strict=True)
    model = model.cuda()
    assert model.supports_varlen_contacts
    lengths = [130, 50, 21]
    toks = ragged_batch(lengths, seed=6)
    with torch.no_grad():
        out = model.forward_varlen(toks, repr_layers=[L], min_saving=None, contacts_only=True)
        for b, n in enumerate(lengths):
            one = alone(model, toks, b, n)
            assert (out["contacts"][b, :n - 2, :n - 2] - one).abs().max().item() <= 1e-6, n
        one = model.forward_varlen(toks[:1], repr_layers=[L], min_saving=None, contacts_only=True)["contacts"][0]
        assert torch.equal(one, alone(model, toks, 0, lengths[0]))


@pytest.mark.parametrize("no_varlen", [False, True], ids=["packed", "padded"])
def test_extract_contacts(tmp_path, no_varlen):
    from esm_amd import Alphabet
    from esm_amd.synth import write_esm2_checkpoint

    L, E, H = 3, 128, 2
    ckpt = write_esm2_checkpoint(str(tmp_path), "esm2_synth_vct", L, E, H, seed=6)
    g = torch.Generator().manual_seed(4)
    aas = "LAGVSERTIDPKQNFYMHWC"
    seqs = {f"p{i}": "".join(aas[j] for j in torch.randint(0, 20, (n,), generator=g).tolist())
            for i, n in enumerate([40, 131, 77, 5, 300, 12])}
    fasta = tmp_path / "in.fasta"
    fasta.write_text("".join(f">{k}\n{v}\n" for k, v in seqs.items()))
    out_dir = tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=ROOT, TORCH_FORCE_NO_WEIGHTS_ONLY_LOAD="1")
    cmd = [sys.executable, "-m", "esm_amd.extract", ckpt, str(fasta), str(out_dir), "--repr_layers", "-1",
           "--include", "mean", "contacts", "--toks_per_batch", "1200"] + (["--no_varlen"] if no_varlen else [])
    subprocess.run(cmd, check=True, env=env, cwd=ROOT, timeout=600)
    sd = synth_esm2_state_dict(L, E, H, seed=6)
    alphabet = Alphabet.from_architecture("ESM-1b")
    for label, s in seqs.items():
        toks = torch.tensor([[alphabet.cls_idx] + alphabet.encode(s) + [alphabet.eos_idx]])
        ref = esm2_forward(sd, toks, L, H, repr_layers=[L], return_contacts=True)
        r = torch.load(out_dir / f"{label}.pt", weights_only=False)
        assert r["contacts"].shape == (len(s), len(s))
        assert (r["contacts"] - ref["contacts"][0]).abs().max().item() < 5e-3
        full = ref["representations"][L][0]
        floor = C.floor_forward(sd, toks, L, H, fold=C.default_fold(E, H), repr_layers=[L])["representations"][L][0]
        bound = max(C.CONTRACT, C.SLACK * C.errors(floor, full)[1]) * full.abs().max().item()
        assert (r["mean_representations"][L] - full[1:len(s) + 1].mean(0)).abs().max().item() <= bound
