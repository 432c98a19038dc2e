"""One engine, one workspace, every entry kind in sequence (esm_amd/engine.py): the padded forward, the token-packed forward with
attention and contact maps, the padded and the packed row-selected forwards, and the padded forward again — each after every
byte of the workspace was set to 0xFF (NaN in fp16 / fp32), so nothing may be read before it is written, whichever entry sized
and used the workspace before.  The engine is compared with itself across call orders, bit for bit; parity against the
references is what the other suites check."""
import argparse

import pytest
import torch

import esm
from esm_amd import msa_scoring, scoring
from esm_amd.packing import pack_plan
from esm_amd.synth import synth_esm2_state_dict, synth_msa_state_dict, synth_msa_tokens

pytestmark = pytest.mark.gpu
PAD, CLS, EOS = 1, 0, 2


def poisoned(model, sizes):
    """Note the workspace size, then poison it for the next call."""
    ws = model._engine.workspace
    sizes.append(ws.numel())
    ws.fill_(255)


def test_one_workspace_serves_every_esm2_entry():
    L, E, H = 2, 128, 2
    model = esm.ESM2(L, E, H).eval()
    model.load_state_dict(synth_esm2_state_dict(L, E, H, seed=17))
    model = model.cuda()
    lengths = [70, 33, 17]  # incl. <cls> / <eos>: T = 70 crosses the 64-row tile edge and the 16-row segment alignment
    T = max(lengths)
    g = torch.Generator().manual_seed(5)
    toks = torch.full((len(lengths), T), PAD, dtype=torch.int64)
    for b, n in enumerate(lengths):
        toks[b, :n] = torch.randint(4, 24, (n,), generator=g)
        toks[b, 0], toks[b, n - 1] = CLS, EOS
    nonpad = toks.ne(PAD).cuda()
    plan = pack_plan(toks, PAD)
    cells = [(0, 0), (0, 63), (0, 64), (0, 69), (1, 1), (1, 32), (2, 16)]  # (sequence, position), none on padding
    sel_padded = torch.tensor([b * T + t for b, t in cells], dtype=torch.int32).cuda()
    sel_packed = torch.tensor([int(plan.segments[b, 0]) + t for b, t in cells], dtype=torch.int32).cuda()
    sizes = []
    with torch.no_grad():
        first = model(toks.cuda(), repr_layers=[L])
        poisoned(model, sizes)
        packed = model.forward_varlen(toks, repr_layers=[L], min_saving=None, need_head_weights=True, return_contacts=True)
        poisoned(model, sizes)
        _, rows_padded = scoring.forward_rows(model, toks.cuda(), sel_padded, return_logits=True)
        poisoned(model, sizes)
        flat = plan.pack(toks, PAD, plan.index("cuda")[0]).contiguous()
        _, rows_packed = scoring.forward_rows_packed(model, flat, plan.segments, sel_packed, return_logits=True)
        poisoned(model, sizes)
        last = model(toks.cuda(), repr_layers=[L])
        sizes.append(model._engine.workspace.numel())
    assert torch.equal(last["logits"], first["logits"])
    assert torch.equal(last["representations"][L], first["representations"][L])
    want = first["logits"].view(-1, first["logits"].shape[-1])[sel_padded.long()]
    assert torch.equal(rows_padded, want) and torch.equal(rows_packed, want)
    assert torch.equal(packed["logits"][nonpad], first["logits"][nonpad])
    assert torch.equal(packed["representations"][L][nonpad], first["representations"][L][nonpad])
    assert sizes == sorted(sizes), sizes


def test_one_workspace_serves_every_msa_entry():
    L, E, H, F = 2, 128, 2, 256
    args = argparse.Namespace(layers=L, embed_dim=E, ffn_embed_dim=F, attention_heads=H, dropout=0.1, attention_dropout=0.1,
                              activation_dropout=0.1, max_positions=1024, embed_positions_msa=True, embed_positions_msa_dim=E,
                              max_tokens=2 ** 14, max_tokens_per_msa=2 ** 14)
    model = esm.MSATransformer(args, esm.Alphabet.from_architecture("msa_transformer")).eval()
    model.load_state_dict(synth_msa_state_dict(L, E, H, F, seed=24), strict=True)
    model = model.cuda()
    R, C = 3, 33
    toks = synth_msa_tokens(1, R, C, seed=3).cuda()
    sel = torch.tensor([0, 1, C - 1, C, 2 * C + 16, R * C - 1], dtype=torch.int32).cuda()  # cells (row * C + column)
    sizes = []
    with torch.no_grad():
        first = model(toks, repr_layers=[L])
        poisoned(model, sizes)
        _, rows = msa_scoring.msa_forward_rows(model, toks, sel, return_logits=True)
        poisoned(model, sizes)
        last = model(toks, repr_layers=[L])
        sizes.append(model._engine.workspace.numel())
    assert torch.equal(last["logits"], first["logits"])
    assert torch.equal(last["representations"][L], first["representations"][L])
    assert torch.equal(rows, first["logits"].view(-1, first["logits"].shape[-1])[sel.long()])
    assert sizes == sorted(sizes), sizes
