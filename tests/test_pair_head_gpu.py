"""``model.pair_logits`` on the MI355X: a linear pairwise head (lm-design's distogram / orientation projection) on the attention
maps without the [B,L,H,T,T] tensor (esm_amd/pair_head.py, csrc/pair_head.hip, esmk_forward_rows_pair), against the fp64
restatement of the head (tests/_pair_head_ref.py) applied to ``model(tokens, need_head_weights=True)["attentions"]`` of the
same model.

Bound: ``PairRef.tol`` with eps_p widened by the gap between the materialised and the recomputed probabilities.  Both come
from the same q, k and lse through exp2(s - lse); tests/test_contacts_fused_gpu.py bounds what that gap does to a contact
probability by 2e-5, and that figure is taken here as the widening of eps_p.  The score bound that eps_p needs is read off the
maps: max |log2 P| over the nonzero probabilities >= max |s - lse| (the kernel's exponent)."""
import math

import pytest
import torch

import esm
from esm_amd import PairHead
from esm_amd.interventions import StreamEdit
from esm_amd.synth import synth_esm2_state_dict, synth_tokens
from _pair_head_ref import PairRef, pair_head_on_maps

pytestmark = pytest.mark.gpu
GAP = 2e-5  # tests/test_contacts_fused_gpu.py: materialised against recomputed probabilities


def build(L, E, H, seed):
    m = esm.ESM2(L, E, H).eval()
    m.load_state_dict(synth_esm2_state_dict(L, E, H, seed=seed))
    return m.cuda()


def ragged_tokens(B, Lmax, seed, lengths):
    toks = synth_tokens(B, Lmax, seed=seed)
    for b, n in enumerate(lengths):  # n residues: <cls> r*n <eos> <pad>*
        toks[b, n + 1] = 2
        toks[b, n + 2:] = 1
    return toks


def lm_design_head(L, H, seed, scale=1.0):
    """A head of lm-design's shape (36 symmetric + 26 plain outputs) on L*H channels, drawn from a seeded generator."""
    g = torch.Generator().manual_seed(seed)
    C = L * H
    state = {"conv1.weight": torch.randn(36, C, 1, 1, generator=g) * scale, "conv1.bias": torch.randn(36, generator=g),
             "conv2.weight": torch.randn(26, C, 1, 1, generator=g) * scale, "conv2.bias": torch.randn(26, generator=g)}
    return PairHead.from_linear_projection({"model": state})


def ref_on_maps(model, toks, head):
    with torch.no_grad():
        attn = model(toks, need_head_weights=True)["attentions"]
    z, mag = pair_head_on_maps(attn, head.matrix(), head.bias(), head.n_sym)
    nz = attn[attn > 0].double()
    sbound = float(nz.log2().abs().max()) if nz.numel() else 1.0
    B, L, H, T, _ = attn.shape
    return PairRef(z, mag, None, sbound, L * H, T, 128 if model.embed_dim // H == 128 else 64)


def check(got, ref, where):
    d = (got.double() - ref.z).abs()
    ratio = (d / ref.tol(extra_eps_p=GAP)).max().item()
    print(f"{where}: max |got - ref| / tol = {ratio:.3f}, max |got - ref| = {d.max().item():.3e}")
    assert torch.isfinite(got).all() and ratio <= 1.0, (where, ratio, d.max().item())


@pytest.mark.parametrize("L,E,H,Lmax,lengths", [
    (3, 128, 2, 45, [45, 30, 7]),      # head_dim 64
    (2, 320, 20, 66, [66, 65, 1]),     # head_dim 16 (8M geometry): heads spread over 64 slots
    (2, 256, 2, 70, [70, 33]),         # head_dim 128 (15B geometry)
])
def test_pair_logits_against_materialised(L, E, H, Lmax, lengths):
    model = build(L, E, H, seed=11)
    toks = ragged_tokens(len(lengths), Lmax, seed=5, lengths=lengths).cuda()
    head = lm_design_head(L, H, seed=3)
    out = model.pair_logits(toks, head)
    S = Lmax
    assert set(out) == {"dist", "omega", "theta", "phi", "all"}
    assert out["dist"].shape == (len(lengths), S, S, 18) and out["phi"].shape == (len(lengths), S, S, 8)
    assert out["omega"].data_ptr() == out["all"][..., 18:36].data_ptr()  # views of one tensor
    check(out["all"], ref_on_maps(model, toks, head), f"L={L} E={E} H={H}")
    # entries that involve a <pad> position hold the bias
    padm = toks[:, 1:-1].eq(1)
    anyp = padm[:, :, None] | padm[:, None, :]
    assert torch.equal(out["all"][anyp], head.bias().cuda().expand(int(anyp.sum()), 62))
    assert torch.equal(out["dist"], out["dist"].transpose(1, 2))


def test_row_alone_equals_row_in_batch_and_chunking():
    """A sequence's map does not depend on the batch it ran in, nor on how ``max_bytes`` cuts the batch."""
    L, E, H, T = 2, 128, 2, 300
    model = build(L, E, H, seed=7)
    toks = ragged_tokens(24, T - 2, seed=2, lengths=[T - 2] * 20 + [257, 128, 31, 5]).cuda()
    head = PairHead(torch.randn(5, L * H, generator=torch.Generator().manual_seed(1)), None,
                    torch.randn(3, L * H, generator=torch.Generator().manual_seed(2)), None)
    full = model.pair_logits(toks, head)
    assert set(full) == {"sym", "asym", "all"}
    for b in (0, 21, 23):
        one = model.pair_logits(toks[b:b + 1], head)["all"]
        assert torch.equal(one[0], full["all"][b]), b
    eng = model._engine
    S = T - 2
    small = eng.rows_pair_bytes(5, T, 0) + 5 * S * S * 8 * 4
    cut = model.pair_logits(toks, head, max_bytes=small)["all"]
    assert torch.equal(cut, full["all"])
    with pytest.raises(ValueError, match="max_bytes"):
        model.pair_logits(toks, head, max_bytes=1 << 16)


def test_logit_rows_are_those_of_forward_rows():
    L, E, H, T, B = 2, 128, 2, 40, 3
    model = build(L, E, H, seed=5)
    toks = ragged_tokens(B, T - 2, seed=4, lengths=[38, 20, 9]).cuda()
    head = lm_design_head(L, H, seed=8)
    model.pair_logits(toks, head)  # engine ready, head set
    eng = model._engine
    sel = torch.tensor([1, 5, T + 3, 2 * T + 7, 2 * T + 8], dtype=torch.int32, device="cuda")
    V = model.alphabet_size
    want = eng.forward_rows(toks, sel, V)
    out = torch.empty((B, T - 2, T - 2, 62), dtype=torch.float32, device="cuda")
    got = eng.forward_rows_pair(toks, sel, V, out)
    assert torch.equal(got, want)
    assert torch.equal(out, model.pair_logits(toks, head)["all"])  # with or without selected rows


def test_stream_edit_changes_pair_logits():
    L, E, H = 3, 128, 2
    model = build(L, E, H, seed=9)
    toks = ragged_tokens(2, 30, seed=3, lengths=[30, 12]).cuda()
    head = lm_design_head(L, H, seed=4)
    base = model.pair_logits(toks, head)["all"].clone()
    vec = torch.randn(E, generator=torch.Generator().manual_seed(17))
    edits = [StreamEdit(1, "add", vec, gain=4.0, positions="residues")]
    with model.stream_edits(edits):
        edited = model.pair_logits(toks, head)["all"].clone()
        with torch.no_grad():
            attn = model(toks, need_head_weights=True)["attentions"]
    assert not torch.equal(edited, base)
    z, mag = pair_head_on_maps(attn, head.matrix(), head.bias(), head.n_sym)
    nz = attn[attn > 0].double()
    ref = PairRef(z, mag, None, float(nz.log2().abs().max()), L * H, toks.shape[1], 64)
    check(edited, ref, "edited")
    assert ((base.double() - z).abs() / ref.tol(extra_eps_p=GAP)).max().item() > 10  # the edit moved the maps
    assert torch.equal(model.pair_logits(toks, head)["all"], base)  # and is gone with the context


def test_refusals():
    from esm_amd import _native as N

    L, E, H = 2, 128, 2
    model = build(L, E, H, seed=1)
    toks = synth_tokens(1, 10, seed=1).cuda()
    head = lm_design_head(L, H, seed=1)
    with pytest.raises(NotImplementedError, match="varlen"):
        model.pair_logits(toks, head, varlen=True)
    with pytest.raises(NotImplementedError, match="window"):
        model.pair_logits(toks, head, window=8)
    with pytest.raises(ValueError, match="input channels"):
        model.pair_logits(toks, lm_design_head(L + 1, H, seed=1))
    eng = model._engine_ready(toks.device)
    eng.set_pair_head(None)
    with pytest.raises(N.EsmkError, match="no pairwise head is set"):
        eng.rows_pair_bytes(1, 12, 0)
    w = torch.zeros(L * H, 65)
    with pytest.raises(N.EsmkError, match="0 \\(clear\\) .. 64"):
        N.check(N.lib.esmk_set_pair_head(eng.handle, N.ptr(w), N.ptr(w), 40, 25))
    with pytest.raises(N.EsmkError, match="null weight or bias"):
        N.check(N.lib.esmk_set_pair_head(eng.handle, None, None, 1, 0))
