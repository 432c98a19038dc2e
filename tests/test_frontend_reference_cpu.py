"""tests/_frontend_ref.py pinned on the CPU: where an oracle of this repository (oracle/esm2_oracle.py, oracle/esm1b_oracle.py,
tests/_esm1_oracle.py, oracle/msa_oracle.py — each pinned to fixtures the reference itself produced) computes the same
quantity, the new reference must give it; the integer bookkeeping is checked against a plain Python loop.  Every input
holds <pad> and <mask> tokens and an interior <pad>."""
import math

import torch

import _frontend_ref as R
from _esm1_oracle import esm1_forward, sinusoidal_positions
from esm_amd.synth import synth_esm1_state_dict, synth_esm1b_state_dict, synth_esm2_state_dict, synth_msa_state_dict
from oracle.esm1b_oracle import esm1b_forward
from oracle.esm2_oracle import esm2_forward, layer_norm, rope_tables
from oracle.msa_oracle import msa_forward

PAD, MASK = 1, 32


def tokens_with_edges(T=21, seed=0, mask=MASK):
    """[6,T]: no pad | trailing pads | an interior pad and masks | a leading pad | token pad token pad pad at the end, a mask
    next to a pad | masks only between <cls> and <eos>."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(4, 24, (6, T), generator=g, dtype=torch.int64)
    t[:, 0] = 0
    t[1, T - 5:] = PAD
    t[2, 7] = PAD
    t[2, 3], t[2, 8] = mask, mask
    t[3, 0] = PAD
    t[4, T - 4], t[4, T - 2:] = PAD, PAD
    t[4, T - 5] = mask
    t[5, 1:T - 1] = mask
    return t


def test_seq_stats_reference_is_the_loop_and_the_oracle_mask():
    t = tokens_with_edges()
    t = torch.cat([t, torch.full((1, t.shape[1]), PAD), torch.full((1, t.shape[1]), MASK)])  # all <pad>, all <mask>
    scale, key_bias, info, keep = R.seq_stats_ref(t, PAD, MASK)
    for b, row in enumerate(t.tolist()):
        n_pad = sum(v == PAD for v in row)
        last = max([i + 1 for i, v in enumerate(row) if v != PAD], default=0)
        assert info[b].tolist() == [n_pad, last], b
        assert keep[b].tolist() == [float(v != PAD) for v in row]
        assert key_bias[b].tolist() == [float("-inf") if v == PAD else 0.0 for v in row]
    assert info[4].tolist() == [3, t.shape[1] - 2]  # token pad token pad pad: the last token counts, the pad before it too
    assert math.isnan(scale[6].item()) and scale[7].item() == 0.0
    # the oracle's divisor (esm2_oracle.py: ratio = n_mask.to(fp32) / src_lengths, 1 - ratio), same bits
    pad = t.eq(PAD)
    ratio = t.eq(MASK).sum(-1).to(torch.float32) / (~pad).sum(-1)
    assert R.same_bits(scale, 1 - ratio)


def test_embed_reference_equals_the_esm2_oracle_layer0():
    L, E, H = 1, 32, 2
    sd = synth_esm2_state_dict(L, E, H, seed=3)
    t = tokens_with_edges()
    scale = R.seq_stats_ref(t, PAD, MASK)[0]
    for dropout in (True, False):
        want = esm2_forward(sd, t, L, H, repr_layers=[0], token_dropout=dropout)["representations"][0]
        got = R.embed_ref(t, sd["embed_tokens.weight"], scale, PAD, MASK, dropout)
        assert torch.equal(got, want), dropout
    assert got[1, -1].abs().max().item() == 0.0 and got[2, 7].abs().max().item() == 0.0  # pad rows
    # out-of-range tokens take a zero row
    bad = torch.tensor([[-1, 33, 5]])
    x = R.embed_ref(bad, sd["embed_tokens.weight"], torch.ones(1), PAD, MASK, False)
    assert x[0, :2].abs().max().item() == 0.0 and torch.equal(x[0, 2], sd["embed_tokens.weight"][5])


def test_learned_positions_reference_equals_the_esm1b_oracle_layer0():
    L, E, H = 1, 32, 2
    t = tokens_with_edges()
    scale, _, _, keep = R.seq_stats_ref(t, PAD, MASK)
    for ln_before in (False, True):
        sd = synth_esm1b_state_dict(L, E, H, seed=4, max_positions=64, ln_before=ln_before)
        want = esm1b_forward(sd, t, L, H, repr_layers=[0])["representations"][0]
        x = R.embed_ref(t, sd["embed_tokens.weight"], scale, PAD, MASK, True)
        # esm1.py:133 adds the positions BEFORE the pad rows are zeroed (:138-139): undo embed_ref's zeroing of pad rows
        x = torch.where(t.eq(PAD).unsqueeze(-1), R.embed_esm1_pad_rows_ref(t, sd["embed_tokens.weight"], scale, 1.0, MASK, True), x)
        x = R.add_positions_ref(x, t, sd["embed_positions.weight"], PAD)
        if ln_before:
            x = layer_norm(x, sd["emb_layer_norm_before.weight"], sd["emb_layer_norm_before.bias"])
        assert torch.equal(x * keep.unsqueeze(-1), want), ln_before
    ids = R.position_ids(t, PAD)
    assert ids[2].tolist()[:10] == [2, 3, 4, 5, 6, 7, 8, 1, 9, 10] and ids[3].tolist()[:3] == [1, 2, 3]
    # the packed form: every segment is a sequence of its own, rows in between are not touched
    rows = torch.cat([t[2], torch.full((11,), 7), t[4][:5]])
    segs = [(0, 21), (32, 5)]
    x0 = torch.randn((rows.numel(), E), generator=torch.Generator().manual_seed(1))
    got = R.add_positions_packed_ref(x0, rows, sd["embed_positions.weight"], segs, PAD)
    assert torch.equal(got[:21], R.add_positions_ref(x0[None, :21], t[2:3], sd["embed_positions.weight"], PAD)[0])
    assert torch.equal(got[21:32], x0[21:32]) and not torch.equal(got[32:], x0[32:])


def test_esm1_reference_matches_the_esm1_oracle_layer0():
    L, E, H, mask = 1, 32, 2, 33
    sd = synth_esm1_state_dict(L, E, H, seed=5)
    t = tokens_with_edges(mask=mask)
    scale = R.seq_stats_ref(t, PAD, mask)[0]
    T = t.shape[1]
    table64 = R.sinus_table_ref(R.sinus_freq(E // 2), T, PAD + 1)
    # the oracle's fp32 table (torch.sin / cos of the same fp32 angles): within 2^-22 of the fp64 values, and the layout
    want_tab = sinusoidal_positions(torch.zeros((1, T), dtype=torch.int64), E, PAD)[0]
    assert (want_tab.double() - table64).abs().max().item() <= R.TABLE_BOUND
    assert torch.equal(table64[:, :E // 2], torch.sin(R.angles32(R.sinus_freq(E // 2), T, PAD + 1).double()))
    sinus = table64.float()
    for dropout in (False, True):
        want = esm1_forward(sd, t, L, H, repr_layers=[0], token_dropout=dropout, mask_idx=mask)["representations"][0]
        ref, bound = R.embed_esm1_ref(t, sd["embed_tokens.weight"], scale, sinus, math.sqrt(E), PAD, mask, dropout)
        # the oracle works in fp32 with sqrt(E) and 0.88 as Python floats folded differently: a few roundings of the same size
        assert ((want.double() - ref).abs() <= 2 * bound + 2.0 ** -23 * sinus.abs().unsqueeze(0)).all(), dropout
        pads = t.eq(PAD)
        fixed = R.embed_esm1_pad_rows_ref(t, sd["embed_tokens.weight"], scale, math.sqrt(E), mask, dropout)
        nan = torch.isnan(ref)  # none here: no row of padding or of masks only
        assert not nan.any()
        # no position term on a pad row: the fp64 value is the scaled embedding alone, the kernel-order fp32 value rounds it
        assert ((ref - fixed.double()).abs()[pads] <= bound[pads]).all() and (bound[pads] > 0).any()


def test_msa_embed_reference_equals_the_msa_oracle_layer0():
    L, E, H = 1, 32, 2
    sd = synth_msa_state_dict(L, E, H, 64, seed=6, max_positions=64)
    g = torch.Generator().manual_seed(7)
    t = torch.randint(4, 24, (2, 3, 19), generator=g, dtype=torch.int64)
    t[:, :, 0] = 0
    t[0, 1, 6], t[0, 1, 15:], t[1, 2, 0], t[1, 0, 9] = PAD, PAD, PAD, MASK
    want = msa_forward(sd, t, L, H, repr_layers=[0])["representations"][0]
    x, keep, col_fill, any_pad = R.msa_embed_ref(t, sd["embed_tokens.weight"], sd["embed_positions.weight"],
                                                 sd["msa_position_embedding"], PAD)
    got = layer_norm(x, sd["emb_layer_norm_before.weight"], sd["emb_layer_norm_before.bias"]) * keep.unsqueeze(-1)
    assert torch.equal(got, want)
    assert any_pad and torch.equal(col_fill, t.eq(PAD).transpose(1, 2).float()) and col_fill.shape == (2, 19, 3)
    clean = t.masked_fill(t.eq(PAD), 5)
    assert R.msa_embed_ref(clean, sd["embed_tokens.weight"], sd["embed_positions.weight"], None, PAD)[3] is False


def test_rope_table_reference_matches_the_oracle_tables():
    for dim in (16, 64, 128):
        inv = R.rope_inv_freq(dim)
        cos64, sin64 = R.rope_table_ref(inv, 1030)
        cos32, sin32 = rope_tables(1030, dim)
        half = dim // 2
        cos32, sin32 = cos32.reshape(1030, -1)[:, :half], sin32.reshape(1030, -1)[:, :half]
        assert (cos32.double() - cos64).abs().max().item() <= R.TABLE_BOUND
        assert (sin32.double() - sin64).abs().max().item() <= R.TABLE_BOUND


def test_packed_stats_and_gather_references():
    t = tokens_with_edges()
    rows = torch.full((64,), 9, dtype=torch.int64)
    rows[0:21], rows[32:53] = t[2], t[4]
    segs = [(0, 21), (32, 21)]
    scale_row, key_bias, row_pos, npad, keep = R.packed_stats_ref(rows, segs, PAD, MASK)
    s2, kb2, info2, kp2 = R.seq_stats_ref(t[[2, 4]], PAD, MASK)
    assert npad.tolist() == info2[:, 0].tolist() == [1, 3]
    assert R.same_bits(scale_row[:21], s2[0].expand(21)) and R.same_bits(scale_row[32:53], s2[1].expand(21))
    assert torch.equal(key_bias[32:53], kb2[1]) and torch.equal(keep[:21], kp2[0]) and row_pos[32:53].tolist() == list(range(21))
    gap = R.gap_rows(segs, 64)
    assert int(gap.sum()) == 22
    assert (scale_row[gap] == 1).all() and (key_bias[gap] == float("-inf")).all() and not row_pos[gap].any() and not keep[gap].any()
    x = torch.arange(37 * 4, dtype=torch.float32).view(37, 4)
    sel = torch.tensor([0, 36, 36, -5, 40, 7], dtype=torch.int32)
    assert R.gather_rows_ref(x, sel)[:, 0].tolist() == [0.0, 144.0, 144.0, 0.0, 144.0, 28.0]
