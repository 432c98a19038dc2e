"""The streaming fp64 contact reference of tests/_contacts_ref.py, checked on every run without a GPU.

1. It equals the oracle's contact head (oracle.esm2_oracle.contact_head, the reference's symmetrize / apc / regression
   on the full [B, L, H, T, T] maps, pads zeroed as esm2.py:135-139 does) in fp64, to rounding, at small shapes in all
   four token layouts, with pads, an interior <eos>, <mask> tokens and a row with no residues (0/0: NaN in both).
2. The error bound the GPU tests use (ContactRef.tol) discriminates: each mutation below, applied to the reference,
   moves some logit by at least 10x the bound — dropping one head of a group, skipping the final kernel's last
   32-channel slab of the apc term, reading a packed segment one row off, taking the wrong layer's weights."""
import math

import pytest
import torch

from _contacts_ref import contact_ref, discrimination, residue_mask
from oracle.esm2_oracle import contact_head

PAD, EOS, CLS, MASK = 1, 2, 0, 32


def _operands(L, B, H, T, D, scale, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(L, B, H, T, D, generator=g, dtype=torch.float64) * scale / math.sqrt(D)  # scores ~ N(0, scale^2)
    k = torch.randn(L, B, H, T, D, generator=g, dtype=torch.float64)
    w = torch.randn(L * H, generator=g, dtype=torch.float64) / math.sqrt(L * H)
    b = torch.randn(1, generator=g, dtype=torch.float64) * 0.3
    return q, k, w, b


def _tokens(B, T, bos, eos, seed):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(4, 24, (B, T), generator=g)
    if bos:
        tok[:, 0] = CLS
    if eos:
        tok[:, -1] = EOS
    return tok


def _oracle(q, k, tokens, w, b, key_bias, bos, eos):
    L, B, H, T, D = q.shape
    s = q @ k.transpose(-1, -2) + key_bias[None, :, None, None, :]
    p = torch.softmax(s, dim=-1).permute(1, 0, 2, 3, 4)  # [B, L, H, T, T]
    keep = tokens.ne(PAD).double()
    p = p * (keep[:, :, None] * keep[:, None, :])[:, None, None]  # esm2.py:135-139
    sd = {"contact_head.regression.weight": w.reshape(1, -1), "contact_head.regression.bias": b.reshape(1)}
    return contact_head(sd, tokens, p, eos_idx=EOS, prepend_bos=bool(bos), append_eos=bool(eos))


@pytest.mark.parametrize("bos,eos", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_streaming_reference_equals_oracle(bos, eos):
    L, B, H, T, D = 3, 3, 4, 23, 16
    q, k, w, b = _operands(L, B, H, T, D, 2.0, seed=11 + 2 * bos + eos)
    tok = _tokens(B, T, bos, eos, seed=5)
    tok[0, T - 6:T - eos] = PAD                  # trailing pads
    tok[1, 7:9] = PAD                            # interior pads
    tok[1, 12] = MASK
    tok[1, 15] = EOS                             # <eos> inside a row
    kb = torch.where(tok.eq(PAD), float("-inf"), 0.0).double()
    ref = contact_ref(q, k, tok, w, b, key_bias=kb, pad_idx=PAD, eos_idx=EOS, bos=bos, eos=eos)
    want = _oracle(q, k, tok, w, b, kb, bos, eos)
    got = ref.prob
    assert got.shape == want.shape
    assert torch.isfinite(want).all()
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-13), (got - want).abs().max().item()
    # the lse handed to the kernel is the softmax's own normaliser over the non-pad keys
    s = q @ k.transpose(-1, -2) + kb[None, :, None, None, :]
    assert torch.allclose(ref.lse, torch.logsumexp(s, -1), rtol=0, atol=1e-12)


def test_streaming_reference_no_residue_row_is_nan_like_oracle():
    L, B, H, T, D = 2, 2, 3, 12, 16
    q, k, w, b = _operands(L, B, H, T, D, 1.0, seed=3)
    tok = _tokens(B, T, 1, 1, seed=8)
    tok[1, 1:-1] = PAD  # <cls> <pad>... <eos>: no residue at all
    kb = torch.where(tok.eq(PAD), float("-inf"), 0.0).double()
    ref = contact_ref(q, k, tok, w, b, key_bias=kb, pad_idx=PAD, eos_idx=EOS)
    want = _oracle(q, k, tok, w, b, kb, 1, 1)
    assert torch.isnan(want[1]).all() and torch.isnan(ref.z[1]).all()
    assert torch.allclose(ref.prob[0], want[0], rtol=1e-12, atol=1e-13)


def test_error_bound_discriminates():
    """Each mutation moves the output by >= 10x ContactRef.tol somewhere (the bound the GPU tests assert), at a
    shape with a partial last 32-channel slab (C = 33) and raw scores of the GPU tests' size."""
    L, H, T, D = 3, 11, 40, 64
    for scale in (1.0, 20.0):  # raw scores ~ N(0, scale^2): up to +-100 at 20
        q, k, w, b = _operands(L, 1, H, T, D, scale, seed=21)
        tok = _tokens(1, T, 1, 1, seed=2)
        ref = contact_ref(q, k, tok, w, b)
        assert ref.tol().max().item() < 1e-3
        muts = {
            "drop one head": contact_ref(q, k, tok, w, b, drop={(1, 5)}),
            "skip last 32-channel slab": contact_ref(q, k, tok, w, b, apc_upto=32),
            "wrong layer's weights": contact_ref(q, k, tok, w, b, w_layer_shift=1),
        }
        # a packed segment read one row off: the same rows of a longer buffer, shifted by one
        qq, kk, _, _ = _operands(L, 1, H, T + 1, D, scale, seed=22)
        tt = _tokens(1, T + 1, 0, 0, seed=4)
        tt[0, 0] = CLS
        tt[0, T - 1] = EOS
        seg = contact_ref(qq[:, :, :, :T], kk[:, :, :, :T], tt[:, :T], w, b)
        off = contact_ref(qq[:, :, :, 1:], kk[:, :, :, 1:], tt[:, :T], w, b)
        for name, m in muts.items():
            assert discrimination(ref, m) >= 10, (scale, name, discrimination(ref, m))
        assert discrimination(seg, off) >= 10, (scale, discrimination(seg, off))


def test_residue_mask_layouts():
    tok = torch.tensor([[CLS, 5, PAD, EOS, 6, EOS]])
    assert residue_mask(tok, PAD, EOS, 1, 1).tolist() == [[False, True, False, False, True, False]]
    assert residue_mask(tok, PAD, EOS, 1, 0).tolist() == [[False, True, False, True, True, True]]
    assert residue_mask(tok, PAD, EOS, 0, 0).tolist() == [[True, True, False, True, True, True]]
