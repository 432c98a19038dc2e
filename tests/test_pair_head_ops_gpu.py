"""The pairwise-head kernels (csrc/pair_head.hip) one op at a time against fp64 restatements (tests/_pair_head_ref.py).

esmk_op_pair_head runs the engine's own launchers (one accumulate launch over all L*H channels, one in-place launch for the
transpose term and the bias) on q, k and lse the test supplies; EVERY element of the output is compared with the fp64
restatement on the kernel's own operand values (q_effective of ops.to_log2_domain, k rounded to the operand dtype, the same
pad marks, lse = fp32(fp64 logsumexp * log2 e)) under ``PairRef.tol``: |got - ref| <= 2 kappa mag + 4u (|ref| + 1),
kappa = eps_p + (L*H + 8) u.  Lengths sit on the kernel's tile edges (16-wide sub-tiles, 32-wide workgroup tiles, more than one
workgroup); head widths cover the 64-slot form with a narrow head (16 of 64 slots used), the full 64 and the 128-slot form; the
output counts cover both store paths (C_out % 4 == 0 or not), one and two output halves (<= 32, > 32) and the limits 1 and 64.

esmk_op_distogram_energy against get_cce_loss' formula in fp64 to 1e-12 relative, and bit for bit across batch sizes."""
import math

import pytest
import torch

from _pair_head_ref import check_against_ref, distogram_energy_ref, pair_head_ref

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
PAD, EOS, CLS = 1, 2, 0


@pytest.fixture(scope="module")
def ops():
    from esm_amd import ops as _ops

    return _ops


def _operands(ops, L, B, H, T, D, d_used, dt, scale, C_out, seed):
    """q (log2-domain operand and its natural-domain value), k with d_used of the D slots in use (narrow heads are spread over
    64 slots, the rest zero: esmk_create), raw scores ~ N(0, (4.8 scale)^2); w ~ N(0, 1), bias ~ N(0, 1)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    kscale = 0.6 * math.sqrt(64.0 / d_used)
    q = torch.randn(L, B, H, T, D, device="cuda", generator=g) * scale
    k = torch.randn(L, B, H, T, D, device="cuda", generator=g) * kscale
    q[..., d_used:] = 0
    k[..., d_used:] = 0
    qk, qe = ops.to_log2_domain(q, dt)
    w = torch.randn(L * H, C_out, device="cuda", generator=g)
    bias = torch.randn(C_out, device="cuda", generator=g)
    return qk.contiguous(), qe, k.to(dt).contiguous(), w, bias


def _tokens(B, T, seed):
    """Row 0: trailing pads, row 1: an interior pad, row 2: nothing but pads; further rows: no pad."""
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(4, 24, (B, T), generator=g)
    tok[:, 0] = CLS
    tok[:, -1] = EOS
    n = max(T // 3, 1)
    tok[0, T - n:] = PAD
    if B > 1 and T >= 5:
        tok[1, T // 2] = PAD
    if B > 2:
        tok[2, :] = PAD
    return tok.cuda()


def _key_bias(tok):
    return torch.where(tok.eq(PAD), float("-inf"), 0.0).float().contiguous()


# (L, H, D slots, head_dim in use, B, T, n_sym, n_asym, dtype, scale, marks): marks = how <pad> reaches the kernel
_CASES = [
    (2, 3, 64, 64, 3, 3, 36, 26, F16, 0.6, "both"),     # S = 1
    (2, 20, 64, 16, 3, 18, 36, 26, BF16, 4.0, "bias"),  # one workgroup tile, second sub-tile partly past T; narrow heads
    (2, 3, 64, 64, 3, 66, 18, 0, F16, 4.0, "tokens"),   # 3 x 3 workgroup tiles, one output half
    (2, 2, 128, 128, 3, 66, 64, 0, BF16, 0.6, "both"),  # 128 slots, 64 outputs
    (2, 2, 128, 128, 3, 130, 1, 0, F16, 4.0, "bias"),   # 5 x 5 tiles, one output, scalar stores
    (2, 3, 64, 64, 3, 130, 0, 1, BF16, 4.0, "both"),    # no symmetric output
    (2, 20, 64, 16, 3, 130, 36, 26, F16, 0.6, "both"),
    (33, 20, 64, 16, 1, 26, 36, 26, F16, 4.0, "none"),  # L*H = 660: lm-design's head on 650M dims
    (2, 3, 64, 64, 2, 33, 17, 18, BF16, 0.6, "both"),   # 35 outputs: second half holds 3, scalar stores
]


@pytest.mark.parametrize("L,H,D,d_used,B,T,n_sym,n_asym,dt,scale,marks", _CASES)
def test_pair_head_op_against_fp64(ops, L, H, D, d_used, B, T, n_sym, n_asym, dt, scale, marks):
    C_out = n_sym + n_asym
    qk, qe, k, w, bias = _operands(ops, L, B, H, T, D, d_used, dt, scale, C_out, seed=T + C_out)
    tok = _tokens(B, T, seed=T) if marks != "none" else _tokens(B + 3, T, seed=T)[3:]
    kb = _key_bias(tok)
    ref = pair_head_ref(qe, k, w, bias, n_sym, key_bias=kb, tokens=tok, pad_idx=PAD)
    got = ops.pair_head(qk, k, ref.lse, w, bias, n_sym=n_sym, key_bias=kb if marks in ("both", "bias") else None,
                        tokens=tok if marks in ("both", "tokens") else None, pad_idx=PAD)
    torch.cuda.synchronize()
    ratio = check_against_ref(got, ref, where=f"T={T} C_out={C_out}")
    print(f"pair_head L={L} H={H} D={D} T={T} outputs={n_sym}+{n_asym}: max |got - ref| / tol = {ratio:.3f}")
    S = T - 2
    if marks != "none":
        # entries that involve a <pad> position hold the bias, exactly; the all-pad row is nothing else
        padm = tok[:, 1:T - 1].eq(PAD)
        anyp = padm[:, :, None] | padm[:, None, :]
        assert torch.equal(got[anyp], bias.expand(int(anyp.sum()), C_out))
        if B > 2:
            assert torch.equal(got[2], bias.expand(S, S, C_out))
    # the symmetric outputs are symmetric bit for bit
    assert torch.equal(got[..., :n_sym], got[..., :n_sym].transpose(1, 2))


def test_pair_head_op_null_key(ops):
    """ESM-1: the learned null key is in the row log-sum-exp and has no column in the map."""
    L, H, D, B, T, n_sym, n_asym = 2, 3, 64, 2, 21, 5, 3
    qk, qe, k, w, bias = _operands(ops, L, B, H, T, D, D, F16, 0.6, n_sym + n_asym, seed=5)
    g = torch.Generator(device="cuda").manual_seed(6)
    null_k = (torch.randn(L, H, D, device="cuda", generator=g) * 0.6).to(F16)
    tok = _tokens(B, T, seed=3)
    ref = pair_head_ref(qe, k, w, bias, n_sym, tokens=tok, pad_idx=PAD, null_k=null_k)
    plain = pair_head_ref(qe, k, w, bias, n_sym, tokens=tok, pad_idx=PAD)
    assert ((ref.z - plain.z).abs() / plain.tol()).max().item() > 10  # the null key matters at this size
    got = ops.pair_head(qk, k, ref.lse, w, bias, n_sym=n_sym, tokens=tok, pad_idx=PAD)
    check_against_ref(got, ref, where="null key")


def test_pair_head_op_batch_invariant(ops):
    """One writer per element, ascending channels: a sequence's map does not depend on the batch it ran in."""
    L, H, D, B, T, n_sym, n_asym = 2, 3, 64, 5, 45, 36, 26
    qk, qe, k, w, bias = _operands(ops, L, B, H, T, D, D, F16, 4.0, n_sym + n_asym, seed=9)
    tok = _tokens(B, T, seed=2)
    ref = pair_head_ref(qe, k, w, bias, n_sym, tokens=tok, pad_idx=PAD)
    full = ops.pair_head(qk, k, ref.lse, w, bias, n_sym=n_sym, tokens=tok, pad_idx=PAD)
    for b in (0, 3):
        one = ops.pair_head(qk[:, b:b + 1].contiguous(), k[:, b:b + 1].contiguous(), ref.lse[:, b:b + 1].contiguous(), w, bias, n_sym=n_sym,
                            tokens=tok[b:b + 1].contiguous(), pad_idx=PAD)
        assert torch.equal(one[0], full[b])


def test_pair_head_op_refusals(ops):
    from esm_amd import _native as N

    L, H, D, B, T = 1, 1, 64, 1, 5
    qk, qe, k, w, bias = _operands(ops, L, B, H, T, D, D, F16, 0.6, 65, seed=1)
    lse = torch.zeros(L, B, H, T, device="cuda", dtype=torch.float64)
    with pytest.raises(N.EsmkError, match="1 .. 64"):
        ops.pair_head(qk, k, lse, w, bias)
    with pytest.raises(N.EsmkError, match="fp16 or bf16"):
        ops.pair_head(qk.float(), k.float(), lse, w[:, :4].contiguous(), None)


# ---- the distogram energy ----------------------------------------------------------------------------------------------
def _energy_case(B, S, width, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    logits = torch.randn(B, S, S, width, device="cuda", generator=g) * 3
    target = torch.randint(0, 18, (S, S), device="cuda", generator=g).to(torch.uint8)
    target[torch.rand(S, S, device="cuda", generator=g) < 0.2] = 255
    return logits, target


@pytest.mark.parametrize("min_sep,inv_temp,first,n_bins", [(0, 1.0, 0, 18), (6, 1.0, 0, 18), (3, 0.37, 18, 18), (0, 2.5, 36, 18)])
def test_distogram_energy_against_fp64(ops, min_sep, inv_temp, first, n_bins):
    B, S = 3, 37
    logits, target = _energy_case(B, S, 62, seed=min_sep + first)
    e, c = ops.distogram_energy(logits, target, first=first, n_bins=n_bins, min_sep=min_sep, inv_temp=inv_temp)
    ref, cnt = distogram_energy_ref(logits[..., first:first + n_bins], target, min_sep, inv_temp)
    assert c.tolist() == [cnt] * B and cnt > 0
    assert ((e - ref).abs() <= 1e-12 * ref.abs()).all(), ((e - ref).abs() / ref.abs()).max().item()
    # a last-axis view of the wide tensor is the same call
    e2, _ = ops.distogram_energy(logits[..., first:first + n_bins], target, min_sep=min_sep, inv_temp=inv_temp)
    assert torch.equal(e, e2)


def test_distogram_energy_ignored_and_empty(ops):
    B, S = 2, 9
    logits, target = _energy_case(B, S, 18, seed=11)
    # only bins <= 5 count (lm-design's dist_cce_pos): the rest become the ignore label
    pos = torch.where(target <= 5, target, torch.full_like(target, 255))
    e, c = ops.distogram_energy(logits, pos)
    ref, cnt = distogram_energy_ref(logits, pos)
    assert c.tolist() == [cnt] * B and ((e - ref).abs() <= 1e-12 * ref.abs()).all()
    none = torch.full_like(target, 255)
    e, c = ops.distogram_energy(logits, none)
    assert e.tolist() == [0.0] * B and c.tolist() == [0] * B
    e, c = ops.distogram_energy(logits, target, min_sep=S)  # no pair that far apart
    assert e.tolist() == [0.0] * B and c.tolist() == [0] * B


def test_distogram_energy_batch_invariant(ops):
    """B = 1 against the same chain inside B = 24: the order of addition does not depend on B."""
    S = 50
    logits, target = _energy_case(24, S, 36, seed=4)
    e, _ = ops.distogram_energy(logits, target, first=0, n_bins=18, min_sep=2, inv_temp=1.3)
    for b in (0, 7, 23):
        one, _ = ops.distogram_energy(logits[b:b + 1], target, first=0, n_bins=18, min_sep=2, inv_temp=1.3)
        assert torch.equal(one[0], e[b])


def test_distogram_energy_refusals(ops):
    from esm_amd import _native as N

    logits, target = _energy_case(1, 4, 18, seed=0)
    with pytest.raises(N.EsmkError, match="inv_temp"):
        ops.distogram_energy(logits, target, inv_temp=0.0)
    with pytest.raises(N.EsmkError, match="min_sep"):
        ops.distogram_energy(logits, target, min_sep=-1)
    with pytest.raises(N.EsmkError, match="inside the ld outputs"):
        ops.distogram_energy(logits, target, first=4, n_bins=18)
