"""The fused contact kernels (csrc/contacts.hip), padded and token-packed, against a streaming fp64 contact head.

Whole-model tests reach these kernels only through the fp16 GEMM floor (5e-3 against the oracle) or by comparing two
engine paths with each other.  Here esmk_op_contacts_fused_ex runs the engine's own launchers (accumulate + reduce per
layer, rt + final once) on q, k and lse the test supplies, and the maps are compared with tests/_contacts_ref.py in
fp64 on the kernel's own operand values: q_effective from ops.to_log2_domain, k rounded to the operand dtype, the same
key bias and token masks, lse = fp32(fp64 logsumexp * log2 e).  A forced head-group count G reaches every (heads per
group, 10-head LDS slab) combination at small sizes: 1, 3, a partial last group, 10, 11, 20 and 40 heads on
head_dim 64; 1, 7, 8 and 20 on head_dim 128 (the 70 KiB LDS form).  Channel counts C = L*H cover the final kernel's
32-channel slabs (1, 31, 32, 33) and real models (660 = 650M, 1440 = 3B, 1920 = 15B); lengths sit on the 32-tile and
128-block edges.

Bound (ContactRef.tol, stated there): the kernel's fp32 error model — chained-MFMA scores, fp32 lse, v_exp_f32, fp32
sums over <= T keys and <= C channels — applied per element to sum_c |w_c| (|a_c| + r_c r_c^T / t_c).  Probabilities
and unsaturated logits are compared against it.  tests/test_contacts_reference_cpu.py shows that dropping one head,
skipping the last 32-channel slab, reading a packed segment one row off, or using the wrong layer's weights moves the
output by at least 10x this bound."""
import math

import pytest
import torch

from _contacts_ref import check_against_ref, contact_ref

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
PAD, EOS, CLS, MASK = 1, 2, 0, 32
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from esm_amd import ops as _ops

    return _ops


def _ceil(a, b):
    return -(-a // b)


def _engine_G(pairs, H, D):
    """contacts_head_groups() of csrc/contacts.hip."""
    G = max(1, min(H, _ceil(1024, max(pairs, 1))))
    hg = _ceil(H, G)
    if D == 128:
        hg = min(hg, 20)
    return _ceil(H, hg)


def _forced_G(H, G):
    return _ceil(H, _ceil(H, G))


def _operands(ops, L, B, H, T, D, dt, scale, seed):
    """q (log2-domain operand, natural-domain value), k; raw scores ~ N(0, (4.8 scale)^2): scale 4 reaches +-100 and
    leaves most of P below the fp32 range.  w ~ N(0, 1), b ~ N(0, 0.3^2): logits of a few units."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    kscale = 0.6 * math.sqrt(64.0 / D)
    qk, qe = ops.to_log2_domain(torch.randn(L, B, H, T, D, device="cuda", generator=g) * scale, dt)
    k = (torch.randn(L, B, H, T, D, device="cuda", generator=g) * kscale).to(dt)
    w = torch.randn(L * H, device="cuda", generator=g)
    b = torch.randn(1, device="cuda", generator=g) * 0.3
    return qk, qe, k, w, b


def _tokens(B, T, bos, eos, masks, seed):
    """Residues 4..23; masks: row 0 trailing pads, row 1 interior pads, <mask> tokens and an <eos> inside the row,
    row 2 (B = 3) an empty sequence (<cls> <eos> <pad>...: no residue)."""
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(4, 24, (B, T), generator=g)
    if bos:
        tok[:, 0] = CLS
    if eos:
        tok[:, -1] = EOS
    if masks and T >= 8:
        n = T // 3
        tok[0, T - n:] = PAD
        if eos:
            tok[0, T - n - 1] = EOS
        if B > 1:
            tok[1, T // 4:T // 4 + 3] = PAD
            tok[1, T // 2] = MASK
            tok[1, T // 2 + 2] = MASK
            tok[1, (2 * T) // 3] = EOS
        if B > 2:
            tok[2, 1] = EOS
            tok[2, 2:] = PAD
    return tok.cuda()


def _key_bias(tok):
    return torch.where(tok.eq(PAD), float("-inf"), 0.0).float().contiguous()


def _padded(ops, D, H, L, B, T, dt, scale, G=0, bos=1, eos=1, masks=False, seed=0):
    qk, qe, k, w, b = _operands(ops, L, B, H, T, D, dt, scale, seed)
    tok = _tokens(B, T, bos, eos, masks, seed)
    kb = _key_bias(tok)
    ref = contact_ref(qe, k, tok, w, b, key_bias=kb, pad_idx=PAD, eos_idx=EOS, bos=bos, eos=eos)
    out, used = ops.contacts_fused(qk, k, ref.lse, tok, w, b, key_bias=kb, pad_idx=PAD, eos_idx=EOS,
                                   prepend_bos=bos, append_eos=eos, head_groups=G)
    torch.cuda.synchronize()
    return out, used, ref, (qk, k, tok, w, b, kb)


# (D, H, L, B, T, G, dtype, scale, masks): forced G -> heads per group (slabs of 10 on head_dim 64), C = L * H
_PADDED = [
    (64, 1, 1, 1, 3, 1, F16, 0.6, False),      # C = 1, S = 1
    (64, 1, 31, 1, 33, 1, BF16, 4.0, False),   # C = 31
    (64, 2, 16, 3, 34, 2, F16, 4.0, True),     # 1 head per group, C = 32, B = 3 with every mask
    (64, 11, 3, 1, 129, 4, BF16, 4.0, False),  # 3 heads per group, partial last group (3,3,3,2), C = 33
    (64, 11, 3, 3, 130, 1, F16, 0.6, True),    # 11 heads: one slab plus one, C = 33
    (64, 20, 33, 1, 127, 2, F16, 4.0, False),  # 10 heads: exactly one slab, C = 660 (650M)
    (64, 20, 1, 1, 257, 1, BF16, 0.6, False),  # 20 heads: two slabs
    (64, 40, 36, 1, 66, 1, BF16, 4.0, False),  # 40 heads: four slabs, C = 1440 (3B production form)
    (64, 40, 1, 2, 128, 13, F16, 4.0, True),   # 4 heads per group
    (64, 2, 1, 1, 4, 1, BF16, 4.0, False),     # S = 2
    (64, 11, 1, 1, 258, 11, BF16, 0.6, False),
    (64, 20, 1, 1, 1026, 2, F16, 4.0, False),  # T ~ 1k: 9 x 9 blocks, S = 1024 = 32 tiles
    (128, 2, 2, 1, 129, 2, F16, 4.0, False),   # head_dim 128, 1 head per group
    (128, 8, 1, 3, 33, 8, BF16, 4.0, True),
    (128, 8, 2, 1, 128, 1, F16, 0.6, False),   # 8 heads per group
    (128, 40, 1, 1, 257, 6, BF16, 4.0, False),  # 7 heads per group (6 groups, the last of 5)
    (128, 40, 48, 1, 130, 2, F16, 4.0, False),  # 20 heads per group (70 KiB LDS), C = 1920 (15B)
    (128, 40, 1, 2, 258, 2, BF16, 0.6, True),
    # appended, so that the ids of the rows above keep their position index
    (64, 11, 2, 3, 130, 4, F16, 4.0, True),    # B = 3, four groups, two query blocks: batch offset, group stride, chunk index
]


@pytest.mark.parametrize("D,H,L,B,T,G,dt,scale,masks", _PADDED)
def test_padded_forced_groups(ops, D, H, L, B, T, G, dt, scale, masks):
    out, used, ref, _ = _padded(ops, D, H, L, B, T, dt, scale, G=G, masks=masks, seed=T + 3 * H + L)
    assert used == _forced_G(H, G)
    assert out.shape == (B, T - 2, T - 2)
    check_against_ref(out, ref, (D, H, L, B, T, G))
    if masks and B == 3:
        assert torch.isnan(out[2]).all()  # no residue: 0/0, as the reference's apc


@pytest.mark.parametrize("bos,eos", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_token_layouts(ops, bos, eos):
    """(1, 1) is ESM-2 / ESM-1b, (1, 0) ESM-1; the other two pin the crop arithmetic of every kernel."""
    out, used, ref, _ = _padded(ops, 64, 4, 2, 2, 45, F16, 4.0, bos=bos, eos=eos, masks=True, seed=7 + 2 * bos + eos)
    assert out.shape == (2, 45 - bos - eos, 45 - bos - eos)
    check_against_ref(out, ref, (bos, eos))


# the engine's own head groups: (D, H, L, B, T, dtype); the G it must report
_ENGINE = [
    (64, 20, 2, 1, 300, BF16),   # 9 block pairs: one head per group
    (64, 20, 1, 2, 1024, F16),   # 128 pairs: G = 8 -> 3 heads per group -> 7 groups
    (64, 40, 1, 16, 1024, BF16),  # 1024 pairs: G = 1, 40 heads in four slabs (3B, full batch)
    (128, 2, 2, 1, 200, F16),
    (128, 40, 1, 8, 1000, F16),  # 512 pairs: G = 2, 20 heads per group (15B, full batch)
]


@pytest.mark.parametrize("D,H,L,B,T,dt", _ENGINE)
def test_engine_head_groups(ops, D, H, L, B, T, dt):
    out, used, ref, _ = _padded(ops, D, H, L, B, T, dt, 4.0, seed=T + B)
    assert used == _engine_G(B * _ceil(T, 128) ** 2, H, D)
    check_against_ref(out, ref, (D, H, L, B, T))


def test_workspace_contents_do_not_matter(ops):
    """The same maps, bit for bit, from a zeroed workspace and one pre-filled with 0xFF (NaN as fp32)."""
    _, used, _, (qk, k, tok, w, b, kb) = _padded(ops, 64, 11, 2, 3, 130, F16, 4.0, G=4, masks=True, seed=5)
    lse = torch.randn(2, 3, 11, 130, device="cuda", dtype=torch.float64) + 5.0
    outs = []
    for fill in (0, 255):
        ws = torch.full((1 << 26,), fill, dtype=torch.uint8, device="cuda")
        o, _ = ops.contacts_fused(qk, k, lse, tok, w, b, key_bias=kb, head_groups=4, workspace=ws)
        outs.append(o.clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


def test_composes_with_attention_lse(ops):
    """lse from the attention kernel itself (ops.attention(..., want_lse=True)) instead of fp64: pins the log2-domain
    handshake between the producer and the contact kernels."""
    D, H, L, B, T = 64, 4, 2, 2, 130
    qk, qe, k, w, b = _operands(ops, L, B, H, T, D, F16, 4.0, seed=31)
    tok = _tokens(B, T, 1, 1, True, 31)
    kb = _key_bias(tok)
    g = torch.Generator(device="cuda").manual_seed(32)
    lse = torch.empty(L, B, H, T, device="cuda")
    for l in range(L):
        v = torch.randn(B, H, T, D, device="cuda", generator=g).to(F16)
        _, lse[l] = ops.attention(qk[l].contiguous(), k[l].contiguous(), ops.make_vt(v), key_bias=kb, want_lse=True)
    ref = contact_ref(qe, k, tok, w, b, key_bias=kb)
    live = tok.ne(PAD)[None, :, None, :].expand(L, B, H, T)
    assert (lse - ref.lse)[live].abs().max().item() < 1e-3
    out, _ = ops.contacts_fused(qk, k, lse, tok, w, b, key_bias=kb)
    check_against_ref(out, ref, "attention lse")


# ---- token-packed form ------------------------------------------------------------------------------------------
# (first row, length), in table order: unsorted, gaps between segments, the first at row 40; empty segments (len 2,
# 1, 0 <= bos + eos), a segment with no residues (<cls> <pad>... <eos>), lengths on the 32 / 128 / 256 edges
_SEGS = [(700, 258), (40, 34), (90, 2), (120, 129), (300, 256), (560, 1), (600, 0), (610, 33), (660, 20), (980, 130),
         (1120, 128), (1260, 3), (1270, 257)]
_ROWS = 1540
_NORES = 8  # index of the no-residue segment


def _packed_inputs(ops, D, H, L, dt, scale, seed):
    qk, qe, k, w, b = _operands(ops, L, 1, H, _ROWS, D, dt, scale, seed)
    qk, qe, k = qk[:, 0], qe[:, 0], k[:, 0]  # [L, H, rows, D]
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(0, 33, (_ROWS,), generator=g)
    gap = torch.ones(_ROWS, dtype=torch.bool)
    for i, (r0, n) in enumerate(_SEGS):
        gap[r0:r0 + n] = False
        if n >= 1:
            tok[r0:r0 + n] = torch.randint(4, 24, (n,), generator=g)
            tok[r0] = CLS
            tok[r0 + n - 1] = EOS
            if n > 40:
                tok[r0 + n // 2:r0 + n // 2 + 2] = PAD  # pads inside a segment
                tok[r0 + n // 3] = MASK
        if i == _NORES:
            tok[r0 + 1:r0 + n - 1] = PAD
    tok = tok.cuda()
    gap = gap.cuda()
    kb = _key_bias(tok)
    kb[gap] = NAN
    for t in (qk, qe, k):
        t[:, :, gap] = NAN
    return qk, qe, k, w, b, tok, kb, gap


def _packed_refs(qe, k, tok, kb, w, b):
    """fp64 reference of every segment as the sequence alone, and the [L, H, rows] lse (NaN in the gaps)."""
    L, H, rows, D = qe.shape
    lse = torch.full((L, H, rows), NAN, dtype=torch.float64, device="cuda")
    refs = []
    for r0, n in _SEGS:
        if n - 2 <= 0:
            refs.append(None)
            continue
        sl = slice(r0, r0 + n)
        ref = contact_ref(qe[:, :, sl][:, None], k[:, :, sl][:, None], tok[None, sl], w, b, key_bias=kb[None, sl])
        lse[:, :, sl] = ref.lse[:, 0]
        refs.append(ref)
    return refs, lse


@pytest.mark.parametrize("D,H,L,G,dt", [(64, 20, 2, 0, F16), (64, 40, 1, 1, BF16), (128, 20, 2, 0, BF16),
                                        (128, 40, 1, 2, F16)])
def test_packed_segments(ops, D, H, L, G, dt):
    qk, qe, k, w, b, tok, kb, gap = _packed_inputs(ops, D, H, L, dt, 4.0, seed=D + H)
    refs, lse = _packed_refs(qe, k, tok, kb, w, b)
    n_out = sum(max(n - 2, 0) ** 2 for _, n in _SEGS)
    sentinel = 12345.0
    out = torch.full((n_out + 4096,), sentinel, device="cuda")
    _, used = ops.contacts_fused(qk, k, lse, tok, w, b, key_bias=kb, segments=_SEGS, head_groups=G, out=out)
    torch.cuda.synchronize()
    pairs = sum(_ceil(n, 128) ** 2 for _, n in _SEGS if n > 2)
    assert used == (_forced_G(H, G) if G else _engine_G(pairs, H, D))
    assert (out[n_out:] == sentinel).all()  # nothing past the ragged maps
    off = 0
    for i, ((r0, n), ref) in enumerate(zip(_SEGS, refs)):
        if ref is None:
            continue
        S = n - 2
        got = out[off:off + S * S].view(1, S, S)
        off += S * S
        check_against_ref(got, ref, (D, H, i, r0, n))
        if i == _NORES:
            assert torch.isnan(got).all()
    assert off == n_out

    # a segment equals the padded form of the same sequence at the same G, bit for bit
    for i in (0, 3):
        r0, n = _SEGS[i]
        sl = slice(r0, r0 + n)
        pad_out, pad_used = ops.contacts_fused(qk[:, :, sl][:, None].contiguous(), k[:, :, sl][:, None].contiguous(),
                                               lse[:, :, sl][:, None].contiguous(), tok[None, sl].contiguous(), w, b,
                                               key_bias=kb[None, sl].contiguous(), head_groups=used)
        assert pad_used == used
        o = sum((m - 2) ** 2 for _, m in _SEGS[:i] if m > 2)
        assert torch.equal(out[o:o + (n - 2) ** 2].view(n - 2, n - 2), pad_out[0]), i

    # the workspace's previous contents do not matter
    ws = torch.full((1 << 27,), 255, dtype=torch.uint8, device="cuda")
    out2, _ = ops.contacts_fused(qk, k, lse, tok, w, b, key_bias=kb, segments=_SEGS, head_groups=G, workspace=ws)
    assert torch.equal(out[:n_out].view(torch.int32), out2.view(torch.int32))


def test_packed_all_segments_empty(ops):
    """Only maps of size 0: nothing is launched and the output is untouched."""
    qk, qe, k, w, b = _operands(ops, 1, 1, 4, 128, 64, F16, 1.0, seed=3)
    tok = _tokens(1, 128, 1, 1, False, 3)[0]
    lse = torch.zeros(1, 4, 128, dtype=torch.float64, device="cuda")
    out = torch.full((16,), 7.0, device="cuda")
    ops.contacts_fused(qk[:, 0], k[:, 0], lse, tok, w, b, segments=[(0, 2), (10, 1), (64, 0)], out=out)
    torch.cuda.synchronize()
    assert (out == 7.0).all()
