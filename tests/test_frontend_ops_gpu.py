"""The token front end of libesmk.so one kernel at a time (csrc/elementwise.hip: seq_stats, packed_stats, zero_gap_rows,
embed, embed_esm1, add_positions, scale_rows, msa_embed, sinus_table, rope_table; csrc/scoring.hip: gather_rows), through
the validated C entries (include/esmk.h, esmk_op_seq_stats ... esmk_op_gather_rows) against the plain references of
tests/_frontend_ref.py (pinned to the oracles in tests/test_frontend_reference_cpu.py).

Integer bookkeeping and everything that is one or two fp32 operations in a fixed order is compared bit for bit; the ESM-1
embedding (a multiply-add the compiler may contract) and the position tables (device sinf / cosf) carry bounds that come
from the number format, not from what the kernels give.  Every output buffer ends in a tail of sentinel elements, and the
tail and every element the contract leaves unwritten must come back unchanged.
"""
import math

import pytest
import torch

import _frontend_ref as R
from esm_amd import ops
from test_c_abi_validation_cpu import PACKED_SEGS_A, PACKED_SEGS_B

pytestmark = pytest.mark.gpu
PAD, MASK, VOCAB = 1, 32, 33
TAIL = 64
F_SENT, I_SENT = -777.25, -12345


class Guarded:
    """A device buffer of `shape` followed by TAIL sentinel elements; `fill` None = sentinels everywhere."""

    def __init__(self, shape, dtype=torch.float32, fill=None):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.sent = F_SENT if dtype.is_floating_point else I_SENT
        self.buf = torch.full((n + TAIL,), self.sent, dtype=dtype, device="cuda")
        if fill is not None:
            self.buf[:n] = fill.reshape(-1).to("cuda")
        self.t = self.buf[:n].view(shape)

    def cpu(self):
        return self.t.cpu()

    def tail_intact(self):
        return bool((self.buf[self.n:] == self.sent).all())

    def untouched(self):
        return bool((self.buf == self.sent).all())


def rand_tokens(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(4, 24, shape, generator=g, dtype=torch.int64)


def randn(shape, seed, std=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * std


# ---- seq_stats ------------------------------------------------------------------------------------------------------------
def stats_batch(T):
    """One batch per T: the rows the kernel's sweeps, reductions and `last` bookkeeping can get wrong."""
    base = rand_tokens((T,), seed=T)
    rows = [base.clone()]  # no pad

    def add(edit):
        r = base.clone()
        edit(r)
        rows.append(r)

    if T >= 2:
        add(lambda r: r.__setitem__(slice(T - max(1, T // 3), T), PAD))  # trailing pads
        add(lambda r: r.__setitem__(0, PAD))  # a leading pad
    if T >= 3:
        add(lambda r: r.__setitem__(T // 2, PAD))  # one interior pad
    if T >= 5:  # token, pad, token, pad, pad at the end of the row
        def tptpp(r):
            r[T - 4], r[T - 2], r[T - 1] = PAD, PAD, PAD
        add(tptpp)

        def masks_by_pads(r):  # masks next to pads
            r[1], r[2], r[3] = MASK, PAD, MASK
            r[T - 1], r[T - 2] = PAD, MASK
        add(masks_by_pads)
    if T > 256:
        add(lambda r: r.__setitem__(torch.tensor([3, 200, 255]), PAD))  # pads only in the first sweep
        add(lambda r: r.__setitem__(torch.tensor([256, min(257, T - 1), T - 1]), PAD))  # pads only behind it
        add(lambda r: r.__setitem__(torch.tensor([255, 256]), PAD))  # on both sides of the boundary
    rows.append(torch.full((T,), PAD, dtype=torch.int64))
    rows.append(torch.full((T,), MASK, dtype=torch.int64))
    return torch.stack(rows)


@pytest.mark.parametrize("with_keep", [False, True])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 255, 256, 257, 1026])
def test_seq_stats(T, with_keep):
    tokens = stats_batch(T)
    B = tokens.shape[0]
    scale, key_bias, info, keep = R.seq_stats_ref(tokens, PAD, MASK)
    g_scale, g_kb, g_keep = Guarded((B,)), Guarded((B, T)), Guarded((B, T))
    g_info = Guarded((B, 2), torch.int32)
    ops.seq_stats(tokens.cuda(), PAD, MASK, want_keep=with_keep, scale=g_scale.t, key_bias=g_kb.t, seq_info=g_info.t,
                  keep=g_keep.t if with_keep else None)
    assert torch.equal(g_info.cpu(), info), (g_info.cpu().tolist(), info.tolist())
    assert torch.equal(R.bits(g_kb.cpu()), R.bits(key_bias))  # exactly +0 / -inf
    assert R.same_bits(g_scale.cpu(), scale)
    assert math.isnan(g_scale.cpu()[-2].item()) and R.bits(g_scale.cpu())[-1].item() == 0  # all <pad>: NaN; all <mask>: +0
    if with_keep:
        assert torch.equal(R.bits(g_keep.cpu()), R.bits(keep)) and g_keep.tail_intact()
    else:
        assert g_keep.untouched()
    assert g_scale.tail_intact() and g_kb.tail_intact() and g_info.tail_intact()


# ---- packed_stats / zero_gap_rows -----------------------------------------------------------------------------------------
def pairs(flat):
    return [(flat[i], flat[i + 1]) for i in range(0, len(flat), 2)]


# a segment of more than one sweep followed by a gap, a segment of one row, two adjacent segments, the last one ending at `rows`
SEGS_C = [(0, 300), (304, 1), (320, 32), (352, 32)]
PACKED_TABLES = [(pairs(PACKED_SEGS_A[0]), PACKED_SEGS_A[1]), (pairs(PACKED_SEGS_B[0]), PACKED_SEGS_B[1]), (SEGS_C, 384),
                 (SEGS_C, 448)]  # ... and the same with a trailing gap


def packed_tokens(segs, rows, seed=0):
    t = rand_tokens((rows,), seed=seed + rows)
    t[::7] = PAD  # gap rows hold anything, pads included: the table decides, not the token
    for start, n in segs:
        t[start:start + n] = rand_tokens((n,), seed=seed + start + 1)
        if n >= 3:
            t[start + 1], t[start + n - 1] = MASK, PAD
        if n >= 9:
            t[start + 4], t[start + 5], t[start + 6] = PAD, MASK, PAD
        if n > 256:
            t[start + 255], t[start + 256], t[start + 258] = PAD, PAD, MASK
    return t


@pytest.mark.parametrize("with_keep", [False, True])
@pytest.mark.parametrize("table", range(len(PACKED_TABLES)))
def test_packed_stats(table, with_keep):
    segs, rows = PACKED_TABLES[table]
    tokens = packed_tokens(segs, rows)
    scale_row, key_bias, row_pos, npad, keep = R.packed_stats_ref(tokens, segs, PAD, MASK)
    g_scale, g_kb, g_keep = Guarded((rows,)), Guarded((rows,)), Guarded((rows,))
    g_pos, g_npad = Guarded((rows,), torch.int32), Guarded((len(segs),), torch.int32)
    ops.packed_stats(tokens.cuda(), segs, PAD, MASK, want_keep=with_keep, scale_row=g_scale.t, key_bias=g_kb.t, row_pos=g_pos.t,
                     seg_npad=g_npad.t, keep=g_keep.t if with_keep else None)
    assert torch.equal(g_npad.cpu(), npad)
    assert torch.equal(g_pos.cpu(), row_pos)
    assert torch.equal(R.bits(g_kb.cpu()), R.bits(key_bias))
    assert R.same_bits(g_scale.cpu(), scale_row)
    gap = R.gap_rows(segs, rows)
    assert gap.any()
    assert (g_scale.cpu()[gap] == 1.0).all() and (g_kb.cpu()[gap] == float("-inf")).all() and not g_pos.cpu()[gap].any()
    if with_keep:
        assert torch.equal(R.bits(g_keep.cpu()), R.bits(keep)) and not g_keep.cpu()[gap].any() and g_keep.tail_intact()
    else:
        assert g_keep.untouched()
    assert g_scale.tail_intact() and g_kb.tail_intact() and g_pos.tail_intact() and g_npad.tail_intact()


@pytest.mark.parametrize("row_bytes", [16, 640, 2560])
def test_zero_gap_rows(row_bytes):
    nan_bits = 0x7FC00001
    for segs, rows in PACKED_TABLES:
        w = row_bytes // 4
        buf = torch.full((rows * w + TAIL,), nan_bits, dtype=torch.int32, device="cuda")
        ops.zero_gap_rows(buf, segs, rows, row_bytes)
        got = buf.cpu()
        body = got[:rows * w].view(rows, w)
        gap = R.gap_rows(segs, rows)
        assert (body[gap] == 0).all() and (body[~gap] == nan_bits).all() and (got[rows * w:] == nan_bits).all(), (segs, rows)


# ---- embed ----------------------------------------------------------------------------------------------------------------
# (B, T, E): B T E / 4 = 10 (below one workgroup), 256 (exactly one), 504 and 1440 (more than one, not a multiple of 256)
EMBED_SHAPES = [(2, 5, 4), (4, 64, 4), (3, 7, 96), (2, 9, 320)]
assert [b * t * e // 4 for b, t, e in EMBED_SHAPES] == [10, 256, 504, 1440]


def embed_tokens(B, T, mask=MASK, vocab=VOCAB, seed=0):
    """Rows with <mask>, <pad>, and — guarded in both kernels by `tok >= 0 && tok < vocab` (a zero row) — -1 and vocab."""
    t = rand_tokens((B, T), seed=seed + 100 * B + T)
    t[0, 1], t[0, 2] = mask, PAD
    t[1, 0], t[1, T - 1] = PAD, mask
    t[0, 3], t[1, 3] = -1, vocab
    if B > 2:
        t[2] = PAD  # a row of padding only: scale = NaN, the rows are zeroed all the same
        t[B - 1, T - 2:] = PAD
    return t


@pytest.mark.parametrize("token_dropout", [0, 1])
@pytest.mark.parametrize("B,T,E", EMBED_SHAPES)
def test_embed(B, T, E, token_dropout):
    tokens = embed_tokens(B, T)
    table = randn((VOCAB, E), seed=E)
    scale = R.seq_stats_ref(tokens, PAD, MASK)[0]
    want = R.embed_ref(tokens, table, scale, PAD, MASK, bool(token_dropout))
    out = Guarded((B, T, E))
    ops.embed(tokens.cuda(), table.cuda(), scale.cuda(), PAD, MASK, bool(token_dropout), out=out.t)
    got = out.cpu()
    assert R.same_bits(got, want)
    assert not got[tokens.eq(PAD)].any() and not got[0, 3].any() and not got[1, 3].any() and out.tail_intact()
    assert R.bits(got[tokens.eq(PAD)]).eq(0).all()  # +0, not -0
    # the engine's packed form: B = rows, T = 1, a divisor per row (launch_packed_stats' scale_row)
    rows = B * T
    scale_row = scale.repeat_interleave(T)
    out2 = Guarded((rows, 1, E))
    ops.embed(tokens.view(rows, 1).cuda(), table.cuda(), scale_row.cuda(), PAD, MASK, bool(token_dropout), out=out2.t)
    assert R.same_bits(out2.cpu().view(B, T, E), want) and out2.tail_intact()


@pytest.mark.parametrize("token_dropout", [0, 1])
@pytest.mark.parametrize("B,T,E", EMBED_SHAPES)
def test_embed_esm1(B, T, E, token_dropout):
    """Not a bit test: hipcc may contract v * embed_scale + pe into one fma.  Bound per element, against fp64:
    3 * 2^-24 * (|embed_scale e| / |scale| + |pe|) — at most three roundings, each at most half an ulp of an intermediate
    no larger than that sum.  Pad rows (no position term: no addition) are bit-determined."""
    mask, vocab = 33, 35
    tokens = embed_tokens(B, T, mask=mask, vocab=vocab, seed=1)
    table = randn((vocab, E), seed=E + 1, std=0.5 / math.sqrt(E))
    sinus = R.sinus_table_ref(R.sinus_freq(max(E // 2, 2)), T, PAD + 1).float()[:, :E].contiguous()
    scale = R.seq_stats_ref(tokens, PAD, mask)[0]
    es = math.sqrt(E)
    ref, bound = R.embed_esm1_ref(tokens, table, scale, sinus, es, PAD, mask, bool(token_dropout))
    out = Guarded((B, T, E))
    ops.embed_esm1(tokens.cuda(), table.cuda(), sinus.cuda(), es, scale.cuda(), PAD, mask, bool(token_dropout), out=out.t)
    got = out.cpu()
    nan = torch.isnan(ref)  # the row of padding only under token dropout: 0 / 0 on both sides
    assert torch.equal(torch.isnan(got), nan) and bool(nan.any()) == (bool(token_dropout) and B > 2)
    err = (got.double() - ref).abs()
    ratio = (err[~nan] / bound[~nan].clamp_min(1e-300)).max().item()
    print(f"\nembed_esm1 B={B} T={T} E={E} dropout={token_dropout}: max err / bound = {ratio:.3f}, max err {err[~nan].max().item():.3e}")
    assert (err[~nan] <= bound[~nan]).all()
    pads = tokens.eq(PAD)
    fixed = R.embed_esm1_pad_rows_ref(tokens, table, scale, es, mask, bool(token_dropout))
    assert R.same_bits(got[pads], fixed[pads])  # the scaled embedding, no position term
    # out-of-range tokens: a zero embedding row, the position term alone
    assert torch.equal(got[0, 3], sinus[3]) and torch.equal(got[1, 3], sinus[3])
    assert out.tail_intact()


# ---- add_positions / scale_rows -------------------------------------------------------------------------------------------
NPOS, PE = 1026, 96
POSITION_T = [5, 256, 257, 600]  # three rows each: rows E / 4 is no multiple of 256 but at T = 256
assert [3 * T * PE // 4 % 256 != 0 for T in POSITION_T] == [True, False, True, True]


@pytest.fixture(scope="module")
def pos_emb():
    t = randn((NPOS, PE), seed=11, std=0.1)
    t[PAD] = 0.0
    return t


def position_tokens(T):
    t = rand_tokens((3, T), seed=40 + T)
    for c in (255, 256, 257, 511, 512):  # pads on both sides of the 256-row sweep boundaries
        if c < T:
            t[0, c] = PAD
    t[1, 0] = PAD
    t[1, T // 2] = PAD
    t[1, T - 1] = PAD
    for c in (255, 511):  # one pad in front of each boundary only: a carry that drops it shows on every later row
        if c < T:
            t[2, c] = PAD
    return t


@pytest.mark.parametrize("T", POSITION_T)
def test_add_positions_and_scale_rows(T, pos_emb):
    tokens = position_tokens(T)
    B = tokens.shape[0]
    x0 = randn((B, T, PE), seed=T)
    want = R.add_positions_ref(x0, tokens, pos_emb, PAD)
    x = Guarded((B, T, PE), fill=x0)
    ops.add_positions(tokens.cuda(), pos_emb.cuda(), x.t, PAD)
    got = x.cpu()
    assert R.same_bits(got, want) and x.tail_intact()
    assert R.same_bits(got[tokens.eq(PAD)], (x0 + pos_emb[PAD])[tokens.eq(PAD)])  # pads take row pad_idx
    # esm1.py:138-139: rows times keep — bit-equal or exactly zero
    keep = tokens.ne(PAD).float().view(-1)
    ops.scale_rows(x.t.view(B * T, PE), keep.cuda())
    got2 = x.cpu()
    assert R.same_bits(got2, want * keep.view(B, T, 1)) and x.tail_intact()
    assert not got2[tokens.eq(PAD)].any() and R.same_bits(got2[tokens.ne(PAD)], want[tokens.ne(PAD)])


def test_add_positions_packed(pos_emb):
    segs, rows = [(0, 300), (304, 7)], 320
    tokens = rand_tokens((rows,), seed=9)
    tokens[[255, 256, 257, 299, 306]] = PAD
    tokens[300:304] = PAD  # gap rows: not a segment's
    x0 = randn((rows, PE), seed=10)
    want = R.add_positions_packed_ref(x0, tokens, pos_emb, segs, PAD)
    x = Guarded((rows, PE), fill=x0)
    ops.add_positions(tokens.cuda(), pos_emb.cuda(), x.t, PAD, segments=segs, longest=300)
    got = x.cpu()
    assert R.same_bits(got, want) and x.tail_intact()
    gap = R.gap_rows(segs, rows)
    assert R.same_bits(got[gap], x0[gap])  # rows outside every segment are not touched
    assert R.same_bits(got[304:311], R.add_positions_ref(x0[None, 304:311], tokens[None, 304:311], pos_emb, PAD)[0])


# ---- msa_embed ------------------------------------------------------------------------------------------------------------
# (B, R, C, D): 1, 2, 3, 5 and 16 column chunks of ceil(C / chunks) columns — the last chunk is shorter at 65, 130 and 1030
# (300 = 5 x 60 divides); 300 and 1030 cross the 256-column sweep
MSA_SHAPES = [(1, 1, 1, 4), (2, 3, 65, 96), (1, 5, 130, 320), (1, 2, 300, 96), (1, 1, 1030, 4)]
MSA_NPOS = 1030 + PAD + 1


def msa_tokens(B, R, C, padded):
    t = rand_tokens((B, R, C), seed=C)
    if not padded:
        return t
    chunks = max(1, min(16, (C + 63) // 64))
    cper = (C + chunks - 1) // chunks
    cols = [k * cper - 1 for k in range(1, chunks)] + [k * cper for k in range(1, chunks)] + [255, 256, C - 1]
    for i, c in enumerate(sorted(set(c for c in cols if 0 <= c < C))):
        t[i % B, i % R, c] = PAD  # pads at the column-chunk seams and at the sweep boundary, spread over the rows
    t[B - 1, R - 1, 0] = PAD  # a leading pad (C = 1: the only token)
    return t


@pytest.mark.parametrize("with_msa_pos", [False, True])
@pytest.mark.parametrize("B,Rm,C,D", MSA_SHAPES)
def test_msa_embed(B, Rm, C, D, with_msa_pos):
    tok_emb = randn((VOCAB, D), seed=D)
    pos = randn((MSA_NPOS, D), seed=D + 1, std=0.1)
    msa_pos = randn((Rm + 2, D), seed=D + 2, std=0.1) if with_msa_pos else None
    dev = lambda t: None if t is None else t.cuda()  # noqa: E731
    g_any = Guarded((1,), torch.int32)
    for padded in (True, False):  # the pad-free batch runs second: any_pad must be reset, not only set
        tokens = msa_tokens(B, Rm, C, padded)
        x, keep, col_fill, any_pad = R.msa_embed_ref(tokens, tok_emb, pos, msa_pos, PAD)
        assert any_pad == padded
        g_x, g_keep, g_fill = Guarded((B, Rm, C, D)), Guarded((B, Rm, C)), Guarded((B, C, Rm))
        ops.msa_embed(tokens.cuda(), tok_emb.cuda(), pos.cuda(), dev(msa_pos), PAD, x=g_x.t, keep=g_keep.t, col_fill=g_fill.t,
                      any_pad=g_any.t)
        assert g_any.cpu().item() == int(padded), (padded, g_any.cpu().item())
        assert R.same_bits(g_x.cpu(), x)
        assert torch.equal(R.bits(g_keep.cpu()), R.bits(keep))
        assert torch.equal(R.bits(g_fill.cpu()), R.bits(col_fill))  # (b, c)-major: [B, C, R]
        assert g_x.tail_intact() and g_keep.tail_intact() and g_fill.tail_intact() and g_any.tail_intact()


# ---- position tables ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [8, 32, 64])
def test_rope_table(half):
    """|device cosf / sinf - fp64 cos / sin of the same fp32 angle| <= 2^-22 (4 fp32 ulp at 1.0; the precise functions are a few
    ulp, the fast hardware path misses by ~1e-4 at 1000 rad).  The ROCm installation this was written against carries no HIP
    math accuracy table, so the bound is the stated one."""
    T = 1030
    inv = R.rope_inv_freq(2 * half)
    cos64, sin64 = R.rope_table_ref(inv, T)
    g_cos, g_sin = Guarded((T, half)), Guarded((T, half))
    ops.rope_table(inv.cuda(), T, cos=g_cos.t, sin=g_sin.t)
    ec = (g_cos.cpu().double() - cos64).abs().max().item()
    es = (g_sin.cpu().double() - sin64).abs().max().item()
    print(f"\nrope_table half={half}: max |cos err| {ec:.3e}, max |sin err| {es:.3e} (bound {R.TABLE_BOUND:.3e})")
    assert ec <= R.TABLE_BOUND and es <= R.TABLE_BOUND
    assert g_cos.cpu().shape == (T, half) and (g_cos.cpu()[0] == 1).all() and not g_sin.cpu()[0].any()  # [T, half], row 0 = angle 0
    assert g_cos.tail_intact() and g_sin.tail_intact()


@pytest.mark.parametrize("half", [2, 160])
def test_sinus_table(half):
    T, pos0 = 1030, 2
    freq = R.sinus_freq(half)
    want = R.sinus_table_ref(freq, T, pos0)
    g = Guarded((T, 2 * half))
    ops.sinus_table(freq.cuda(), T, pos0, out=g.t)
    got = g.cpu()
    e_sin = (got[:, :half].double() - want[:, :half]).abs().max().item()
    e_cos = (got[:, half:].double() - want[:, half:]).abs().max().item()
    print(f"\nsinus_table half={half}: max |sin err| {e_sin:.3e}, max |cos err| {e_cos:.3e} (bound {R.TABLE_BOUND:.3e})")
    assert e_sin <= R.TABLE_BOUND and e_cos <= R.TABLE_BOUND
    # layout: sin | cos halves, row stride 2 half; column 0 has frequency 1: row t holds sin / cos of pos0 + t
    a = torch.arange(pos0, pos0 + T, dtype=torch.float64)
    assert (got[:, 0].double() - torch.sin(a)).abs().max().item() <= R.TABLE_BOUND
    assert (got[:, half].double() - torch.cos(a)).abs().max().item() <= R.TABLE_BOUND
    assert g.tail_intact()


# ---- gather_rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 300])
@pytest.mark.parametrize("E", [4, 320])
def test_gather_rows(E, n):
    """sel is device data: gather_rows_kernel clamps it (`min(max(sel[i], 0), N - 1)`), so -3 reads row 0 and N + 5 row N - 1."""
    N = 37
    x = randn((N, E), seed=E + n)
    sel = torch.randint(0, N, (n,), generator=torch.Generator().manual_seed(n), dtype=torch.int32)
    if n == 1:
        sels = [torch.tensor([v], dtype=torch.int32) for v in (0, N - 1, -3, N + 5)]
    else:
        sel[:8] = torch.tensor([0, N - 1, -3, N + 5, 7, 7, 7, 0], dtype=torch.int32)
        sels = [sel]
    for s in sels:
        out = Guarded((n, E))
        ops.gather_rows(x.cuda(), s.cuda(), out=out.t)
        assert R.same_bits(out.cpu(), R.gather_rows_ref(x, s)) and out.tail_intact(), s[:8].tolist()
