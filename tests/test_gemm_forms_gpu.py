"""The generalised-addressing forms of the persistent GEMM (gemm8_kernel<..., GEN = true>) and the tied row-attention
softmax, one launch at a time (esmk_op_gemm_ex, esmk_op_msa_row_softmax), against the fp64 reference of
tests/_gemm_ref.py with its per-element bound.

Guards: every operand sits inside a larger buffer whose elements outside the logical view are NaN, so a stray read
shows as NaN in the output; every output region sits inside a buffer filled with a sentinel bit pattern, and after each
launch the sentinels outside what the form writes (the guard zones, gaps between ldc and N, other layers, the [T, Tp)
key padding) must be unchanged."""
import math

import pytest
import torch

import _gemm_ref as G

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
PAD = 4096
SENT = {torch.float32: 0x7FA5A5A5, torch.float16: 0x7DA5, torch.bfloat16: 0x7FA5}
LOG2E = 1.4426950408889634
H12, E768 = 12, 768


@pytest.fixture(scope="module")
def ops():
    from esm_amd import ops as _ops

    return _ops


def ceil64(n):
    return (n + 63) // 64 * 64


def operand(t):
    """t inside a NaN-guarded buffer (same dtype and shape).  Integer tensors (row positions) are guarded by 0: a position
    read from outside the view stays inside the rotary table instead of reading past it."""
    fill = float("nan") if t.dtype.is_floating_point else 0
    buf = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype, device="cuda")
    v = buf[PAD:PAD + t.numel()]
    v.copy_(t.reshape(-1))
    return v.view(t.shape)


class Out:
    """An output region of n elements inside a sentinel-filled buffer."""

    def __init__(self, n, dtype):
        self.dtype = dtype
        self.buf = torch.empty(n + 2 * PAD, dtype=dtype, device="cuda")
        self.bits().fill_(SENT[dtype])
        self.v = self.buf[PAD:PAD + n]

    def bits(self):
        return self.buf.view(torch.int32 if self.dtype == torch.float32 else torch.int16)

    def check(self, written=None):
        torch.cuda.synchronize()
        same = self.bits() == SENT[self.dtype]
        assert bool(same[:PAD].all()) and bool(same[-PAD:].all()), "a store left the output region"
        if written is not None:
            assert bool(same[PAD:-PAD][~written.reshape(-1)].all()), "a store outside the form's output layout"


def within(got, val, bnd, what):
    err = (got.double() - val).abs()
    bad = ~(err <= bnd)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the fp64 bound; first flat "
                             f"index {i}: got {got.reshape(-1)[i].item()} want {val.reshape(-1)[i].item()} "
                             f"bound {bnd.reshape(-1)[i].item()}")


def rnd(*shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(dtype)


def bits_equal(a, b):
    ib = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.contiguous().view(ib), b.contiguous().view(ib))


# ---------------------------------------------------------------------------------------------------------------------
# tied row-attention scores (engine_msa.hip:284-306)
# ---------------------------------------------------------------------------------------------------------------------
SCORE_CELLS = [  # (C, R, B, S); "e" = the engine's row_score_slices
    (1, 1, 1, 1), (2, 2, 2, 2), (63, 3, 1, 3), (64, 8, 2, 8), (65, 7, 1, 7), (255, 64, 1, 4), (256, 8, 2, "e"),
    (257, 7, 2, 7), (257, 64, 2, "e"), (1023, 2, 2, 2), (1024, 1, 1, 1), (1024, 8, 1, "e"), (100, 30, 1, 5),
    (100, 30, 2, 6), (128, 256, 1, 8),
]


def tied_scores(ops, q, k, B, R, C, S, H):
    """the engine's launch: q, k [B, R, H, C, 64] (the QKV epilogue's [(b, r), H, C, 64]) -> fp32 [B, S, H, C, Cp]."""
    Cp, os_, Rs = ceil64(C), q.element_size(), R // S
    out = Out(B * S * H * C * Cp, torch.float32)
    ops.gemm_ex(1, A=q, W=k, out=out.v, M=C, N=Cp, n_valid=C, K=Rs * 64, ldc=Cp, a_row_bytes=128, w_row_bytes=128,
                a_kt_bytes=H * C * 64 * os_, w_kt_bytes=H * C * 64 * os_, batch=B * S * H, batch_inner=H,
                a_bo=Rs * H * C * 64 * os_, w_bo=Rs * H * C * 64 * os_, a_bi=C * 64 * os_, w_bi=C * 64 * os_,
                o_bo=H * C * Cp * 4, o_bi=C * Cp * 4)
    out.check()
    return out.v.view(B, S, H, C, Cp)


@pytest.mark.parametrize("C,R,B,S", SCORE_CELLS)
@pytest.mark.parametrize("dt", DT)
def test_tied_scores(ops, C, R, B, S, dt):
    H = H12
    if S == "e":
        S = G.row_score_slices(B, H, R, C)
    q = operand(rnd(B, R, H, C, 64, seed=C + R, scale=0.125, dtype=dt))
    k = operand(rnd(B, R, H, C, 64, seed=C * R + 1, dtype=dt))
    got = tied_scores(ops, q, k, B, R, C, S, H)
    parts, pb = G.row_scores(q.permute(1, 3, 0, 2, 4), k.permute(1, 3, 0, 2, 4), S)
    Cp = ceil64(C)
    within(got[..., :C], G.scores_layout(parts, Cp)[..., :C], G.scores_layout(pb, Cp)[..., :C], "scores")


@pytest.mark.parametrize("n_valid", [200, 256])
@pytest.mark.parametrize("dt", DT)
def test_whole_tile_past_n_valid(ops, n_valid, dt):
    """N = 512: the second 256-column tile lies wholly past n_valid (gemm8.hip set_tile, lim < 0); W holds n_valid rows."""
    M, N, K = 300, 512, 192
    a = operand(rnd(M, K, seed=1, dtype=dt))
    w = operand(rnd(n_valid, K, seed=2, dtype=dt))
    bias = operand(rnd(N, seed=3))
    out = Out(M * N, torch.float32)
    ops.gemm_ex(1, A=a, W=w, bias=bias, out=out.v, M=M, N=N, K=K, n_valid=n_valid, ldc=N)
    out.check()
    y, b = G.dense(a, w, bias[:n_valid])
    within(out.v.view(M, N)[:, :n_valid], y, b, "n_valid")


# ---------------------------------------------------------------------------------------------------------------------
# row softmax (elementwise.hip msa_row_softmax_kernel)
# ---------------------------------------------------------------------------------------------------------------------
SOFTMAX_CELLS = [  # (B, R, C, nslice, any_pad, pads: "row0" | "others" | None, layer, Ltot)
    (1, 1, 1, 1, 0, None, 0, 1), (2, 3, 65, 2, 1, "row0", 1, 3), (1, 4, 257, 3, 1, "others", 0, 2),
    (2, 5, 100, 4, 0, "row0", 2, 3), (1, 5, 1024, 5, 1, "row0", 0, 1), (1, 6, 513, 6, 1, "row0", 3, 4),
    (2, 7, 31, 7, 1, "others", 0, 1), (1, 8, 1000, 8, 1, "row0", 1, 2),
]


@pytest.mark.parametrize("B,R,C,S,any_pad,pads,layer,Ltot", SOFTMAX_CELLS)
@pytest.mark.parametrize("dt", DT)
def test_row_softmax(ops, B, R, C, S, any_pad, pads, layer, Ltot, dt):
    H, Cp = 3, ceil64(C)
    sc = rnd(B, S, H, C, Cp, seed=C + S, scale=2.0)
    sc[..., C:] = float("nan")  # K padding of the GEMM: garbage by contract, never read
    keep = torch.ones(B, R, C, device="cuda")
    if pads == "row0":
        keep[:, 0, C // 3:C // 3 + 2] = 0
        keep[:, :, C - C // 4:] = 0
    elif pads == "others" and R > 1:
        keep[:, 1:, C // 2:] = 0
    any_pad_t = torch.tensor([any_pad], dtype=torch.int32, device="cuda")
    probs = Out(B * H * C * Cp, dt)
    attn = Out(B * Ltot * H * C * C, torch.float32)
    ops.msa_row_softmax(operand(sc).reshape(-1), operand(keep).reshape(-1), any_pad_t, probs.v, B, H, R, C, Cp,
                        nslice=S, attn_out=attn.v, layer=layer, num_layers=Ltot)
    probs.check()
    wa = torch.zeros(B, Ltot, H, C, C, dtype=torch.bool, device="cuda")
    wa[:, layer] = True
    attn.check(wa)
    pad0 = (keep[:, 0] == 0) if any_pad else None
    p, pb = G.row_softmax(sc[..., :C].permute(1, 2, 0, 3, 4), pad0)
    p, pb = p.permute(1, 0, 2, 3), pb.permute(1, 0, 2, 3)  # [B, H, C, C]
    got = probs.v.view(B, H, C, Cp)
    within(got[..., :C], p, G.store(p, pb, dt), "probs")
    assert bool((got[..., C:] == 0).all()), "probabilities of the K padding must be exactly 0"
    within(attn.v.view(B, Ltot, H, C, C)[:, layer], p, pb, "row_attentions")


# ---------------------------------------------------------------------------------------------------------------------
# row-attention context (engine_msa.hip:314-333)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,R,B", [(1, 3, 1), (65, 256, 1), (257, 7, 2), (1000, 2, 1)])
@pytest.mark.parametrize("dt", DT)
def test_row_context(ops, C, R, B, dt):
    H, E, Cp = H12, E768, ceil64(C)
    os_ = 2
    p = torch.zeros(B, H, C, Cp, dtype=dt, device="cuda")
    p[..., :C] = torch.softmax(rnd(B, H, C, C, seed=C, scale=3.0), -1).to(dt)  # zero K padding, as the softmax leaves it
    vt = torch.zeros(B, H, R, 64, Cp, dtype=dt, device="cuda")
    vt[..., :C] = rnd(B, H, R, 64, C, seed=R, dtype=dt)  # the engine clears [C, Cp)
    p, vt = operand(p), operand(vt)
    out = Out(B * R * C * E, dt)
    ops.gemm_ex(7, A=p, W=vt, out=out.v, M=C, N=R * 64, K=Cp, ldc=E, a_row_bytes=Cp * os_, w_row_bytes=Cp * os_,
                batch=B * H, batch_inner=H, a_bo=H * C * Cp * os_, a_bi=C * Cp * os_, w_bo=H * R * 64 * Cp * os_,
                w_bi=R * 64 * Cp * os_, ctx_R=R, ctx_C=C)
    out.check()
    ctx, cb = G.row_context(p[..., :C].permute(1, 0, 2, 3), vt[..., :C].permute(2, 4, 0, 1, 3))
    within(out.v, G.ctx_layout(ctx, E), G.ctx_layout(G.store(ctx, cb, dt), E), "context")


# ---------------------------------------------------------------------------------------------------------------------
# MSA q / k / v (engine_msa.hip:244-262, engine.hip: qkv_gemm_args) and the row-mapped residual (engine_msa.hip:263-275), plain and split weights
# ---------------------------------------------------------------------------------------------------------------------
def linear_args(ops, a, w32, dt, split):
    """GemmArgs fields of A / W and the reference operands: plain W, or the split_weight image with a_kt_repeat, whose
    reference repeats each 64-wide K tile of A against W_hi | W_lo, i.e. a . (W_hi + W_lo)^T over 2K products."""
    M, K = a.shape
    if not split:
        wq = operand(w32.to(dt))
        return dict(A=a, W=wq, K=K), (a, wq)
    img = operand(ops.split_weight(w32))
    a2 = a.view(M, K // 64, 1, 64).expand(M, K // 64, 2, 64).reshape(M, 2 * K)
    return dict(A=a, W=img, K=2 * K, a_row_bytes=K * 2, a_kt_repeat=1), (a2, img)


def msa_qkv(ops, x, wq, wv, bias, T, Tp, sc, dt, split, keep=None, vt_rows=0, H=H12):
    """the engine's q/k (EPI_QKV_ROPE, unit rotary tables) and v (EPI_V_T) launches on rows x [M, E]."""
    M, E = x.shape
    cos = operand(torch.ones(T, 32, device="cuda"))
    sin = operand(torch.zeros(T, 32, device="cuda"))
    q, k = Out(M * E, dt), Out(M * E, dt)
    vt = Out(M // T * E * Tp, dt)
    fq, refq = linear_args(ops, x, wq, dt, split)
    ops.gemm_ex(5, bias=bias[:2 * E], q=q.v, k=k.v, cos=cos, sin=sin, M=M, N=2 * E, T=T, H=H, E=E, Tp=Tp, scaling=sc,
                row_keep=keep, **fq)
    fv, refv = linear_args(ops, x, wv, dt, split)
    ops.gemm_ex(6, bias=bias[2 * E:], vt=vt.v, M=M, N=E, T=T, H=H, E=E, Tp=Tp, vt_rows=vt_rows, **fv)
    q.check()
    k.check()
    return q, k, vt, refq, refv


@pytest.mark.parametrize("B,R,C", [(2, 3, 1), (2, 3, 31), (1, 2, 32), (2, 3, 33), (1, 4, 65), (1, 7, 257)])
@pytest.mark.parametrize("dt", DT)
def test_msa_row_qkv(ops, B, R, C, dt, split=False):
    E, H, M = E768, H12, B * R * C
    Cp = ceil64(C)
    x = operand(rnd(M, E, seed=M, dtype=dt))
    wq, wv = rnd(2 * E, E, seed=1, scale=E ** -0.5), rnd(E, E, seed=2, scale=E ** -0.5)
    bias = operand(rnd(3 * E, seed=3, scale=0.1))
    keep = torch.ones(B, R, C, device="cuda")
    keep[:, :, C - C // 3:] = 0
    keep[0, R - 1, 0] = 0
    keep = operand(keep.reshape(-1))
    sc = (1.0 / math.sqrt(64.0)) / math.sqrt(R)
    q, k, vt, (a_q, w_q), (a_v, w_v) = msa_qkv(ops, x, wq, wv, bias, C, Cp, sc, dt, split, keep=keep, vt_rows=R)
    # fp64: rows (b, r, c); q scaled and masked, k and v plain
    yq, bq = G.dense(a_q, w_q[:E], bias[:E])
    yk, bk = G.dense(a_q, w_q[E:], bias[E:2 * E])
    yv, bv = G.dense(a_v, w_v, bias[2 * E:])
    yq, bq = G.scale(yq, bq, sc)
    kp = keep.double()[:, None]
    yq, bq = yq * kp, bq * kp

    def lay(t):
        return G.qk_layout(t.view(B * R, C, H, 64))

    within(q.v.view(B * R, H, C, 64), lay(yq), lay(G.store(yq, bq, dt)), "q")
    within(k.v.view(B * R, H, C, 64), lay(yk), lay(G.store(yk, bk, dt)), "k")
    vv, vb = yv.view(B * R, C, H, 64), G.store(yv, bv, dt).view(B * R, C, H, 64)
    written = G.vt_rows_layout(torch.ones_like(vv), B, R, Cp) != 0
    vt.check(written)
    got = vt.v.view(B, H, R, 64, Cp)
    within(got[written.view_as(got)], G.vt_rows_layout(vv, B, R, Cp)[written.view_as(got)],
           G.vt_rows_layout(vb, B, R, Cp)[written.view_as(got)], "vt rows")
    # masked q rows are exactly 0; kept rows and all of k equal a launch without row_keep, bit for bit
    q2, k2, _, _, _ = msa_qkv(ops, x, wq, wv, bias, C, Cp, sc, dt, split, keep=None, vt_rows=R)
    qm = keep.view(B * R, 1, C, 1).expand(B * R, H, C, 64) != 0
    assert bool((q.v.view(B * R, H, C, 64)[~qm] == 0).all())
    assert bits_equal(q.v.view(B * R, H, C, 64)[qm], q2.v.view(B * R, H, C, 64)[qm])
    assert bits_equal(k.v, k2.v)


@pytest.mark.parametrize("B,R,C", [(1, 1, 65), (2, 7, 33), (1, 33, 9)])
@pytest.mark.parametrize("dt", DT)
def test_msa_column_qkv(ops, B, R, C, dt, split=False):
    """column attention: sequences = MSA columns (b, c) of R rows, ESM-2 V^T layout with permuted keys, Tp = Rp."""
    E, H, M = E768, H12, B * R * C
    Rp = ceil64(R)
    x = operand(rnd(M, E, seed=M + 7, dtype=dt))
    wq, wv = rnd(2 * E, E, seed=4, scale=E ** -0.5), rnd(E, E, seed=5, scale=E ** -0.5)
    bias = operand(rnd(3 * E, seed=6, scale=0.1))
    sc = LOG2E / math.sqrt(64.0)
    q, k, vt, (a_q, w_q), (a_v, w_v) = msa_qkv(ops, x, wq, wv, bias, R, Rp, sc, dt, split)
    yq, bq = G.scale(*G.dense(a_q, w_q[:E], bias[:E]), sc)
    yk, bk = G.dense(a_q, w_q[E:], bias[E:2 * E])
    yv, bv = G.dense(a_v, w_v, bias[2 * E:])

    def lay(t):
        return G.qk_layout(t.view(B * C, R, H, 64))

    within(q.v.view(B * C, H, R, 64), lay(yq), lay(G.store(yq, bq, dt)), "q")
    within(k.v.view(B * C, H, R, 64), lay(yk), lay(G.store(yk, bk, dt)), "k")
    vv, vb = yv.view(B * C, R, H, 64), G.store(yv, bv, dt).view(B * C, R, H, 64)
    written = G.vt_esm2_layout(torch.ones_like(vv), Rp) != 0
    vt.check(written)
    got = vt.v.view(B * C, H, 64, Rp)
    within(got[written], G.vt_esm2_layout(vv, Rp)[written], G.vt_esm2_layout(vb, Rp)[written], "vt")


@pytest.mark.parametrize("B,R,C", [(2, 1, 1), (2, 1, 65), (1, 7, 65), (1, 32, 257)])
@pytest.mark.parametrize("dt", DT)
def test_row_mapped_residual(ops, B, R, C, dt, split=False):
    E, M = E768, B * R * C
    h = operand(rnd(M, E, seed=M, dtype=dt))  # out-proj input rows (b, c, r)
    wo = rnd(E, E, seed=8, scale=E ** -0.5)
    bias = operand(rnd(E, seed=9, scale=0.1))
    x0 = rnd(M, E, seed=10)  # residual stream rows (b, r, c)
    out = Out(M * E, torch.float32)
    out.v.copy_(x0.reshape(-1))
    f, (a, w) = linear_args(ops, h, wo, dt, split)
    ops.gemm_ex(4, bias=bias, out=out.v, M=M, N=E, rowmap_R=R, rowmap_C=C, **f)
    out.check()
    y, yb = G.dense(a, w, bias)
    val, bnd = G.resid_rowmap(x0, y, yb, B, R, C)
    within(out.v.view(M, E), val, bnd, "row-mapped residual")
    # a dense residual launch on the rows in GEMM order, then the row permutation: the same bits
    idx = G.rowmap_rows(B, R, C).cuda()
    d = x0[idx].contiguous()
    if split:
        ops.linear_split(h, w, bias, epilogue=4, out=d)
    else:
        ops.linear(h, w, bias, epilogue=4, out=d)
    x2 = x0.clone()
    x2[idx] = d
    assert bits_equal(out.v.view(M, E), x2)


@pytest.mark.parametrize("form", ["row_qkv", "column_qkv", "residual"])
def test_split_weights(ops, form):
    """precision mode f16x2: the MSA forms with a_kt_repeat on a split_weight image, against fp64 on W_hi + W_lo."""
    dt = torch.float16
    if form == "row_qkv":
        test_msa_row_qkv(ops, 2, 3, 33, dt, split=True)
    elif form == "column_qkv":
        test_msa_column_qkv(ops, 2, 7, 33, dt, split=True)
    else:
        test_row_mapped_residual(ops, 1, 7, 65, dt, split=True)


# ---------------------------------------------------------------------------------------------------------------------
# head_dim 128 (engine.hip:402) and rotary positions of token-packed batches (engine.hip:404)
# ---------------------------------------------------------------------------------------------------------------------
def qkv128(ops, x, w, bias, B, T, H, dt, row_pos=None, Tp=None, with_v=True):
    """q / k with the head_pad_index weight order and the 64-slot rotary table, v in natural order; head_dim 128."""
    M, E = x.shape
    Tp = Tp or ceil64(T)
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 128, 2).float() / 128))
    cos, sin = G.rope_tables(inv_freq, T)
    cos, sin = operand(cos.cuda()), operand(sin.cuda())
    wimg = torch.cat((G.weight_image(w[:E], H), G.weight_image(w[E:2 * E], H))).to(dt)
    bimg = torch.cat((G.weight_image(bias[:E, None], H)[:, 0], G.weight_image(bias[E:2 * E, None], H)[:, 0]))
    q, k = Out(M * E, dt), Out(M * E, dt)
    sc = LOG2E / math.sqrt(128.0)
    ops.gemm_ex(5, A=x, W=operand(wimg), bias=operand(bimg), q=q.v, k=k.v, cos=cos, sin=sin, M=M, N=2 * E, K=E, T=T,
                H=H, E=E, Tp=Tp, scaling=sc, head_dim=128, row_pos=row_pos)
    q.check()
    k.check()
    vt = None
    if with_v:
        vt = Out(B * E * Tp, dt)
        ops.gemm_ex(6, A=x, W=operand(w[2 * E:].to(dt)), bias=operand(bias[2 * E:].contiguous()), vt=vt.v, M=M, N=E,
                    K=E, T=T, H=H, E=E, Tp=Tp, head_dim=128)
    return q, k, vt, cos, sin, sc


def qk_ref(x, w, bias, cos, sin, pos, sc, H, dt, Bs, T):
    E = x.shape[1]
    out = []
    for i, s in ((0, sc), (1, 1.0)):
        y, b = G.dense(x, w[i * E:(i + 1) * E].to(dt), bias[i * E:(i + 1) * E])
        if s != 1.0:
            y, b = G.scale(y, b, s)
        y, b = G.rope(y.view(-1, H, 128), b.view(-1, H, 128), cos, sin, pos)
        out.append((G.qk_layout(y.view(Bs, T, H, 128)), G.qk_layout(G.store(y, b, dt).view(Bs, T, H, 128))))
    return out


@pytest.mark.parametrize("E,H,B,T", [(256, 2, 2, 1), (256, 2, 3, 31), (256, 2, 2, 32), (256, 2, 2, 33),
                                     (256, 2, 2, 1026), (5120, 40, 2, 1), (5120, 40, 2, 33)])
@pytest.mark.parametrize("dt", DT)
def test_head_dim_128(ops, E, H, B, T, dt):
    x = operand(rnd(B * T, E, seed=T + E, dtype=dt))
    w = rnd(3 * E, E, seed=11, scale=E ** -0.5)
    bias = rnd(3 * E, seed=12, scale=0.1)
    q, k, vt, cos, sin, sc = qkv128(ops, x, w, bias, B, T, H, dt)
    pos = torch.arange(T, device="cuda").repeat(B)
    (vq, bq), (vk, bk) = qk_ref(x, w, bias, cos, sin, pos, sc, H, dt, B, T)
    within(q.v.view(B, H, T, 128), vq, bq, "q")
    within(k.v.view(B, H, T, 128), vk, bk, "k")
    Tp = ceil64(T)
    yv, bv = G.dense(x, w[2 * E:].to(dt), bias[2 * E:])
    vv, vb = yv.view(B, T, H, 128), G.store(yv, bv, dt).view(B, T, H, 128)
    written = G.vt_esm2_layout(torch.ones_like(vv), Tp) != 0
    vt.check(written)
    got = vt.v.view(B, H, 128, Tp)
    within(got[written], G.vt_esm2_layout(vv, Tp)[written], G.vt_esm2_layout(vb, Tp)[written], "vt")


SEGS = [(0, 40), (40, 0), (50, 70), (130, 1), (131, 33)]  # a gap at rows [40, 50), an empty segment, restarts


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dt", DT)
def test_packed_positions(ops, hd, dt):
    rows = 164
    E, H = 256, 256 // hd
    Tp = ceil64(rows) + 64
    x = operand(rnd(rows, E, seed=hd, dtype=dt))
    w = rnd(3 * E, E, seed=13, scale=E ** -0.5)
    bias = rnd(3 * E, seed=14, scale=0.1)
    pos = torch.zeros(rows, dtype=torch.int32)
    for s0, n in SEGS:
        pos[s0:s0 + n] = torch.arange(n, dtype=torch.int32)
    pos = pos.cuda()
    if hd == 128:
        q, k, _, cos, sin, sc = qkv128(ops, x, w, bias, 1, rows, H, dt, row_pos=operand(pos), Tp=Tp, with_v=False)
        (vq, bq), (vk, bk) = qk_ref(x, w, bias, cos, sin, pos.long(), sc, H, dt, 1, rows)
    else:
        inv_freq = 1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))
        cos, sin = (operand(t.cuda()) for t in G.rope_tables(inv_freq, rows))
        sc = LOG2E / 8.0
        q, k = Out(rows * E, dt), Out(rows * E, dt)
        ops.gemm_ex(5, A=x, W=operand(w[:2 * E].to(dt)), bias=operand(bias[:2 * E]), q=q.v, k=k.v, cos=cos, sin=sin,
                    M=rows, N=2 * E, K=E, T=rows, H=H, E=E, Tp=Tp, scaling=sc, row_pos=operand(pos))
        q.check()
        k.check()
        ref = []
        for i, s in ((0, sc), (1, 1.0)):
            y, b = G.dense(x, w[i * E:(i + 1) * E].to(dt), bias[i * E:(i + 1) * E])
            if s != 1.0:
                y, b = G.scale(y, b, s)
            y, b = G.rope(y.view(rows, H, 64), b.view(rows, H, 64), cos, sin, pos.long())
            ref.append((G.qk_layout(y[None]), G.qk_layout(G.store(y, b, dt)[None])))
        (vq, bq), (vk, bk) = ref
    within(q.v.view(1, H, rows, hd), vq, bq, "packed q")
    within(k.v.view(1, H, rows, hd), vk, bk, "packed k")
    # each segment alone, padded (positions m % T): the same bits
    for s0, n in SEGS:
        if n == 0:
            continue
        xs = operand(x[s0:s0 + n].contiguous())
        if hd == 128:
            qs, ks, _, _, _, _ = qkv128(ops, xs, w, bias, 1, n, H, dt, with_v=False)
        else:
            cs, ss = (operand(t.cuda()) for t in G.rope_tables(inv_freq, n))
            qs, ks = Out(n * E, dt), Out(n * E, dt)
            ops.gemm_ex(5, A=xs, W=operand(w[:2 * E].to(dt)), bias=operand(bias[:2 * E]), q=qs.v, k=ks.v, cos=cs,
                        sin=ss, M=n, N=2 * E, K=E, T=n, H=H, E=E, Tp=ceil64(n), scaling=sc)
        torch.cuda.synchronize()
        assert bits_equal(q.v.view(H, rows, hd)[:, s0:s0 + n], qs.v.view(H, n, hd)), (s0, n)
        assert bits_equal(k.v.view(H, rows, hd)[:, s0:s0 + n], ks.v.view(H, n, hd)), (s0, n)


# ---------------------------------------------------------------------------------------------------------------------
# the generalised kernel with dense fields against the dense launch (ops.linear)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", [0, 1, 2, 4])
@pytest.mark.parametrize("dt", DT)
def test_dense_equivalence(ops, epi, dt):
    """ldc = N (explicitly) selects the generalised kernel; every output element sees the same MFMA sequence over K and
    the same epilogue as in the dense kernels, so the bits must agree.  Then a batched launch (batch 4, batch_inner 2)
    against one dense launch per entry."""
    M, N, K = 300, 320, 256
    odt = dt if epi in (0, 2) else torch.float32
    a = operand(rnd(M, K, seed=20, dtype=dt))
    w = operand(rnd(N, K, seed=21, scale=K ** -0.5, dtype=dt))
    bias = operand(rnd(N, seed=22, scale=0.1))
    x0 = rnd(M, N, seed=23)
    ldc = N + 64  # a gap of 64 elements after every row: must stay untouched
    out = Out(M * ldc, odt)
    if epi == 4:
        out.v.view(M, ldc)[:, :N].copy_(x0)
    ops.gemm_ex(epi, A=a, W=w, bias=bias, out=out.v, M=M, N=N, K=K, ldc=ldc)
    written = torch.zeros(M, ldc, dtype=torch.bool, device="cuda")
    written[:, :N] = True
    out.check(written)
    got = out.v.view(M, ldc)[:, :N]
    want = x0.clone() if epi == 4 else None
    want = ops.linear(a, w, bias, epilogue=epi, out=want)
    assert bits_equal(got, want), "generalised and dense launches differ"
    if epi in (0, 1, 4):
        y, b = G.dense(a, w, bias)
        if epi == 4:
            y, b = y + x0.double(), b + G.U * (y + x0.double()).abs()
        within(got, y, G.store(y, b, dt) if epi == 0 else b, "generalised dense")
    # batched: z = zo * 2 + zi
    Z = 4
    ab = operand(rnd(Z, M, K, seed=24, dtype=dt))
    wb = operand(rnd(Z, N, K, seed=25, scale=K ** -0.5, dtype=dt))
    x0b = rnd(Z, M, N, seed=26)
    osz = torch.tensor([], dtype=odt).element_size()
    outb = Out(Z * M * N, odt)
    if epi == 4:
        outb.v.copy_(x0b.reshape(-1))
    es = a.element_size()
    ops.gemm_ex(epi, A=ab, W=wb, bias=bias, out=outb.v, M=M, N=N, K=K, batch=Z, batch_inner=2, a_bo=2 * M * K * es,
                a_bi=M * K * es, w_bo=2 * N * K * es, w_bi=N * K * es, o_bo=2 * M * N * osz, o_bi=M * N * osz)
    outb.check()
    for z in range(Z):
        want = x0b[z].clone() if epi == 4 else None
        want = ops.linear(ab[z], wb[z], bias, epilogue=epi, out=want)
        assert bits_equal(outb.v.view(Z, M, N)[z], want), z
