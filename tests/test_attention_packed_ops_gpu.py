"""The packed attention core and the packed map kernel, one kernel at a time, against a plain fp64 softmax.

esmk_op_attention_packed / esmk_op_attention_probs_packed reach the token-packed forms of csrc/attention.hip and
csrc/attention128.hip (segments of one row space, a work list of 128-query blocks, ragged [L, H, len, len] maps) without
a model around them.  Whole-model tests pin these forms by bit-equality between layouts only, which cannot catch an error
every layout shares; here each segment is compared with test_attention_variants_gpu.py's reference

    s = q k^T + key_bias;  p = softmax(s);  o = p v;  lse = logsumexp(s)

in fp64 on the kernels' own operand values, with that file's tolerances (ctx 4 eps, lse 1e-3, maps 2e-3 max p + 1e-6 plus
the output dtype's epsilon for low-precision maps), AND bit for bit with esmk_op_attention_ex /
esmk_op_attention_probs_ex on the segment alone.  Segment lengths sit on and next to the 32 / 64 / 128-row edges; the
segments start at multiples of 16 with gaps of different sizes, the first one not at row 0."""
import pytest
import torch

import test_attention_variants_gpu as V

pytestmark = pytest.mark.gpu
NEG = float("-inf")

# (length, kind): plain | trail = the last 20 tokens are <pad> | inner = <pad> inside, a whole 64-key tile among them |
# allpad = padding only
SEGMENTS = [(1, "plain"), (2, "plain"), (31, "plain"), (32, "plain"), (33, "plain"), (63, "plain"), (64, "plain"),
            (65, "plain"), (100, "trail"), (127, "plain"), (128, "plain"), (40, "allpad"), (129, "plain"),
            (200, "inner"), (300, "plain")]
GAPS = [0, 16, 0, 32, 0, 0, 48, 0, 16, 0, 0, 16, 0, 64, 0]


@pytest.fixture(scope="module")
def ops():
    from esm_amd import ops as _ops

    return _ops


def _layout():
    segs, row = [], 16
    for (n, _), gap in zip(SEGMENTS, GAPS):
        segs.append((row, n))
        row += (n + 15) // 16 * 16 + gap
    rows = (row + 127) // 128 * 128
    return segs, rows


def _key_bias(segs, rows):
    bias = torch.full((rows,), NEG, device="cuda")   # gap rows are padding, as esmk_forward_packed marks them
    for (start, n), (_, kind) in zip(segs, SEGMENTS):
        bias[start:start + n] = 0
        if kind == "trail":
            bias[start + n - 20:start + n] = NEG
        elif kind == "inner":
            bias[start + 3] = bias[start + 17] = NEG
            bias[start + 64:start + 128] = NEG
            bias[start + n - 2] = NEG
        elif kind == "allpad":
            bias[start:start + n] = NEG
    return bias


@pytest.mark.parametrize("D,dt,scale,lowp", [
    (64, torch.float16, 4.0, False), (64, torch.bfloat16, 0.6, True), (64, torch.float16, 0.6, True),
    (64, torch.bfloat16, 4.0, False), (128, torch.float16, 0.6, False), (128, torch.bfloat16, 4.0, True),
    (128, torch.float16, 4.0, True), (128, torch.bfloat16, 0.6, False)])
def test_packed_ops_against_fp64_and_each_segment_alone(ops, D, dt, scale, lowp):
    H, L, layer = 3, 2, 1
    segs, rows = _layout()
    qk, q, k, v = V._inputs(ops, 1, H, rows, D, dt, scale, seed=rows + D + int(scale * 10))
    if scale >= 4.0:
        assert (q[0].double() @ k[0].double().transpose(-1, -2)).abs().max().item() > 60   # raw scores towards +-100
    bias = _key_bias(segs, rows)
    vt = ops.make_vt_packed(v[0])
    ctx, lse = ops.attention_packed(qk[0], k[0], vt, segs, bias, want_lse=True)
    out_dtype = dt if lowp else torch.float32
    flat, views = ops.attention_probs_packed(qk[0], k[0], lse, segs, bias, layer=layer, num_layers=L, out_dtype=out_dtype)
    assert ctx.shape == (rows, H * D) and lse.shape == (H, rows)
    assert torch.isfinite(ctx).all() and torch.isfinite(lse).all() and torch.isfinite(flat).all()
    assert len(views) == len(segs) and flat.numel() == L * H * sum(n * n for _, n in segs)
    in_seg = torch.zeros(rows, dtype=torch.bool, device="cuda")
    for i, ((start, n), (_, kind)) in enumerate(zip(segs, SEGMENTS)):
        sl = slice(start, start + n)
        in_seg[sl] = True
        qs, qe, ks, vs = (t[:, :, sl].contiguous() for t in (qk, q, k, v))
        b = None if kind == "plain" else bias[sl][None].contiguous()
        got_p = views[i]
        assert got_p.shape == (L, H, n, n)
        assert (got_p[0] == 0).all()                                   # only slice `layer` is written
        # ---- fp64 reference on the operand values ---------------------------------------------------------------
        p_ref, o_ref, lse_ref = V._ref(qe, ks, vs, b)
        if kind == "allpad":
            # no key to attend to: finite (zero) context and lse, an all-zero map, never NaN
            assert (ctx[sl] == 0).all() and (lse[:, sl] == 0).all() and (got_p == 0).all()
        else:
            real = torch.ones(1, n, dtype=torch.bool, device="cuda") if b is None else ~torch.isinf(b)
            V._check_ctx(ctx[sl], o_ref, dt, rows=real.reshape(-1))
            V._check_lse(lse[None, :, sl], lse_ref, mask=real[:, None, :].expand(1, H, n))
            keep = real.double()
            p_ref = torch.nan_to_num(p_ref) * keep[:, None, :, None] * keep[:, None, None, :]
            V._check_probs(got_p[layer][None], p_ref, out_dtype)
            assert (got_p[layer][None][p_ref == 0] == 0).all()         # <pad> rows and columns: exact zeros
            # rows of every real query sum to 1: the map tolerance with the row's sum (1) in the place of max p; the
            # roundings of a low-precision map add at most eps * sum p = eps
            sums = got_p[layer].double().sum(-1)[:, real[0]]
            tol = 2e-3 + 1e-6 + (V._eps(out_dtype) if out_dtype != torch.float32 else 0.0)
            assert (sums - 1).abs().max().item() <= tol, (n, kind, (sums - 1).abs().max().item())
        # ---- bit for bit: the segment alone through esmk_op_attention_ex / esmk_op_attention_probs_ex -----------
        # interior pads and padding only: the padded form the engine launches (with seq_info); trailing pads: without
        # seq_info — with it the padded kernel ends the key loop at the last real token and mirrors the pad query rows,
        # a case the engine never packs (a segment ends at its last real token)
        info = V._seq_info(b) if kind in ("inner", "allpad") else None
        a_ctx, a_lse = ops.attention(qs, ks, ops.make_vt(vs), b, want_lse=True, seq_info=info)
        assert torch.equal(ctx[sl], a_ctx), (n, kind)
        assert torch.equal(lse[:, sl], a_lse[0]), (n, kind)
        a_p = ops.attention_probs(qs, ks, a_lse, b, layer=layer, num_layers=L, out_dtype=out_dtype)
        assert torch.equal(got_p[layer], a_p[0, layer]), (n, kind)
    assert (ctx[~in_seg] == 0).all()                                   # gap rows are not written


def test_packed_ops_without_key_bias_and_order_of_work(ops):
    """key_bias NULL: no segment has pads.  Long segments behind short ones: the work list is sorted by length, the
    output layout follows the table order."""
    D, dt, H = 64, torch.float16, 2
    segs = [(0, 5), (16, 300), (320, 64), (384, 129)]
    rows = 640
    qk, q, k, v = V._inputs(ops, 1, H, rows, D, dt, 0.6, seed=4)
    ctx, lse = ops.attention_packed(qk[0], k[0], ops.make_vt_packed(v[0]), segs, None, want_lse=True)
    flat, views = ops.attention_probs_packed(qk[0], k[0], lse, segs)
    for (start, n), got in zip(segs, views):
        sl = slice(start, start + n)
        qs, ks, vs = (t[:, :, sl].contiguous() for t in (qk, k, v))
        a_ctx, a_lse = ops.attention(qs, ks, ops.make_vt(vs), want_lse=True)
        assert torch.equal(ctx[sl], a_ctx) and torch.equal(lse[:, sl], a_lse[0])
        assert torch.equal(got[0], ops.attention_probs(qs, ks, a_lse)[0, 0])
