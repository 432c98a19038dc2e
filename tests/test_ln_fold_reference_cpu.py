"""tests/_ln_fold_ref.py pinned without a GPU, and the METHOD of the LayerNorm fold apart from the kernels:
  * in fp64, LayerNorm(x) w^T + b = rstd ((x - c) W''^T) + b + bias2 for c = mean + delta sigma — exactly for the
    unrounded image, and for the rounded image up to delta sigma rstd rowsum(W''), with the row sums measured here
    (the figures of DESIGN.md §4.8);
  * the finalize bounds: an fp32 emulation of the documented operation order stays below HALF of either bound on every
    input the GPU tests run (producer shapes, finalize cases, a four-step chain);
  * the reference's own pieces: half_ulp against the spacing torch rounds with, the head spread against the layout of a
    head-padded model, gelu64 against torch, and that the faults the GPU tests are there to catch move the reference by
    more than its bounds."""
import math

import pytest
import torch

import _ln_fold_ref as R

DTYPES = [torch.float16, torch.bfloat16]


def ratio(err, bound):
    return (err / bound).max().item()


# ---- the method ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("E,Nn,d", [(320, 96, 16), (480, 96, 24), (1280, 128, 64)])
def test_fold_identity_in_fp64(dtype, E, Nn, d):
    g = torch.Generator().manual_seed(E)
    x = R.make_rows(16, E, seed=3).double()
    w = torch.randn(Nn, E, generator=g, dtype=torch.float64) / math.sqrt(E)
    gamma = 1 + 0.1 * torch.randn(E, generator=g, dtype=torch.float64)
    beta = 0.1 * torch.randn(E, generator=g, dtype=torch.float64)
    b = torch.randn(Nn, generator=g, dtype=torch.float64)
    ln = torch.nn.functional.layer_norm(x, (E,), gamma, beta, R.EPS) @ w.T + b
    f = R.fold_image(w, gamma, beta, dtype, d)
    mean, var, rstd = R.ln_stats(x)
    sigma = var.sqrt()
    scale = ln.abs().max().item()
    img = f["image"].double()
    rowsum = img.sum(-1)
    outs = {}
    for delta in (0.0, 0.5, -0.5, 3.0, -3.0):
        c = mean + delta * sigma
        xc = x - c[:, None]
        exact = rstd[:, None] * (xc @ f["exact"].T) + b + f["bias2"]
        assert (exact - ln).abs().max().item() <= 1e-11 * scale, delta  # the unrounded image: the identity itself
        outs[delta] = rstd[:, None] * (xc @ img.T) + b + f["bias2"]
    base = outs[0.0]
    # the rounding of the image alone (delta = 0): |x - mean| . |W'' - exact| rstd, each element within half an ulp
    assert ((base - ln).abs() <= rstd[:, None] * ((x - mean[:, None]).abs() @ R.half_ulp(f["exact"], dtype).T) + 1e-11 * scale).all()
    for delta, out in outs.items():
        resid = -(delta * sigma * rstd)[:, None] * rowsum[None, :]  # what a constant costs: it meets the rows' sums
        assert ((out - base) - resid).abs().max().item() <= 1e-11 * scale, delta
        assert ((out - base).abs() <= (abs(delta) * sigma * rstd)[:, None] * rowsum.abs()[None, :] + 1e-11 * scale).all()
    print(f"\nrowsum(W'') {dtype} E={E}: max {rowsum.abs().max().item():.2e}, rms {rowsum.pow(2).mean().sqrt().item():.2e}; "
          f"per unit of delta that is {(sigma * rstd).max().item() * rowsum.abs().max().item() / scale:.2e} of max |y|")
    # each of the E elements is off by at most half an ulp: the row sum is E half ulps at the very most
    assert (rowsum.abs() <= R.half_ulp(f["exact"], dtype).sum(-1) + 1e-12).all()


def test_head_spread_is_the_padded_head_layout():
    for d in (16, 24, 32):
        rows = [R.head_spread_index(n, d) for n in range(3 * d)]
        assert len(set(rows)) == 3 * d and max(rows) < 3 * 64
        for n, r in enumerate(rows):
            head, i = divmod(n, d)
            assert r // 64 == head
            assert r % 64 == (i if i < d // 2 else 32 + i - d // 2)
            # the rotary partner of dim i < d / 2 is dim i + d / 2: 32 slots further, as for head_dim 64
            if i < d // 2:
                assert rows[n + d // 2] == r + 32
    assert [R.head_spread_index(n, 64) for n in range(130)] == list(range(130))
    assert [R.head_spread_index(n, 16) for n in (0, 7, 8, 15, 16, 31)] == [0, 7, 32, 39, 64, 103]
    f = R.fold_image(torch.ones(48, 64), torch.ones(64), torch.ones(64), torch.float16, 24)
    assert f["rows"].tolist() == [R.head_spread_index(n, 24) for n in range(48)]


# ---- the pieces of the reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES + [torch.float32], ids=["fp16", "bf16", "fp32"])
def test_half_ulp_is_the_rounding_of_torch(dtype):
    g = torch.Generator().manual_seed(1)
    y = torch.randn(20000, generator=g, dtype=torch.float64) * torch.logspace(-9, 4, 20000, dtype=torch.float64)
    y = torch.cat([y, torch.tensor([1.0, 2.0, 0.5, 4.0, 2.0 ** -14, 2.0 ** -24, 0.0])])
    err = (y.to(dtype).double() - y).abs()
    h = R.half_ulp(y, dtype)
    assert (err <= h).all()
    assert (err / h).max().item() > 0.99  # and not a loose figure
    one = torch.tensor([1.0], dtype=torch.float64)
    assert R.half_ulp(one, dtype).item() == 2.0 ** -(R.MANT[dtype] + 1)


def test_gelu64_and_the_polynomial_bounds():
    x = torch.linspace(-12, 12, 4801, dtype=torch.float64)
    assert (R.gelu64(x) - torch.nn.functional.gelu(x)).abs().max().item() < 1e-15
    assert R.gelu64(torch.tensor([-100.0, 0.0, 100.0], dtype=torch.float64)).tolist() == [-0.0, 0.0, 100.0]
    slope = ((R.gelu64(x + 1e-6) - R.gelu64(x)) / 1e-6).abs().max().item()
    assert 1.12 < slope < R.GELU_SLOPE
    for t16, (clamp, b_in, b_out) in R.GELU_SETS.items():
        xs = torch.tensor([0.0, clamp, -clamp, clamp + 1e-3, -10.0, 100.0], dtype=torch.float64)
        assert R.gelu_poly_bound(xs, t16).tolist() == pytest.approx([b_in, b_in, b_in, b_out * (clamp + 1e-3), b_out * 10, b_out * 100])
        assert R.gelu_poly_bound(xs[1:2], t16, slack=1e-6).item() == pytest.approx(b_out * clamp)  # may be beyond the clamp


def test_producer_case_has_the_row_classes():
    a, w, bias, x0, mean_prev = R.producer_case(33, 264, 64, torch.float16, seed=5)
    out, bound = R.producer(a, w, bias, x0)
    mean, var, _ = R.ln_stats(out)
    lag = R.lag_of_rows(33)
    for m in range(33):
        c = R.row_class(m)
        sd = var[m].sqrt().item()
        if c == "constant":
            assert var[m].item() == 0.0 and out[m, 0].item() == 0.75 + m % 3  # exactly constant in fp32 too
            assert abs(mean_prev[m].item() - mean[m].item()) <= lag[m].item() * R.CONST_LAG_UNIT + 1e-6
        else:
            assert abs((mean_prev[m].double() - mean[m]).item() - lag[m].item() * sd) <= 1e-5 * (1 + abs(mean[m].item()))
        if c == "offset":
            assert 45 < mean[m].item() < 55
        if c == "channel":
            assert out[m].abs().max().item() > 250 * 3
    assert set(lag.tolist()) == set(R.LAGS)
    assert bound.min().item() > 0


# ---- the finalize bounds against the fp32 emulation of the documented order -------------------------------------------
def check_emulation(x32, mean_prev, what):
    mean_e, rstd_e = R.emulate_chain(x32, mean_prev)
    mean, var, rstd = R.ln_stats(x32)
    b_mean, b_rstd = R.finalize_bounds(x32, mean_prev)
    r_mean = ratio((mean_e.double() - mean).abs(), b_mean)
    r_rstd = ratio((rstd_e.double() - rstd).abs() / rstd, b_rstd)
    print(f"\nemulation {what}: mean {r_mean:.3f}, rstd {r_rstd:.3f} of the finalize bounds")
    assert torch.isfinite(rstd_e).all()
    assert r_mean <= 0.5 and r_rstd <= 0.5, (what, r_mean, r_rstd)
    const = var == 0
    if const.any():  # the window the GPU tests assert for exactly constant rows
        top = R.EPS ** -0.5
        assert (rstd_e[const].double() >= (1 - 1e-3) * top).all() and (rstd_e[const].double() <= (1 + 4 * 2.0 ** -23) * top).all()
    return mean_e


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("M,N,K", R.PRODUCER_SHAPES)
def test_emulation_on_the_producer_inputs(M, N, K, dtype):
    a, w, bias, x0, mean_prev = R.producer_case(M, N, K, dtype, seed=100 + M)
    out, _ = R.producer(a, w, bias, x0)
    check_emulation(out.float(), mean_prev, f"producer ({M},{N},{K})")


@pytest.mark.parametrize("rows", R.FINALIZE_ROWS)
@pytest.mark.parametrize("parts", R.FINALIZE_PARTS)
def test_emulation_on_the_finalize_inputs(rows, parts):
    x, mean_prev = R.finalize_case(rows, parts)
    check_emulation(x, mean_prev, f"finalize rows={rows} parts={parts}")
    # the fp64 finalize of the fp64 sums of the fp32 d is the fp64 statistics up to the ONE rounding of d = x - mean_prev
    # (u |d| each): an eighth of the bounds' constants
    _, _, parts64, _ = R.producer_side(x, mean_prev, torch.float16)
    mean, rstd, _, _ = R.finalize(parts64, mean_prev, x.shape[1])
    m0, _, r0 = R.ln_stats(x)
    b_mean, b_rstd = R.finalize_bounds(x, mean_prev)
    assert ratio((mean - m0).abs(), b_mean) <= 0.125 and ratio((rstd - r0).abs() / r0, b_rstd) <= 0.125


def test_emulation_on_the_chain_inputs():
    """four sub-layers: every step's error stays below half the bound of that step alone (no drift)"""
    c = R.CHAIN
    x = R.make_rows(c["M"], c["E"], seed=31)
    mean_prev = R.ln_stats(x)[0].float()  # rowstats: the mean itself
    for step in range(c["steps"]):
        a, w, bias, _, _ = R.producer_case(c["M"], c["E"], c["K"], torch.float16, seed=40 + step)
        x = R.producer(a, w, bias, x)[0].float()
        mean_prev = check_emulation(x, mean_prev, f"chain step {step}")


# ---- the faults the GPU tests are there to catch move the reference by more than its bounds ---------------------------
def test_faults_exceed_the_bounds():
    a, w, bias, x0, mean_prev = R.producer_case(129, 264, 64, torch.float16, seed=7)
    out = R.producer(a, w, bias, x0)[0].float()
    d, h16, parts, pb = R.producer_side(out, mean_prev, torch.float16)
    # the last partial slab (8 columns) dropped
    dropped = parts.clone()
    dropped[:, -1] = 0
    assert ((dropped - parts).abs() > 10 * pb)[:, -1, 1].float().mean().item() > 0.7
    # mean_prev of row m + 1
    _, h_next, parts_next, _ = R.producer_side(out, torch.roll(mean_prev, -1), torch.float16)
    assert (h_next != h16).any(-1).float().mean().item() > 0.9
    assert ((parts_next - parts).abs() > 10 * pb)[..., 0].any(-1).float().mean().item() > 0.9
    # the head spread applied with d = 64 (the identity) to a head_dim-16 image
    assert [R.head_spread_index(n, 16) for n in range(32)] != [R.head_spread_index(n, 64) for n in range(32)]
    # the other coefficient set, or a clamp moved by 0.25, beyond the clamp: 3.2e-5 |x| against 2e-6 |x| — an operand-dtype
    # polynomial in an fp32 epilogue is 16 x its bound at every |x| > 4.75, and the reverse shows in the sign of the tail
    x = torch.tensor([-6.0, 6.0], dtype=torch.float64)
    assert (R.gelu_poly_bound(x, True) > 10 * R.gelu_poly_bound(x, False)).all()
