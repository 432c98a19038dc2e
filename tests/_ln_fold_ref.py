"""fp64 reference of the LayerNorm fold (reference esm/modules.py:120-140: LayerNorm -> Linear) and of the
GELU of the GEMM epilogues (esm/modules.py:17-24), with the a-priori error bounds the GPU tests assert
(tests/test_ln_fold_ops_gpu.py, tests/test_gelu_epilogue_gpu.py) and the inputs those tests run on.  Plain torch on the
CPU or the GPU (every function follows the device of its arguments); tests/test_ln_fold_reference_cpu.py pins the module
without a GPU.

Bounds, u = 2^-24 (fp32 unit roundoff).  None of them is tuned against a kernel.
  * dot products: a K-term fp32 sum of exact products plus a bias and a residual is within (K + 2) u (|a| |w|^T + |bias| +
    |x0|) of the exact value (K - 1 additions of the sum, one of the bias, one of the residual: each at most u of a partial
    sum that the magnitudes bound);
  * partial sums of a 128-column slab (128 values d, fixed order): |S1 - sum d| <= 128 u sum |d| (127 additions),
    |S2 - sum d^2| <= 129 u sum d^2 (128 fused multiply-adds and the rounding of the tree);
  * a store in the operand dtype: half an ulp at the element (``half_ulp``);
  * LayerNorm statistics of the two-pass kernel (rowstats_kernel): the row sum is a chain of E / 64 additions per lane and
    a 6-level butterfly, the division and the subtraction x - mean add one rounding each, the same again for the squares:
    (E / 64 + 8) u relative to mean |x| for the mean, and to the variance (plus the square of the mean's error) for rstd;
  * finalize (producer partial sums -> ln_finalize_kernel), against the fp64 statistics of the fp32 rows:
        |d rstd| / rstd <= 4 * 2^-23 (dm^2 + var) / (var + 1e-5) + 4 * 2^-23
        |d mean|        <= 8 * 2^-23 (|mean| + mean |d|),              dm = mean of d = x - mean_prev
    var = S2 / E - dm^2 cancels dm^2 + var against dm^2, hence the first form; the mean adds dm to mean_prev.  These two
    carry constants that are not derived: ``emulate_chain`` replays the documented order of the kernels in fp32 (16 values
    per lane in four quads, an 8-lane row_shr tree, slabs added in order, var = S2 / E - dm^2 unfused) and the CPU suite
    requires the emulation to stay below HALF of either bound on every input the GPU tests use.
  * GELU polynomial (esm_amd/csrc/common.h gelu_fast; the figures tests/test_host_cpu.py asserts for the coefficient
    sets): fp32 set 2e-6 inside the clamp (4.75) and 2e-6 |x| beyond; operand-dtype set 8e-6 inside (4) and 3.2e-5 |x|
    beyond, never positive on the left tail.
"""
import math

import torch

U = 2.0 ** -24
EPS = 1e-5
MANT = {torch.float16: 10, torch.bfloat16: 7, torch.float32: 23}
EMIN = {torch.float16: -14, torch.bfloat16: -126, torch.float32: -126}
DT_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
GELU_SLOPE = 1.13  # max |gelu'|
GELU_SETS = {False: (4.75, 2e-6, 2e-6), True: (4.0, 8e-6, 3.2e-5)}  # T16: clamp, absolute inside, relative beyond
LAGS = (0.0, 0.01, 1.0, 10.0)  # mean_prev = true mean + lag * sigma_row
CONST_LAG_UNIT = 0.01  # a constant row has no spread: its lag is LAGS * 0.01 in absolute units (<= 0.1)
ROW_CLASSES = ("plain", "offset", "constant", "channel")


def gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def half_ulp(y, dtype):
    """half the spacing of `dtype` at |y| (fp64 tensor), the subnormal spacing below the normal range"""
    e = torch.frexp(y.abs().double().clamp_min(2.0 ** -1000))[1] - 1  # floor(log2 |y|)
    e = e.clamp_min(EMIN[dtype])
    return torch.ldexp(torch.ones_like(y, dtype=torch.float64), e - MANT[dtype] - 1)


def gelu_poly_bound(x, t16, slack=0.0):
    """|gelu_fast<t16>(x) - gelu(x)| at the fp64 pre-activation x (known to within `slack`)"""
    clamp, b_in, b_out = GELU_SETS[bool(t16)]
    ax = x.abs()
    inside = torch.full_like(ax, b_in)
    return torch.where(ax + slack <= clamp, inside, torch.maximum(inside, b_out * (ax + slack)))


# ---- inputs -----------------------------------------------------------------------------------------------------------
def make_rows(rows, E, seed, classes=ROW_CLASSES):
    """fp32 [rows, E] on the CPU, row m of class classes[m % len]: plain (randn * 3 + 0.7), offset (+ 50), constant (every
    element 0.75 + m % 3 exactly), channel (one channel 300 x the spread)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, E, generator=g, dtype=torch.float64) * 3 + 0.7
    for m in range(rows):
        c = classes[m % len(classes)]
        if c == "offset":
            x[m] += 50.0
        elif c == "constant":
            x[m] = 0.75 + m % 3
        elif c == "channel":
            x[m, (7 * m + 3) % E] = 900.0
    return x.float()


def row_class(m, classes=ROW_CLASSES):
    return classes[m % len(classes)]


def lag_of_rows(rows):
    """row m lags by LAGS[(m // 4) % 4]: every (class, lag) pair occurs from 16 rows on; rows 0 - 3 have no lag"""
    return torch.tensor([LAGS[(m // len(ROW_CLASSES)) % len(LAGS)] for m in range(rows)], dtype=torch.float64)


def lagged_mean(x):
    """mean_prev fp32 [rows] for the fp32 / fp64 rows x: the fp64 mean + lag * sigma_row (constant rows: lag * 0.01)"""
    x = x.double()
    sd = x.var(-1, unbiased=False).sqrt()
    unit = torch.where(sd > 0, sd, torch.full_like(sd, CONST_LAG_UNIT))
    return (x.mean(-1) + lag_of_rows(x.shape[0]).to(x.device) * unit).float()


def producer_case(M, N, K, dtype, seed):
    """a [M,K], w [N,K] (dtype), bias fp32 [N], x0 fp32 [M,N] such that out = x0 + a w^T + bias has rows of make_rows' classes
    (constant rows exactly: a row of zeros in a, bias a multiple of 2^-8), and mean_prev fp32 [M].  All on the CPU."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dtype)
    bias = (torch.randn(N, generator=g) * 256).round() / 256
    for m in range(M):
        if row_class(m) == "constant":
            a[m] = 0
    target = make_rows(M, N, seed + 1).double()
    x0 = (target - (a.double() @ w.double().T + bias.double())).float()
    out = x0.double() + a.double() @ w.double().T + bias.double()
    return a, w, bias, x0, lagged_mean(out)


# ---- statistics -------------------------------------------------------------------------------------------------------
def ln_stats(x):
    """mean, biased variance, rstd = (var + 1e-5)^-1/2 of the rows, fp64 (ESM1bLayerNorm, modules.py:68-81)"""
    x = x.double()
    mean = x.mean(-1)
    var = x.var(-1, unbiased=False)
    return mean, var, (var + EPS).rsqrt()


def rowstats_bounds(x):
    """(|d mean|, |d rstd| / rstd) of the two-pass kernel on the fp32 rows x"""
    x = x.double()
    E = x.shape[-1]
    mean, var, _ = ln_stats(x)
    c = (E / 64 + 8) * U
    dmean = c * x.abs().mean(-1)
    # mean((x - mean')^2) = var + dmean^2 exactly; x - mean' and the squares are rounded (4 u), the sum as above (c);
    # d rstd / rstd = d var / (2 (var + eps)), and eps, the root and the division add a rounding each
    dvar = (c + 4 * U) * (var + dmean ** 2) + dmean ** 2
    return dmean, dvar / (2 * (var + EPS)) + 4 * U


# ---- load time --------------------------------------------------------------------------------------------------------
def head_spread_index(n, d):
    """esm_amd/csrc/elementwise.hip head_pad_index, d < 64: row head * d + i -> head * 64 + (i if i < d / 2 else 32 + i - d / 2)"""
    if d == 64:
        return n
    head, i = divmod(n, d)
    return head * 64 + (i if i < d // 2 else 32 + i - d // 2)


def fold_image(w, gamma, beta, dtype, head_dim=64):
    """W'' = T(w gamma - rowmean(w gamma)), bias2 = w . beta of the rows of w, spread to head * 64 + slot for head_dim < 64.
    Returns a dict: rows (destination row of every source row), exact (fp64, unrounded), image (rounded to dtype),
    image_bound, bias2, bias2_bound — all indexed by SOURCE row."""
    w, gamma, beta = w.double(), gamma.double(), beta.double()
    Nn, K = w.shape
    wg = w * gamma
    exact = wg - wg.mean(-1, keepdim=True)
    mean_err = K * U * wg.abs().mean(-1, keepdim=True)  # the fp32 row mean
    rows = torch.tensor([head_spread_index(n, head_dim) for n in range(Nn)], device=w.device)
    return dict(rows=rows, exact=exact, image=exact.to(dtype), image_bound=half_ulp(exact.abs() + mean_err, dtype) + mean_err,
                bias2=w @ beta, bias2_bound=(K + 2) * U * (w.abs() @ beta.abs()))


# ---- producer / finalize / consumer -------------------------------------------------------------------------------------
def dot_bound(a, w, *adds):
    """(K + 2) u (|a| |w|^T + sum |adds|)"""
    a, w = a.double(), w.double()
    mag = a.abs() @ w.abs().T
    for t in adds:
        if t is not None:
            mag = mag + t.double().abs()
    return (a.shape[-1] + 2) * U * mag


def producer(a, w, bias, x0):
    """out = x0 + a w^T + bias in fp64, and its bound"""
    out = x0.double() + a.double() @ w.double().T + (0 if bias is None else bias.double())
    return out, dot_bound(a, w, bias, x0)


def producer_side(out32, mean_prev, dtype):
    """What the producer derives from ITS fp32 rows out32 [M,N]: d = fl32(out - mean_prev), h16 = T(d), and per 128-column
    slab (sum d, sum d^2) in fp64 with their bounds.  Returns (d fp32, h16, parts fp64 [M,P,2], bounds fp64 [M,P,2])."""
    d = out32.float() - mean_prev.float()[:, None]
    M, N = d.shape
    P = (N + 127) // 128
    dd = torch.nn.functional.pad(d.double(), (0, P * 128 - N)).view(M, P, 128)
    parts = torch.stack([dd.sum(-1), (dd * dd).sum(-1)], -1)
    bounds = torch.stack([128 * U * dd.abs().sum(-1), 129 * U * (dd * dd).sum(-1)], -1)
    return d, d.to(dtype), parts, bounds


def finalize(parts, mean_prev, E):
    """ln_finalize in fp64: parts [M,P,2] -> (mean_new, rstd, dm, var)"""
    s = parts.double().sum(1)
    dm = s[:, 0] / E
    var = (s[:, 1] / E - dm * dm).clamp_min(0)
    return mean_prev.double() + dm, (var + EPS).rsqrt(), dm, var


def finalize_bounds(x, mean_prev):
    """(|d mean|, |d rstd| / rstd) of partial sums + finalize against the fp64 statistics of the fp32 rows x"""
    x = x.double()
    d = x - mean_prev.double()[:, None]
    mean, var, _ = ln_stats(x)
    dm = d.mean(-1)
    return 8 * 2.0 ** -23 * (mean.abs() + d.abs().mean(-1)), 4 * 2.0 ** -23 * (dm * dm + var) / (var + EPS) + 4 * 2.0 ** -23


def consumer(a, w, bias, bias2, rstd):
    """pre = rstd (a w^T) + bias + bias2 in fp64 on the rounded operands, and its bound (the fma and the bias sum are two
    of the K + 2 roundings)"""
    a, w = a.double(), w.double()
    r = rstd.double()[:, None]
    b = (0 if bias is None else bias.double()) + (0 if bias2 is None else bias2.double())
    babs = (0 if bias is None else bias.double().abs()) + (0 if bias2 is None else bias2.double().abs())
    pre = r * (a @ w.T) + b
    return pre, (a.shape[-1] + 2) * U * (r * (a.abs() @ w.abs().T) + babs)


def gelu_out_bound(pre, pre_bound, dtype, t16=True):
    """|T(gelu_fast(pre')) - gelu64(pre)| for |pre' - pre| <= pre_bound"""
    val = gelu64(pre)
    b = GELU_SLOPE * pre_bound + gelu_poly_bound(pre, t16, pre_bound)
    return val, b + half_ulp(val.abs() + b, dtype)


# ---- fp32 emulation of the documented order (CPU suite) ---------------------------------------------------------------
def _f32(t):
    return t.to(torch.float32)


def emulate_partials(d):
    """The producer's (S1, S2) of every 128-column slab in fp32, in the order esm_amd/csrc/gemm9.hip documents: lane c of a
    row's eight takes columns 32 jb + 4 c .. + 3 of the slab for jb = 0..3, S1 += (d0 + d1) + (d2 + d3), S2 = four fused
    multiply-adds; then lane l adds lane l-1, then l-2, then l-4 (row_shr) and lane 7 holds the sum.  d fp32 [M,N]."""
    M, N = d.shape
    P = (N + 127) // 128
    q = torch.nn.functional.pad(_f32(d), (0, P * 128 - N)).view(M, P, 4, 8, 4)  # [row, slab, jb, lane, e]
    s1 = torch.zeros(M, P, 8)
    s2 = torch.zeros(M, P, 8)
    for jb in range(4):
        v = q[:, :, jb]
        s1 = s1 + ((v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3]))
        for e in range(4):  # fma: one rounding of the exact d * d + s (fp64 holds the 48-bit product; double rounding aside)
            s2 = _f32(v[..., e].double() * v[..., e].double() + s2.double())
    for s in (1, 2, 4):
        for t in (s1, s2):
            t[..., s:] = t[..., s:] + t[..., :-s].clone()
    return torch.stack([s1[..., 7], s2[..., 7]], -1)


def emulate_finalize(parts32, mean_prev, E):
    """ln_finalize_kernel in fp32: slabs in order, dm = S1 / E, var = max(S2 / E - dm dm, 0), mean += dm, rstd = 1 / sqrt"""
    s1 = torch.zeros(parts32.shape[0])
    s2 = torch.zeros(parts32.shape[0])
    for k in range(parts32.shape[1]):
        s1 = s1 + parts32[:, k, 0]
        s2 = s2 + parts32[:, k, 1]
    inv_e = torch.tensor(1.0 / E, dtype=torch.float32)
    dm = s1 * inv_e
    var = (s2 * inv_e - dm * dm).clamp_min(0)
    return _f32(mean_prev) + dm, 1.0 / torch.sqrt(var + torch.tensor(EPS, dtype=torch.float32))


def emulate_chain(x, mean_prev):
    """fp32 rows x, fp32 mean_prev -> (mean, rstd) as the producer + finalize compute them"""
    d = _f32(x) - _f32(mean_prev)[:, None]
    return emulate_finalize(emulate_partials(d), mean_prev, x.shape[1])


# ---- the cases of the GPU tests (the CPU suite runs the emulation on the same rows) ---------------------------------
ROWSTATS_ROWS = (1, 9)
ROWSTATS_E = (4, 320, 516, 1280, 1284, 2560, 5120)
PRODUCER_SHAPES = ((1, 128, 64), (7, 264, 192), (129, 480, 320), (257, 1280, 64), (384, 512, 128))
CONSUMER_SHAPES = ((1, 8, 64), (7, 264, 192), (129, 520, 320), (257, 1280, 64))
FINALIZE_PARTS = (1, 3, 10)
FINALIZE_ROWS = (1, 300)
CHAIN = dict(M=130, E=480, K=64, steps=4)


def finalize_case(rows, parts, seed=21):
    """rows of E = 128 parts columns (the last slab 8 columns short when parts > 1) and their lagged mean_prev"""
    E = 128 * parts - (8 if parts > 1 else 0)
    x = make_rows(rows, E, seed + parts)
    return x, lagged_mean(x)
