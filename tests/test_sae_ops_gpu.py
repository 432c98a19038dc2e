"""The kernels of csrc/sae.hip one launch at a time (esmk_op_sae_rows, esmk_op_sae_topk, esmk_op_sae_segment_max,
esmk_op_sae_decode) against the numpy restatements of tests/_sae_ref.py, and the encoder product through the chain of ops.

Selection, the operand image, the segment maximum and the decode are EXACT: indices, values, counts and bits are compared for
equality.  The one inexact quantity, z = <w_enc, u> + b_enc through the f16x3 form of the dense GEMM, is held against the exact
three-term sum of the two fp16 images in fp64 with the bound of tests/test_precision_ops_gpu.py::test_f16x3_product,
(3 K + 2) u (|A3| |W3|^T + |bias|), u = 2^-24; the largest ratio is printed (`pytest -s`).

MEASURED on an MI355X: (rows, F, E) = (67, 192, 64) 0.023, (300, 4160, 320) 0.008, (260, 1024, 1280) 0.002 of the bound; z within
2.6e-7 .. 1.4e-6 of the largest |z| from the unsplit fp32 operands.

Every output buffer carries a spare row pre-filled with a sentinel that must survive the launch; z rows carry four spare
columns of +inf behind the F features that must not be read (they would be active)."""
import numpy as np
import pytest
import torch

import _sae_ref as ref
from esm_amd import _native as nat
from esm_amd import ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENT_I = 0x7BFF7BFF
CAND = None


def cand():
    global CAND
    if CAND is None:
        CAND = ops.sae_cand()
    return CAND


def sent_f32(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def sent_i32(*shape):
    return torch.full(shape, SENT_I, dtype=torch.int32, device="cuda")


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- top-k ---------------------------------------------------------------------------------------------------------------
# the places where one thread's share of a row ends (a float4: 3 | 4), one wavefront's (64 float4: 255 | 256) and one round
# of the workgroup's (256 float4: 1023 | 1024)
EDGES = (3, 4, 255, 256, 1023, 1024)
KINDS = ("sparse", "none", "fewer", "all", "cand", "cand+1", "ties_top", "ties_straddle", "all_equal", "specials", "levels")


def build_row(kind, F, k, thr, rng):
    """one row of z: actives lie in (1.5, 3) (above every threshold used), the rest is negative, zero or EQUAL to its threshold"""
    fill = rng.choice(3, size=F)
    z = np.where(fill == 0, -rng.random(F).astype(np.float32) - 0.1, np.where(fill == 1, np.float32(0.0), thr)).astype(np.float32)

    def plant(idx, vals):
        z[np.asarray(idx, dtype=np.int64)] = np.asarray(vals, dtype=np.float32)

    def some(m):
        return rng.choice(F, size=min(m, F), replace=False)

    if kind == "sparse":
        idx = some(40)
        plant(idx, 1.5 + 1.5 * rng.random(len(idx)))
    elif kind == "fewer":
        idx = some(max(k // 2, 1) if k > 1 else 0)
        plant(idx, 1.5 + 1.5 * rng.random(len(idx)))
    elif kind == "all":
        z[:] = (1.5 + 1.5 * rng.random(F)).astype(np.float32)
    elif kind in ("cand", "cand+1"):
        idx = some(cand() + (kind == "cand+1"))
        plant(idx, 1.5 + 1.5 * rng.random(len(idx)))
    elif kind == "ties_top":  # equal values inside the top k, at the share edges
        idx = some(40)
        plant(idx, 1.5 + rng.random(len(idx)))
        plant([e for e in EDGES if e < F], 2.75)
    elif kind == "ties_straddle":  # k - 1 larger values, then equal values over the k-th and (k + 1)-th place, at the share edges
        edges = [e for e in EDGES if e < F]
        rest = np.setdiff1d(np.arange(F), edges)
        plant(rng.choice(rest, size=min(k - 1, len(rest)), replace=False), 2.5 + 0.5 * rng.random(min(k - 1, len(rest))))
        plant(edges, 2.0)
    elif kind == "all_equal":
        z[:] = 1.75
    elif kind == "specials":
        idx = some(48)
        plant(idx, 1.5 + 1.5 * rng.random(len(idx)))
        plant(idx[:3], [np.inf, np.inf, np.nan])
        plant(idx[3:6], [-np.inf, np.nan, -np.inf])
    elif kind == "levels":  # every feature active, four distinct values: ties everywhere, also over the k-th place
        z[:] = (1.5 + 0.25 * rng.integers(0, 4, size=F)).astype(np.float32)
    return z


def build_z(F, n, k, thr, seed):
    rng = np.random.default_rng(seed)
    kinds = [KINDS[i % len(KINDS)] for i in range(n)] if n > 1 else ["sparse"]
    return np.stack([build_row(kind, F, k, thr, rng) for kind in kinds]), kinds


def run_topk(z, F, k, thr, k_sae=0, want_cutoff=False):
    n = z.shape[0]
    zd = torch.full((n + 1, F + 4), float("inf"), device="cuda")
    zd[:n, :F] = torch.from_numpy(z).cuda()
    idx, val, cnt = sent_i32(n + 1, k), sent_f32(n + 1, k), sent_i32(n + 1)
    thr_arg = torch.from_numpy(thr).cuda() if isinstance(thr, np.ndarray) else thr
    out = ops.sae_topk(zd, k, thr_arg, k_sae=k_sae, n=n, indices=idx, values=val, n_active=cnt, want_path=True,
                       want_cutoff=want_cutoff, F=F)
    torch.cuda.synchronize()
    assert bool((idx[n:] == SENT_I).all()) and bool(torch.isnan(val[n:]).all()) and bool((cnt[n:] == SENT_I).all()), \
        "a store behind the last row"
    return idx[:n].cpu().numpy(), val[:n].cpu().numpy(), cnt[:n].cpu().numpy(), out


@pytest.mark.parametrize("k", [1, 8, 32, 256])
@pytest.mark.parametrize("n", [1, 5, 67])
@pytest.mark.parametrize("F", [192, 4160, 8192])
def test_topk(F, n, k):
    rng = np.random.default_rng(F + n)
    thr_vec = rng.choice(np.array([0.0, 0.5, 1.0], dtype=np.float32), size=F)
    for thr in (0.0, thr_vec):
        fill_thr = thr if isinstance(thr, np.ndarray) else np.zeros(F, dtype=np.float32)
        z, kinds = build_z(F, n, k, fill_thr, seed=1000 * F + 10 * n + k)
        if isinstance(thr, np.ndarray):  # entries equal to their threshold exist and are not active (the test is >)
            assert bool(((z == thr[None, :]) & (thr[None, :] > 0)).any())
        want_idx, want_val, want_cnt = ref.topk(z, thr, k)
        idx, val, cnt, out = run_topk(z, F, k, thr)
        path = out["path"].cpu().numpy()
        assert np.array_equal(cnt, want_cnt), (kinds, cnt.tolist(), want_cnt.tolist())
        bad = np.nonzero((idx != want_idx).any(1) | (bits32(val) != bits32(want_val)).any(1))[0]
        assert bad.size == 0, [(int(i), kinds[i], int(path[i])) for i in bad[:6]]
        # the two paths are taken where the count says, and only there
        assert np.array_equal(path > 0, want_cnt > cand()), (kinds, path.tolist(), want_cnt.tolist())
        if n == 67:
            by_kind = {kind: i for i, kind in enumerate(kinds)}
            assert want_cnt[by_kind["none"]] == 0 and (idx[by_kind["none"]] == -1).all() and (val[by_kind["none"]] == 0).all()
            if k > 1:
                assert 0 < want_cnt[by_kind["fewer"]] < k and idx[by_kind["fewer"], -1] == -1
            assert want_cnt[by_kind["all"]] == F and want_cnt[by_kind["all_equal"]] == F
            assert np.array_equal(idx[by_kind["all_equal"]], np.where(np.arange(k) < F, np.arange(k), -1))  # ties go to the lower index
            if F > cand() + 1:
                assert want_cnt[by_kind["cand"]] == cand() and path[by_kind["cand"]] == 0
                assert want_cnt[by_kind["cand+1"]] == cand() + 1 and path[by_kind["cand+1"]] > 0
                assert path[by_kind["all"]] > 0 and path[by_kind["all_equal"]] > 0 and path[by_kind["levels"]] > 0
            sp = by_kind["specials"]
            assert np.isinf(val[sp, 0]) and val[sp, 0] > 0 and not np.isnan(val[sp]).any()
            if k >= 2:
                assert np.isinf(val[sp, 1]) and idx[sp, 0] < idx[sp, 1]
            # the planted tie over the k-th place: the (k + 1)-th best has the value of the k-th
            st = by_kind["ties_straddle"]
            if k < 256 and F > 256:
                more, _, _ = ref.topk(z[st:st + 1], thr, k + 1)
                assert z[st, more[0, k]] == val[st, k - 1]


def test_topk_all_8192_active_takes_the_radix_select():
    """every feature of a row of 8192 active: the radix select runs (asserted through the entry's path output), with distinct
    values (the value digits decide) and with one value everywhere (the four value digits and the two high index digits are
    the same for all 8192 keys: six passes leave them all, at least seven run)"""
    F = 8192
    rng = np.random.default_rng(5)
    z = np.stack([(1.0 + rng.random(F)).astype(np.float32), np.full(F, 2.5, dtype=np.float32)])
    for k in (1, 32, 256):
        idx, val, cnt, out = run_topk(z, F, k, 0.0)
        path = out["path"].cpu().numpy()
        want_idx, want_val, want_cnt = ref.topk(z, 0.0, k)
        assert cnt.tolist() == [F, F] and want_cnt.tolist() == [F, F]
        assert path[0] >= 1 and path[1] >= 7, path.tolist()
        assert np.array_equal(idx, want_idx) and np.array_equal(bits32(val), bits32(want_val))


@pytest.mark.parametrize("F,k_sae,k", [(192, 8, 8), (4160, 64, 32), (8192, 256, 1)])
def test_topk_of_a_topk_autoencoder(F, k_sae, k):
    """k_sae > 0: n_active = min(k_sae, count); cutoff = the key of the k_sae-th feature where a row has more actives, else 0"""
    thr = np.zeros(F, dtype=np.float32)
    z, kinds = build_z(F, 23, k_sae, thr, seed=77 + F)
    idx, val, cnt, out = run_topk(z, F, k, 0.0, k_sae=k_sae, want_cutoff=True)
    want_idx, want_val, want_cnt = ref.topk(z, 0.0, k, k_sae=k_sae)
    assert np.array_equal(cnt, want_cnt) and np.array_equal(idx, want_idx) and np.array_equal(bits32(val), bits32(want_val))
    full_idx, full_val, full_cnt = ref.topk(z, 0.0, k_sae + 1)
    cut = out["cutoff"].cpu().numpy().view(np.uint64)
    for i in range(z.shape[0]):
        if full_idx[i, k_sae] < 0:  # at most k_sae actives
            assert cut[i] == 0, (i, kinds[i])
        else:
            key = (int(bits32(full_val[i, k_sae - 1:k_sae])[0]) << 32) | (0xFFFFFFFF - int(full_idx[i, k_sae - 1]))
            assert int(cut[i]) == key, (i, kinds[i])


# ---- the operand image -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [64, 320, 480])
@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_rows_image(E, scale):
    g = torch.Generator(device="cuda").manual_seed(E)
    N = 37
    x = torch.randn(N, E, device="cuda", generator=g) * 3
    x[0, :4] = torch.tensor([0.0, -0.0, 1e-6, 60000.0])
    b_dec = torch.randn(E, device="cuda", generator=g)
    Ep = (E + 63) // 64 * 64
    lists = {"repeats": torch.tensor([5, 0, 5, 36, 36, 1, 0], dtype=torch.int32, device="cuda"), "null": None}
    for name, rows in lists.items():
        for bd in (b_dec, None):
            n = N if rows is None else rows.numel()
            out = torch.full((n + 1, 3 * Ep + 8), 0x7BFF, dtype=torch.int16, device="cuda").view(torch.float16)
            ops.sae_rows(x, rows, bd, scale, out=out, n=n)
            got = out.view(torch.int16).cpu().numpy()
            assert (got[n:] == 0x7BFF).all() and (got[:n, 3 * Ep:] == 0x7BFF).all(), "a store outside the image"
            u = ref.u_rows(x.cpu().numpy(), None if rows is None else rows.cpu().numpy(), None if bd is None else bd.cpu().numpy(), scale)
            want = ref.image_rows(u).view(np.int16)
            assert np.array_equal(got[:n, :3 * Ep], want), (name, bd is not None, np.argwhere(got[:n, :3 * Ep] != want)[:4].tolist())
            if Ep > E:  # the pad columns are zero in all three slots
                t = got[:n, :3 * Ep].reshape(n, Ep // 64, 3, 64)
                assert (t[:, -1, :, E - Ep:] == 0).all()
            lo = got[:n, :3 * Ep].reshape(n, Ep // 64, 3, 64)[:, :, 2]
            assert (lo != 0).any()


def test_rows_image_clamps_the_row_list():
    """A listed row is device data: -3 gives the image of row 0, N + 5 that of row N - 1."""
    N, E = 9, 320
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(N, E, device="cuda", generator=g) * 3
    b_dec = torch.randn(E, device="cuda", generator=g)
    rows = torch.tensor([-3, N + 5, 4], dtype=torch.int32, device="cuda")
    got = ops.sae_rows(x, rows, b_dec, 0.37).view(torch.int16).cpu().numpy()
    want = ref.image_rows(ref.u_rows(x.cpu().numpy()[[0, N - 1, 4]], None, b_dec.cpu().numpy(), 0.37)).view(np.int16)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()


# ---- the encoder product through the chain of ops --------------------------------------------------------------------------
@pytest.mark.parametrize("rows,F,E", [(67, 192, 64), (300, 4160, 320), (260, 1024, 1280)])
def test_encoder_product(rows, F, E):
    g = torch.Generator(device="cuda").manual_seed(rows)
    x = torch.randn(rows, E, device="cuda", generator=g)
    b_dec = 0.1 * torch.randn(E, device="cuda", generator=g)
    w = torch.randn(F, E, device="cuda", generator=g) / E ** 0.5
    b_enc = torch.randn(F, device="cuda", generator=g)
    a3 = ops.sae_rows(x, None, b_dec, 0.37)
    w3 = torch.zeros((F, 3 * E), dtype=torch.float16, device="cuda")
    ops.split_weight_ex(w, w3, E, 3)
    z = sent_f32(rows + 1, F)
    ops.linear(a3, w3, b_enc, nat.EPI_STORE_F32, out=z[:rows])
    assert bool(torch.isnan(z[rows:]).all()) and not bool(torch.isnan(z[:rows]).any())
    # the images themselves are the restated ones
    assert np.array_equal(a3.cpu().numpy().view(np.int16),
                          ref.image_rows(ref.u_rows(x.cpu().numpy(), None, b_dec.cpu().numpy(), 0.37)).view(np.int16))
    assert np.array_equal(w3.cpu().numpy().view(np.int16), ref.weight_image(w.cpu().numpy()).view(np.int16))
    a3d, w3d = a3.double(), w3.double()
    three = a3d @ w3d.t() + b_enc.double()
    bound = (3 * E + 2) * U * (a3d.abs() @ w3d.abs().t() + b_enc.double().abs())
    r = ((z[:rows].double() - three).abs() / bound).max().item()
    full = torch.from_numpy(ref.z64(x.cpu().numpy(), w.cpu().numpy(), b_enc.cpu().numpy(), b_dec.cpu().numpy(), 0.37)).cuda()
    e3 = (z[:rows].double() - full).abs().max().item() / full.abs().max().item()
    print(f"\nsae encoder product ({rows},{F},{E}): {r:.3f} of the accumulation bound; {e3:.2e} of the largest |z| from the "
          f"unsplit fp32 operands")
    assert r <= 1.0, r


# ---- the per-sequence maximum ----------------------------------------------------------------------------------------------
def segment_case(F, seed, k_sae=0):
    rng = np.random.default_rng(seed)
    lens = [1, 7, 40]
    rows = np.array([(b, 1 + t) for b, n in enumerate(lens) for t in range(n)], dtype=np.int32)
    n = len(rows)
    z = np.where(rng.random((n, F)) < 0.3, 1.0 + rng.integers(0, 6, size=(n, F)) * 0.25, -1.0).astype(np.float32)  # few levels: ties
    z[:, 5] = -0.5           # a feature that is never active
    z[:, 6] = 0.75           # equal to its threshold below: never active
    z[8:, 7] = 2.0           # the same value at every position of the last sequence: the lowest position wins
    z[3, 9], z[5, 9] = np.inf, np.inf
    z[4, 10] = np.nan
    thr = np.zeros(F, dtype=np.float32)
    thr[6] = 0.75
    seg_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return z, thr, rows, seg_start


@pytest.mark.parametrize("F,k_sae", [(192, 0), (1088, 0), (192, 16)])
def test_segment_max(F, k_sae):
    z, thr, rows, seg_start = segment_case(F, 3 + F, k_sae)
    n, B = len(rows), 3
    want_max, want_arg = ref.segment_max(z, thr, rows, B, k_sae=k_sae)
    assert want_arg[2, 7] == 1 and (want_arg[:, 5] == -1).all() and (want_arg[:, 6] == -1).all() and want_arg[1, 9] == 3
    zd, thr_d = torch.from_numpy(z).cuda(), torch.from_numpy(thr).cuda()
    rows_d, seg_d = torch.from_numpy(rows).cuda(), torch.from_numpy(seg_start).cuda()
    cut = ops.sae_topk(zd, min(k_sae, 8), thr_d, k_sae=k_sae, want_cutoff=True)["cutoff"] if k_sae else None
    for split in (None, 4, 20):  # one launch; two launches that split the middle sequence; ... that split the last
        pmax = torch.zeros((B + 1, F), device="cuda")
        parg = torch.full((B + 1, F), -1, dtype=torch.int32, device="cuda")
        pmax[B], parg[B] = float("nan"), SENT_I
        parts = [(0, n)] if split is None else [(0, split), (split, n - split)]
        for lo, c in parts:
            ops.sae_segment_max(zd[lo:lo + c], rows_d[lo:lo + c], seg_d, pmax[:B], parg[:B], thr_d,
                                cutoff=None if cut is None else cut[lo:lo + c], row0=lo, n=c)
        assert bool(torch.isnan(pmax[B]).all()) and bool((parg[B] == SENT_I).all())
        assert np.array_equal(bits32(pmax[:B].cpu().numpy()), bits32(want_max)), split
        assert np.array_equal(parg[:B].cpu().numpy(), want_arg), split


# ---- decode ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [64, 1280])
@pytest.mark.parametrize("k", [1, 64])
@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_decode(E, k, scale):
    rng = np.random.default_rng(E + k)
    n, F = 9, 300
    w_dec = rng.standard_normal((F, E)).astype(np.float32)
    b_dec = rng.standard_normal(E).astype(np.float32)
    idx = rng.integers(0, F, size=(n, k)).astype(np.int32)
    val = (rng.random((n, k)) * 3).astype(np.float32)
    idx[1, :] = -1                      # an empty row: the bias alone
    idx[2, k // 2:] = -1                # unused slots behind the used ones
    idx[3, 0] = -1                      # and in front
    val[idx < 0] = 0
    for bd in (b_dec, None):
        out = sent_f32(n + 1, E)
        ops.sae_decode(torch.from_numpy(idx).cuda(), torch.from_numpy(val).cuda(), torch.from_numpy(w_dec).cuda(),
                       None if bd is None else torch.from_numpy(bd).cuda(), float(np.float32(1.0 / scale)), out=out[:n])
        assert bool(torch.isnan(out[n:]).all())
        want = ref.decode(idx, val, w_dec, bd, scale)
        assert np.array_equal(bits32(out[:n].cpu().numpy()), bits32(want)), (bd is not None)
