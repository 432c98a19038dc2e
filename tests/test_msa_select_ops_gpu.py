"""The five MSA row-selection entries (csrc/msa_select.hip), one op at a time, against the numpy references of
tests/_msa_select_ref.py.  Everything but the race keys is integer arithmetic or comparison logic and must be exact; the keys
are one fp64 logarithm and one product and must lie within 4 fp64 ulp of numpy's.

Shapes: N in {1, 2, 63, 64, 65, 257} (below, at and past the 64-row tile, several row tiles) crossed with L in {1, 3, 4, 5, 63,
64, 65, 255, 1021} (below a dword, dword tails, below / at / past the 128-column LDS chunk, eight chunks with a tail), the row
stride equal to L, L + 3 (rows not dword aligned: the byte path) and a multiple of 4 past L (the dword path with garbage behind
L), plus a dword-strided matrix at an odd address.  One 2049 x 130 alignment runs 33 row tiles with a remainder, the column
tiles dealt to several workgroups."""
import numpy as np
import pytest
import torch

import _msa_select_ref as M
from esm_amd import ops

pytestmark = pytest.mark.gpu

NS = (1, 2, 63, 64, 65, 257)
LS = (1, 3, 4, 5, 63, 64, 65, 255, 1021)
SEEDS = (0, 1, 2, 12345)


def byte_msa(n, L, seed):
    """Rows over ALL byte values: three random ancestors, every row a copy mutated at its own rate (0 .. 0.4); half of the
    mutations flip bit 7 alone (a byte pair that differs only there, 0x00 against 0x80 included), and one row is duplicated."""
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 256, (3, L), dtype=np.int64)
    anc[0, : L // 2] = 0
    a = anc[rng.integers(0, 3, n)]
    hit = rng.random((n, L)) < rng.uniform(0.0, 0.4, (n, 1))
    flip = rng.random((n, L)) < 0.5
    a = np.where(hit & flip, a ^ 0x80, np.where(hit, rng.integers(0, 256, (n, L)), a))
    if n >= 4:
        a[n - 1] = a[n // 2]
    return a.astype(np.uint8)


def strided(a, ld, seed, odd_address=False):
    """The device matrix uint8 [N, ld] holding ``a`` in its first columns and garbage (all byte values, different in every row)
    behind them; ``odd_address``: the matrix starts one byte into its allocation."""
    n, L = a.shape
    rng = np.random.default_rng(seed + 99)
    full = rng.integers(0, 256, (n, ld), dtype=np.int64).astype(np.uint8)
    full[:, :L] = a
    if not odd_address:
        return torch.from_numpy(full).cuda()
    flat = torch.zeros(n * ld + 1, dtype=torch.uint8, device="cuda")
    flat[1:] = torch.from_numpy(full.reshape(-1)).cuda()
    out = flat[1:].view(n, ld)
    assert out.data_ptr() % 4 == 1 and out.is_contiguous()
    return out


def strides(L):
    return (L, L + 3, (L + 3) // 4 * 4 + 4)


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32).cuda()


# ---- mismatch rows and neighbour counts against brute force ------------------------------------------------------------------
@pytest.mark.parametrize("L", LS)
def test_mismatch_rows_and_neighbour_counts_are_exact(L):
    for n in NS:
        a = byte_msa(n, L, 7 * n + L)
        want = M.mism(a)
        query = [0, n - 1, n // 2, -3, n + 5]  # the last two are clamped to the first and the last row
        thresholds = (-1, 0, M.max_mismatch(0.2, L), L)
        for ld in strides(L):
            dev = strided(a, ld, n + ld)
            got = ops.msa_mismatch_rows(dev, i32(query), L=L)
            assert got.dtype == torch.int32 and tuple(got.shape) == (len(query), n)
            assert np.array_equal(got.cpu().numpy(), M.mismatch_rows(a, query)), (n, L, ld)
            for m in thresholds:
                cnt = ops.msa_neighbor_counts(dev, m, L=L)
                assert np.array_equal(cnt.cpu().numpy(), (want <= m).sum(1)), (n, L, ld, m)
        dev = strided(a, (L + 3) // 4 * 4, n, odd_address=True)
        assert np.array_equal(ops.msa_mismatch_rows(dev, i32([n - 1]), L=L).cpu().numpy()[0], want[n - 1]), (n, L)
        m = M.max_mismatch(0.2, L)
        assert np.array_equal(ops.msa_neighbor_counts(dev, m, L=L).cpu().numpy(), (want <= m).sum(1)), (n, L)


def test_identical_rows_are_all_neighbours():
    for n, L in ((65, 5), (257, 130)):
        a = np.repeat(byte_msa(1, L, 3), n, axis=0)
        dev = torch.from_numpy(a).cuda()
        assert int(ops.msa_mismatch_rows(dev, i32([0, n - 1])).abs().sum()) == 0
        for m, want in ((-1, 0), (0, n), (L, n)):
            assert ops.msa_neighbor_counts(dev, m).tolist() == [want] * n, (n, L, m)


@pytest.fixture(scope="module")
def big():
    """The 2049 x 130 generator alignment, its brute-force neighbour counts at theta 0.2, and its device copy."""
    a = M.family_msa(2049, 130, 0)
    m = M.max_mismatch(0.2, 130)
    assert m == 25  # 0.2 * 130 is 26.0 in fp64
    return a, m, M.neighbor_counts(a, m), torch.from_numpy(a).cuda()


def test_neighbour_counts_over_many_workgroups(big):
    a, m, want, dev = big
    got = ops.msa_neighbor_counts(dev, m)
    assert np.array_equal(got.cpu().numpy(), want)
    assert want.max() > 64 and want.min() == 1  # neighbours in several column tiles; rows with none but themselves
    assert np.array_equal(ops.msa_neighbor_counts(dev, m).cpu().numpy(), want)  # the output is zeroed by the entry itself
    assert ops.msa_neighbor_counts(dev, 130).tolist() == [2049] * 2049
    q = [0, 1024, 2048]
    assert np.array_equal(ops.msa_mismatch_rows(dev, i32(q)).cpu().numpy(), M.mismatch_rows(a, q))
    pad = strided(a, 135, 5)  # rows at odd addresses
    assert np.array_equal(ops.msa_neighbor_counts(pad, m, L=130).cpu().numpy(), want)


# ---- the greedy pick against the integer reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L", [(257, 65), (2049, 130)])
def test_greedy_select_is_the_integer_rule(n, L):
    a = M.family_msa(n, L, 1)
    dev = torch.from_numpy(a).cuda()
    for mode in (0, 1):
        want = M.greedy(a, 32, 0, mode)
        for num in (1, 2, 32):
            got = ops.msa_greedy_select(dev, num, first=0, mode=mode)
            assert got.dtype == torch.int32 and got.tolist() == want[:num], (n, L, mode, num)
    first = n // 2  # the row the last row duplicates: after it the duplicate has the smallest sum, 0
    assert ops.msa_greedy_select(dev, 2, first=first, mode=1).tolist() == [first, n - 1] == M.greedy(a, 2, first, 1)
    pad = strided(a, L + 2, 3)
    assert ops.msa_greedy_select(pad, 32, mode=0, L=L).tolist() == M.greedy(a, 32, 0, 0)


def test_greedy_select_ties_go_to_the_lower_row():
    """The duplicated row has the sums of its original at every step: it must lose each tie to the lower index, and be picked
    right behind it when every row is picked."""
    a = M.family_msa(65, 65, 2)
    assert np.array_equal(a[64], a[32])
    dev = torch.from_numpy(a).cuda()
    for mode in (0, 1):
        want = M.greedy(a, 65, 0, mode)
        got = ops.msa_greedy_select(dev, 65, first=0, mode=mode).tolist()  # num = N: every row, in pick order
        assert got == want and sorted(got) == list(range(65))
        assert got.index(32) < got.index(64)
    # all rows equal: every sum ties at 0, so the picks ascend
    same = torch.from_numpy(np.repeat(a[:1], 9, axis=0)).cuda()
    assert ops.msa_greedy_select(same, 9, first=4, mode=0).tolist() == [4, 0, 1, 2, 3, 5, 6, 7, 8]


# ---- ranks -----------------------------------------------------------------------------------------------------------------------
def test_rank_keys_is_a_permutation_with_exact_tie_rules():
    nan, inf = float("nan"), float("inf")
    small = [0.5, nan, 0.5, inf, -1.0, nan, inf, -0.0, 0.0, -inf]
    got = ops.rank_keys(torch.tensor(small, dtype=torch.float64).cuda()).tolist()
    assert got == M.ranks(small).tolist() == [4, 8, 5, 6, 1, 9, 7, 2, 3, 0]
    assert got[9] == 0 and got[4] == 1 and got[7] < got[8] and got[0] < got[2] and got[3] < got[6] < got[1] < got[5]
    rng = np.random.default_rng(5)
    for n in (1, 255, 256, 257, 1500):
        key = rng.integers(0, 40, n).astype(np.float64) / 8.0  # many exact ties
        key[rng.random(n) < 0.05] = np.inf
        key[rng.random(n) < 0.05] = np.nan
        key[rng.random(n) < 0.05] = -np.inf
        got = ops.rank_keys(torch.from_numpy(key).cuda())
        assert got.dtype == torch.int32 and sorted(got.tolist()) == list(range(n)), n
        assert np.array_equal(got.cpu().numpy(), M.ranks(key)), n


# ---- race keys -------------------------------------------------------------------------------------------------------------------
def ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


@pytest.mark.parametrize("n,L", [(257, 65), (2049, 130)])
def test_race_keys_and_the_selection_of_the_smallest(n, L, big):
    for seed in SEEDS:
        a = M.family_msa(n, L, seed)
        counts = big[2] if (n, seed) == (2049, 0) else M.neighbor_counts(a, M.max_mismatch(0.2, L))
        cdev = torch.from_numpy(counts.astype(np.int32)).cuda()
        for sub in (0, 3):
            u = M.race_u(n, seed, sub)
            assert not (u == 0).any()
            plain = ops.msa_race_keys(n, seed, sub, device="cuda").cpu().numpy()
            # the entry returns keys only: with all counts one, key = -log(u), and since neighbouring 24-bit u are at least
            # 2^-24 apart in -log(u) while the key is good to a few ulp, exp(-key) * 2^24 rounds to the integer the device drew
            assert np.array_equal(np.rint(np.exp(-plain) * 2.0 ** 24) * 2.0 ** -24, u), (n, seed, sub)
            want_plain = M.race_keys(n, seed, sub)
            assert ulps(plain, want_plain).max() <= 4.0, (n, seed, sub, ulps(plain, want_plain).max())
            got = ops.msa_race_keys(n, seed, sub, counts=cdev).cpu().numpy()
            want = M.race_keys(n, seed, sub, counts)
            assert ulps(got, want).max() <= 4.0, (n, seed, sub, ulps(got, want).max())
            for w, g, c in ((want, got, cdev), (want_plain, plain, None)):
                gap = M.min_relative_gap(w)
                assert gap > 1e-9, (n, seed, sub, gap)  # distinct keys are far enough apart for 4 ulp not to reorder them
                for num in (2, 32, n - 1):
                    keys = ops.msa_race_keys(n, seed, sub, counts=c, device="cuda")
                    keys[0] = -1.0
                    pick = (ops.rank_keys(keys) < num).nonzero().view(-1).tolist()
                    assert pick == M.weighted_pick(n, num, seed, sub, None if c is None else counts), (n, seed, sub, num)


def test_race_keys_edge_counts_and_geometry():
    n = 70000  # more rows than one launch's threads: the grid-stride path; the keys depend on (seed, subsample, i) alone
    counts = np.ones(n, dtype=np.int32)
    counts[[1, 5]] = [0, -7]
    counts[9] = 2 ** 31 - 1
    got = ops.msa_race_keys(n, 2 ** 63 + 11, 4, counts=torch.from_numpy(counts).cuda()).cpu().numpy()
    want = M.race_keys(n, 2 ** 63 + 11, 4, counts)
    assert np.isinf(got[1]) and np.isinf(got[5]) and got[1] > 0 and got[5] > 0
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and ulps(got[fin], want[fin]).max() <= 4.0
    head = ops.msa_race_keys(300, 2 ** 63 + 11, 4, device="cuda").cpu().numpy()
    assert np.array_equal(head[[0, 2, 3, 4, 299]], got[[0, 2, 3, 4, 299]])  # the same key alone and among 70000
