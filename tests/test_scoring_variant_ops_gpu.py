"""The two single-kernel entries of multi-mutant variant scoring (csrc/scoring.hip), one op at a time: the joint-mask batch
builder against a clone-and-assign in torch, and the per-variant sum against a host loop that takes the fp32 difference of
every row and adds in fp64 in index order (exact: no tolerance)."""
import numpy as np
import pytest
import torch

from esm_amd import ops

pytestmark = pytest.mark.gpu
B, T, MASK = 2, 70, 32


def tokens_of(b, t, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(4, 24, (b, t), generator=g, dtype=torch.int64)


def want_rows(tokens, sets, src, mask=MASK):
    """The clone-and-assign: copy i is sequence src[i] with the positions of sets[i] that lie inside the row masked."""
    t = tokens.shape[1]
    out = []
    for s, b in zip(sets, src):
        row = tokens[min(max(b, 0), tokens.shape[0] - 1)].clone()
        for p in s:
            if 0 <= p < t:
                row[p] = mask
        out.append(row)
    return torch.stack(out)


def run(tokens, sets, src=None, offsets=None, mask=MASK):
    pos = torch.tensor([p for s in sets for p in s], dtype=torch.int32)
    if offsets is None:
        offsets = [0]
        for s in sets:
            offsets.append(offsets[-1] + len(s))
    off = torch.tensor(offsets, dtype=torch.int32)
    src_d = None if src is None else torch.tensor(src, dtype=torch.int32).cuda()
    return ops.mask_rows_multi(tokens.cuda(), off.cuda(), pos.cuda(), src_d, mask_idx=mask).cpu()


@pytest.mark.parametrize("with_src", [False, True])
def test_mask_rows_multi_equals_clone_and_assign(with_src):
    tokens = tokens_of(B, T, seed=3)
    g = torch.Generator().manual_seed(4)
    sets = [torch.randperm(T, generator=g)[:k].tolist() for k in (1, 2, 7, 70, 2, 1, 7)]
    sets[1] = [0, T - 1]  # both ends of the row
    assert sorted(sets[3]) == list(range(T))  # every position
    src = [1, 0, 1, 1, 0, 0, 1] if with_src else None
    got = run(tokens, sets, src)
    assert got.dtype == torch.int64 and got.shape == (len(sets), T)
    assert torch.equal(got, want_rows(tokens, sets, src if with_src else [0] * len(sets)))
    assert (got[3] == MASK).all() and int((got[0] == MASK).sum()) == 1
    if not with_src:  # a [T] row is the only sequence
        assert torch.equal(run(tokens[0], sets), got)


def test_mask_rows_multi_device_data_rules():
    """The lists are device data the host never saw: nothing in them may make the kernel read or write outside its rows."""
    tokens = tokens_of(B, T, seed=5)
    # a repeated position; positions -1 and T (mask nothing) next to a real one; an empty list; a far-away position
    sets = [[5, 5, 9, 5], [-1, T, 12], [], [2 ** 31 - 1, -(2 ** 31), 3]]
    got = run(tokens, sets, src=[0, 1, 1, 0])
    assert torch.equal(got, want_rows(tokens, sets, [0, 1, 1, 0]))
    assert got[0].eq(MASK).nonzero().view(-1).tolist() == [5, 9] and got[1].eq(MASK).nonzero().view(-1).tolist() == [12]
    assert torch.equal(got[2], tokens[1])  # the empty list: a plain copy
    # a source row of B + 3 (clamped to the last sequence) and a negative one (clamped to the first)
    got = run(tokens, [[4], [6]], src=[B + 3, -7])
    assert torch.equal(got, want_rows(tokens, [[4], [6]], [B - 1, 0]))
    # a descending offset pair is an empty list; offsets outside [0, total] are clamped to it
    pos = [1, 2, 3, 4, 5, 6]
    flat = [pos]  # run() flattens the sets: here the position list is given whole and the offsets by hand
    got = run(tokens, flat, offsets=[0, 2, 1, 4, -3, 2, 100])  # copies: [0,2) | [2,1) empty | [1,4) | [4,0) empty | [0,2) | [2,6)
    want = want_rows(tokens, [[1, 2], [], [2, 3, 4], [], [1, 2], [3, 4, 5, 6]], [0] * 6)
    assert torch.equal(got, want)
    # no position at all (total = 0): plain copies
    got = run(tokens, [[], []], src=[1, 0])
    assert torch.equal(got, tokens[[1, 0]])


def test_mask_rows_multi_copy_loop_wraps_the_grid():
    """n = 9000 copies at T = 8: more copies than the 8192 workgroups of the grid cap, so the copy loop takes a second turn."""
    n, t = 9000, 8
    tokens = tokens_of(3, t, seed=6)
    g = torch.Generator().manual_seed(7)
    k = torch.randint(0, 4, (n,), generator=g)  # 0 .. 3 positions per copy
    off = torch.zeros((n + 1,), dtype=torch.int64)
    off[1:] = k.cumsum(0)
    pos = torch.randint(0, t, (int(off[-1]),), generator=g)
    src = torch.randint(0, 3, (n,), generator=g)
    want = tokens[src].clone()
    copy = torch.repeat_interleave(torch.arange(n), k)
    want[copy, pos] = MASK
    got = ops.mask_rows_multi(tokens.cuda(), off.to(torch.int32).cuda(), pos.to(torch.int32).cuda(), src.to(torch.int32).cuda(),
                              mask_idx=MASK).cpu()
    assert torch.equal(got, want)
    assert not torch.equal(got[8192:], tokens[src[8192:]])  # the copies of the second turn were masked too


# ---- score_rows -----------------------------------------------------------------------------------------------------------
def host_sums(lp, wt, mt, offsets):
    """The definition, on the host: fp32 difference per row, added in fp64 in index order; columns clamped to [0, V), offsets
    to [0, n_rows]."""
    n_rows, V = lp.shape
    rows, wt, mt = lp.numpy(), wt.tolist(), mt.tolist()
    out = []
    for v in range(len(offsets) - 1):
        lo, hi = (min(max(o, 0), n_rows) for o in (offsets[v], offsets[v + 1]))
        total = 0.0  # a Python float: fp64
        for r in range(lo, hi):
            term = rows[r, min(max(mt[r], 0), V - 1)] - rows[r, min(max(wt[r], 0), V - 1)]
            assert term.dtype == np.float32
            total += float(term)
        out.append(total)
    return torch.tensor(out, dtype=torch.float64)


def table(seed=11):
    g = torch.Generator().manual_seed(seed)
    lp = torch.log_softmax(4.0 * torch.randn((111, 33), generator=g), -1)
    wt = torch.randint(0, 33, (111,), generator=g, dtype=torch.int32)
    mt = torch.randint(0, 33, (111,), generator=g, dtype=torch.int32)
    return lp, wt, mt


def test_score_rows_is_the_ordered_fp64_sum():
    lp, wt, mt = table()
    offsets = [0, 1, 3, 6, 70, 70, 111]  # ranges of 1, 2, 3, 64, none and 41 rows
    assert [b - a for a, b in zip(offsets, offsets[1:])] == [1, 2, 3, 64, 0, 41]
    got = ops.score_rows(lp.cuda(), wt.cuda(), mt.cuda(), torch.tensor(offsets, dtype=torch.int32).cuda())
    want = host_sums(lp, wt, mt, offsets)
    assert got.dtype == torch.float64 and got.shape == (6,)
    assert torch.equal(got.cpu(), want)
    assert got[4].item() == 0.0
    # a single row: the fp32 difference itself, the float score_mutations computes
    assert got[0].item() == (lp[0, mt[0]] - lp[0, wt[0]]).item()
    # one lane per variant: the same ranges in another launch geometry (each 50 times over: two workgroups) give the same
    # bits; the wrap-around pair (70, 0) is one more empty range
    many = offsets[:-1] * 50 + [111]
    big = ops.score_rows(lp.cuda(), wt.cuda(), mt.cuda(), torch.tensor(many, dtype=torch.int32).cuda()).cpu()
    assert torch.equal(big, host_sums(lp, wt, mt, many))
    assert torch.equal(big[:5], want[:5]) and torch.equal(big[6 * 49: 6 * 49 + 5], want[:5])


def test_score_rows_device_data_rules():
    lp, wt, mt = table(seed=12)
    wt[3], mt[3], wt[4], mt[4] = -1, 33, 2 ** 31 - 1, -(2 ** 31)  # columns outside [0, V): clamped
    offsets = [-5, 3, 6, 2, 500, 111, 90]  # below 0, a descending pair (empty), beyond n_rows, and descending at the end
    got = ops.score_rows(lp.cuda(), wt.cuda(), mt.cuda(), torch.tensor(offsets, dtype=torch.int32).cuda()).cpu()
    assert torch.equal(got, host_sums(lp, wt, mt, offsets))
    assert got[2].item() == 0.0 and got[4].item() == 0.0 and got[5].item() == 0.0  # [6,2), [111,111), [111,90)
    assert got[3].item() != 0.0  # [2, 111)
    only = ops.score_rows(lp.cuda(), wt.cuda(), mt.cuda(), torch.tensor([3, 5], dtype=torch.int32).cuda()).cpu()
    want = (lp[3, 32] - lp[3, 0]).double() + (lp[4, 0] - lp[4, 32]).double()
    assert only.item() == want.item()
