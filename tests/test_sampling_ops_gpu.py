"""The three single-kernel entries of sampling (csrc/sampling.hip), one op at a time, against the numpy references of
tests/_sampling_ref.py: the shuffle and the uniforms bit for bit (integer arithmetic), the drawn token against the fp64 draw
on every decided row (the threshold is farther than 1e-5 * total from every boundary of the cumulative sum; at most 0.5 % of
the rows may be undecided), logq within 4 fp32 ulp at max(1, |log total|), the write-back exactly."""
import functools
import math

import numpy as np
import pytest
import torch

import _sampling_ref as R
from esm_amd import _native as N
from esm_amd import ops

pytestmark = pytest.mark.gpu
V = 33
STANDARD = sum(1 << v for v in range(4, 24))  # the 20 standard residues of the ESM-1b alphabet


def i32(x):
    return torch.tensor(x, dtype=torch.int32).cuda()


# ---- permute_positions --------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 63, 0, 64, 65, 1022)
CHAINS = (5, 0, 17, 3, 2 ** 31 - 1, 9, 1)


def lists_of(lengths):
    return [list(range(1 + 3 * c, 1 + 3 * c + n)) for c, n in enumerate(lengths)]


def run_permute(lists, chains, seed, epoch):
    off = [0]
    for ps in lists:
        off.append(off[-1] + len(ps))
    got = ops.permute_positions(i32(off), i32([p for ps in lists for p in ps]), i32(chains), seed=seed, epoch=epoch).cpu().tolist()
    return [got[a:b] for a, b in zip(off, off[1:])]


def test_permute_positions_is_the_reference_shuffle():
    lists = lists_of(LENGTHS)
    seed = 0xDEADBEEF12345678
    got = run_permute(lists, CHAINS, seed, epoch=4)
    for ps, chain, g in zip(lists, CHAINS, got):
        assert g == R.shuffle(ps, seed, chain, 4), (len(ps), chain)
    assert got[3] == [] and got[0] == lists[0] and got[6] != lists[6]
    # the chains in another order, and each alone: the same slices
    order = [6, 2, 0, 5, 3, 1, 4]
    again = run_permute([lists[i] for i in order], [CHAINS[i] for i in order], seed, epoch=4)
    assert again == [got[i] for i in order]
    for i in (2, 6):
        assert run_permute([lists[i]], [CHAINS[i]], seed, epoch=4) == [got[i]]
    other = run_permute(lists, CHAINS, seed, epoch=5)
    assert other[6] != got[6] and other[4] != got[4] and sorted(other[6]) == lists[6]
    assert run_permute(lists, CHAINS, seed + 1, epoch=4)[6] != got[6]


def test_permute_positions_device_data_rules():
    """Offsets are device data: clamped to [0, total], a descending pair is an empty list; elements outside every slice are 0."""
    pos = list(range(10, 20))
    got = ops.permute_positions(i32([5, 2, 2, 50]), i32(pos), i32([1, 2, 3]), seed=7, epoch=0).cpu().tolist()
    assert got == [0, 0] + R.shuffle(pos[2:10], 7, 3, 0)  # [5, 2) and [2, 2) are empty, [2, 50) is [2, 10)
    got = ops.permute_positions(i32([-4, 3, 3, 10]), i32(pos), i32([1, 2, 3]), seed=7, epoch=0).cpu().tolist()
    assert got == R.shuffle(pos[0:3], 7, 1, 0) + R.shuffle(pos[3:10], 7, 3, 0)
    many = 300  # more chains than one workgroup has lanes
    lists = [list(range(5)) for _ in range(many)]
    out = run_permute(lists, list(range(many)), 3, 1)
    assert all(out[c] == R.shuffle(lists[c], 3, c, 1) for c in range(many))


# ---- sample_rows ----------------------------------------------------------------------------------------------------------
N_ROWS = 4096
SEED, STEP = 0x0123456789ABCDEF, 37


@functools.lru_cache(maxsize=None)
def table():
    """Log-probabilities of N(0, 3^2) logits, the counters of every row and the token each row excludes; left unchanged."""
    rng = np.random.default_rng(23)
    logits = (3.0 * rng.standard_normal((N_ROWS, V))).astype(np.float32)
    lp = torch.log_softmax(torch.from_numpy(logits), -1).numpy()
    chain = rng.integers(0, 2 ** 31 - 1, N_ROWS).astype(np.int32)
    index = rng.integers(0, 1024, N_ROWS).astype(np.int32)
    exclude = rng.integers(4, 24, N_ROWS).astype(np.int32)
    exclude[::7] = -1
    return lp, chain, index, exclude


@pytest.mark.parametrize("with_exclude", [False, True])
@pytest.mark.parametrize("temperature", [0.5, 1.0, 2.0])
def test_sample_rows_against_the_fp64_draw(temperature, with_exclude):
    lp, chain, index, exclude = table()
    inv_t = 1.0 / temperature
    tok, logq, u = ops.sample_rows(torch.from_numpy(lp).cuda(), i32(chain), i32(index), STANDARD, inv_t, seed=SEED, step=STEP,
                                   exclude=i32(exclude) if with_exclude else None)
    tok, logq, u = tok.cpu().numpy(), logq.cpu().numpy(), u.cpu().numpy()
    want_u = R.uniform(SEED, chain, STEP, index)
    assert u.dtype == np.float32 and np.array_equal(u.view(np.uint32), want_u.view(np.uint32))
    undecided, worst = 0, 0.0
    for i in range(N_ROWS):
        ex = int(exclude[i]) if with_exclude else -1
        cand = R.candidates(V, STANDARD, ex)
        assert int(tok[i]) in cand, i
        want, want_logq, decided = R.draw(lp[i], u[i], STANDARD, inv_t, ex)
        if not decided:
            undecided += 1
            continue
        assert int(tok[i]) == want, (i, int(tok[i]), want)
        z = lp[i][cand].astype(np.float64) * float(np.float32(inv_t))
        log_total = math.log(np.exp(z - z.max()).sum())
        err = abs(float(logq[i]) - want_logq)
        worst = max(worst, err / R.logq_bound(log_total))
        assert err <= R.logq_bound(log_total), (i, float(logq[i]), want_logq)
    print(f"temperature {temperature} exclude {with_exclude}: undecided {undecided} of {N_ROWS}, worst logq error {worst:.3f} "
          "of the bound")
    assert undecided <= R.UNDECIDED_CAP * N_ROWS, undecided


def test_sample_rows_does_not_depend_on_the_launch():
    """A row's draw depends on its own counter and values only: any subset, in any order, gives the same bits."""
    lp, chain, index, _ = table()
    full = ops.sample_rows(torch.from_numpy(lp).cuda(), i32(chain), i32(index), STANDARD, 1.0, seed=SEED, step=STEP)
    pick = np.random.default_rng(1).permutation(N_ROWS)[:301]
    part = ops.sample_rows(torch.from_numpy(lp[pick]).cuda(), i32(chain[pick]), i32(index[pick]), STANDARD, 1.0, seed=SEED,
                           step=STEP)
    for a, b in zip(full, part):
        assert torch.equal(a.cpu()[torch.from_numpy(pick)], b.cpu())
    other = ops.sample_rows(torch.from_numpy(lp).cuda(), i32(chain), i32(index), STANDARD, 1.0, seed=SEED, step=STEP + 1)
    assert not torch.equal(other[2], full[2]) and not torch.equal(other[0], full[0])
    assert ops.sample_rows(torch.from_numpy(lp).cuda(), i32(chain), i32(index), STANDARD, 1.0, seed=SEED, step=STEP,
                           want_u=False)[2] is None


def one_row(row, mask, inv_t=1.0, exclude=None, seed=SEED, step=STEP, chain=0, index=0):
    lp = torch.tensor([row], dtype=torch.float32).cuda()
    tok, logq, u = ops.sample_rows(lp, i32([chain]), i32([index]), mask, inv_t, seed=seed, step=step,
                                   exclude=None if exclude is None else i32([exclude]))
    return int(tok.item()), float(logq.item()), float(u.item())


def test_sample_rows_edge_rows():
    row = torch.log_softmax(torch.linspace(-2.0, 2.0, V), -1).tolist()
    # one candidate only: it is drawn with probability 1
    assert one_row(row, 1 << 9)[:2] == (9, 0.0)
    assert one_row(row, (1 << 9) | (1 << 12), exclude=12)[:2] == (9, 0.0)
    # u = 0: the first candidate (a counter whose uniform is exactly 0)
    tok, _, u = one_row(row, STANDARD, seed=2024, chain=7, step=3, index=17499144)
    assert u == 0.0 and tok == 4
    # all mass on the last candidate: the others underflow to weight 0
    heavy = [-200.0] * V
    heavy[23] = 0.0
    assert one_row(heavy, STANDARD)[:2] == (23, 0.0)
    # ... and on the first one
    heavy = [-200.0] * V
    heavy[4] = 0.0
    assert one_row(heavy, STANDARD)[:2] == (4, 0.0)
    # an exclude that empties the candidate set
    assert one_row(row, 1 << 9, exclude=9)[:2] == (-1, 0.0)
    assert one_row(row, 0)[0] == -1
    assert one_row(row, 1 << 40)[0] == -1  # only bits below V count
    # an exclude outside the vocabulary excludes nothing
    assert one_row(row, 1 << 9, exclude=-1)[0] == 9 and one_row(row, 1 << 9, exclude=64)[0] == 9
    # V = 64 with bit 63 allowed
    wide = [-200.0] * 64
    wide[63] = -0.5
    assert one_row(wide, 1 << 63)[:2] == (63, 0.0)
    assert one_row(wide, (1 << 63) | 1)[0] == 63
    assert one_row(wide, 2 ** 64 - 1, inv_t=0.0)[:2] == (63, 0.0)
    # greedy: the largest log-probability among the candidates, an exact tie to the lowest index
    tie = [-3.0] * V
    tie[2], tie[7], tie[11], tie[20] = 0.0, -1.0, -1.0, -1.0  # token 2 is no candidate
    assert one_row(tie, STANDARD, inv_t=0.0)[:2] == (7, 0.0)
    assert one_row(tie, STANDARD, inv_t=0.0, exclude=7)[:2] == (11, 0.0)


def test_sample_rows_frequencies():
    """65536 rows sharing one distribution: every token's count within 5 sigma + 1 of its expectation (fixed seed)."""
    n = 65536
    rng = np.random.default_rng(5)
    logits = (1.5 * rng.standard_normal(V)).astype(np.float32)
    row = torch.log_softmax(torch.from_numpy(logits), -1)
    lp = row.repeat(n, 1).contiguous().cuda()
    chain = torch.arange(n, dtype=torch.int32).cuda() % 64
    index = torch.div(torch.arange(n, dtype=torch.int32).cuda(), 64, rounding_mode="floor").to(torch.int32)
    inv_t = 1.0 / 1.5
    tok, _, _ = ops.sample_rows(lp, chain.contiguous(), index.contiguous(), STANDARD, inv_t, seed=99, step=0)
    counts = torch.bincount(tok.cpu().long(), minlength=V).numpy()
    cand = R.candidates(V, STANDARD)
    z = row.numpy()[cand].astype(np.float64) * float(np.float32(inv_t))
    p = np.exp(z - z.max())
    p /= p.sum()
    assert counts.sum() == n and counts[[v for v in range(V) if v not in cand]].sum() == 0
    for v, pv in zip(cand, p):
        assert abs(counts[v] - n * pv) <= 5.0 * math.sqrt(n * pv * (1.0 - pv)) + 1.0, (v, counts[v], n * pv)


# ---- commit_tokens --------------------------------------------------------------------------------------------------------
def test_commit_tokens_writes_exactly_the_named_elements():
    B, T = 3, 70
    g = torch.Generator().manual_seed(2)
    guard = 64  # int64 elements in front of and behind the matrix: nothing outside it may change
    buf = torch.randint(4, 24, (guard + B * T + guard,), generator=g, dtype=torch.int64)
    before = buf.clone()
    dev = buf.cuda()
    tokens = dev[guard: guard + B * T].view(B, T)
    slot = [0, 2, 1, 1, 0, 2, 7, -3, 1]
    pos = [0, 69, 5, 6, -1, 70, 4, 9, 2 ** 31 - 1]
    tok = [30, 31, -1, 29, 28, 27, 26, 25, 24]
    assert ops.commit_tokens(tokens, i32(slot), i32(pos), i32(tok)) is tokens
    want = before.clone()
    m = want[guard: guard + B * T].view(B, T)
    m[0, 0], m[2, 69], m[1, 6] = 30, 31, 29  # token -1 and positions -1, 70 and 2^31 - 1 write nothing
    m[2, 4], m[0, 9] = 26, 25  # slots 7 and -3 are clamped to the last and the first chain
    assert torch.equal(dev.cpu(), want)
    n = 70000  # more rows than one turn of the grid: every element of a [1000, 70] matrix exactly once
    big = torch.zeros((1000, 70), dtype=torch.int64).cuda()
    e = torch.randperm(n, generator=g)
    ops.commit_tokens(big, i32((e // 70).tolist()), i32((e % 70).tolist()), i32((e % 31).tolist()))
    assert torch.equal(big.cpu().view(-1)[e], e % 31)


# ---- validation -----------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    lp = torch.zeros((4, V), dtype=torch.float32).cuda()
    four = i32([0, 1, 2, 3])
    out_t, out_q = torch.full((4,), 77, dtype=torch.int32).cuda(), torch.full((4,), 7.0).cuda()

    def d(lp_=lp, chain=four, index=four, tok=out_t, logq=out_q, n=4, v=V, inv_t=1.0):
        return N.lib.esmk_op_sample_rows(N.ptr(lp_), N.ptr(chain), N.ptr(index), None, STANDARD, inv_t, 1, 0, N.ptr(tok),
                                         N.ptr(logq), None, n, v, N.cur_stream())

    for kw in (dict(lp_=None), dict(chain=None), dict(index=None), dict(tok=None), dict(logq=None), dict(n=0), dict(n=-1),
               dict(v=65), dict(v=0), dict(inv_t=-0.5), dict(inv_t=float("nan"))):
        assert d(**kw) != 0, kw
    tokens = torch.full((2, 8), 5, dtype=torch.int64).cuda()
    c = N.lib.esmk_op_commit_tokens
    assert c(None, N.ptr(four), N.ptr(four), N.ptr(four), 4, 2, 8, N.cur_stream()) != 0
    assert c(N.ptr(tokens), N.ptr(four), N.ptr(four), N.ptr(four), 0, 2, 8, N.cur_stream()) != 0
    assert c(N.ptr(tokens), N.ptr(four), N.ptr(four), N.ptr(four), 4, 0, 8, N.cur_stream()) != 0
    perm_out = torch.full((4,), 77, dtype=torch.int32).cuda()
    p = N.lib.esmk_op_permute_positions
    assert p(N.ptr(i32([0, 4])), N.ptr(four), N.ptr(i32([0])), None, 1, 4, 1, 0, N.cur_stream()) != 0
    assert p(N.ptr(i32([0, 4])), N.ptr(four), N.ptr(i32([0])), N.ptr(perm_out), 0, 4, 1, 0, N.cur_stream()) != 0
    assert p(N.ptr(i32([0, 4])), N.ptr(four), N.ptr(i32([0])), N.ptr(perm_out), 1, 0, 1, 0, N.cur_stream()) != 0
    torch.cuda.synchronize()
    assert out_t.cpu().tolist() == [77] * 4 and out_q.cpu().tolist() == [7.0] * 4 and perm_out.cpu().tolist() == [77] * 4
    assert (tokens.cpu() == 5).all()
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            ops.sample_rows(lp, four, four, STANDARD, 1.0, seed=bad)
