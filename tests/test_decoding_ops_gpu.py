"""The two decoding entries (csrc/sampling.hip: esmk_op_sample_rows_ex, esmk_op_select_rows), one op at a time, against the
numpy references of tests/_decoding_ref.py.  Filters off: the bits of esmk_op_sample_rows.  Filters on: the kept set and the
token equal the fp64 reference on every decided row (every E_r farther than 1e-5 W from top_p W, and the draw over the kept
set decided by the rule of tests/_sampling_ref.py; at most 0.5 % of the rows may be undecided), logq within 4 fp32 ulp at
max(1, |log total|).  Scores within 4 fp32 ulp at max(1, |score|) on every row.  The selection is comparison logic: exact."""
import math

import numpy as np
import pytest
import torch

import _decoding_ref as D
import _sampling_ref as R
import test_sampling_ops_gpu as S  # the 4096-row table of the plain draw's test: built once, shared, left unchanged
from esm_amd import ops

pytestmark = pytest.mark.gpu
V, N_ROWS, STANDARD, SEED, STEP = S.V, S.N_ROWS, S.STANDARD, S.SEED, S.STEP
ALL64 = 2 ** 64 - 1


def i32(x):
    return torch.tensor(np.asarray(x), dtype=torch.int32).cuda()


def bits(kept):
    """The kept sets of a call as Python ints in [0, 2^64)."""
    return [int(k) & ALL64 for k in kept.cpu().tolist()]


def run_ex(lp, chain, index, mask=STANDARD, inv_t=1.0, exclude=None, **kw):
    out = ops.sample_rows_ex(torch.from_numpy(np.ascontiguousarray(lp)).cuda(), i32(chain), i32(index), mask, inv_t, seed=SEED,
                             step=STEP, exclude=None if exclude is None else i32(exclude), **kw)
    return [None if t is None else t.cpu() for t in out]


# ---- filters off ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_exclude", [False, True])
@pytest.mark.parametrize("inv_t", [1.0 / 0.7, 1.0, 0.0], ids=["tempered", "plain", "greedy"])
def test_filters_off_is_sample_rows_bit_for_bit(inv_t, with_exclude):
    lp, chain, index, exclude = S.table()
    ex = i32(exclude) if with_exclude else None
    dev = torch.from_numpy(lp).cuda()
    want = ops.sample_rows(dev, i32(chain), i32(index), STANDARD, inv_t, seed=SEED, step=STEP, exclude=ex)
    got = ops.sample_rows_ex(dev, i32(chain), i32(index), STANDARD, inv_t, seed=SEED, step=STEP, exclude=ex, top_k=0, top_p=1.0,
                             score=None)
    assert torch.equal(got[0], want[0])
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    assert torch.equal(got[2].view(torch.int32), want[2].view(torch.int32))
    assert got[3] is None
    cand = [sum(1 << v for v in R.candidates(V, STANDARD, int(exclude[i]) if with_exclude else -1)) for i in range(N_ROWS)]
    assert bits(got[4]) == cand
    # asking for a score changes nothing else
    more = ops.sample_rows_ex(dev, i32(chain), i32(index), STANDARD, inv_t, seed=SEED, step=STEP, exclude=ex, score="entropy",
                              want_u=False, want_kept=False)
    assert torch.equal(more[0], want[0]) and torch.equal(more[1].view(torch.int32), want[1].view(torch.int32))
    assert more[2] is None and more[4] is None and more[3].dtype == torch.float32


# ---- filters on -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inv_t", [1.0, 1.0 / 0.7, 0.5])
@pytest.mark.parametrize("top_k,top_p", [(0, 0.9), (5, 0.5), (3, 1.0)])
def test_filtered_draw_against_the_fp64_reference(top_k, top_p, inv_t):
    lp, chain, index, _ = S.table()
    tok, logq, u, _, kept = run_ex(lp, chain, index, inv_t=inv_t, top_k=top_k, top_p=top_p)
    tok, logq, u, kept = tok.numpy(), logq.numpy(), u.numpy(), bits(kept)
    want_u = R.uniform(SEED, chain, STEP, index)
    assert np.array_equal(u.view(np.uint32), want_u.view(np.uint32))
    undecided, worst, sizes = 0, 0.0, 0
    for i in range(N_ROWS):
        assert kept[i] != 0 and kept[i] & ~STANDARD == 0 and (kept[i] >> int(tok[i])) & 1, i
        want_tok, want_logq, want_kept, decided = D.draw_ex(lp[i], u[i], STANDARD, inv_t, top_k, top_p)
        if not decided:
            undecided += 1
            continue
        assert kept[i] == want_kept, (i, bin(kept[i]), bin(want_kept))
        assert int(tok[i]) == want_tok, (i, int(tok[i]), want_tok)
        sizes += bin(want_kept).count("1")
        z = lp[i][R.candidates(V, want_kept)].astype(np.float64) * float(np.float32(inv_t))
        log_total = math.log(np.exp(z - z.max()).sum())
        err = abs(float(logq[i]) - want_logq)
        worst = max(worst, err / R.logq_bound(log_total))
        assert err <= R.logq_bound(log_total), (i, float(logq[i]), want_logq)
    print(f"top_k {top_k} top_p {top_p} inv_t {inv_t:.3f}: undecided {undecided} of {N_ROWS}, mean kept "
          f"{sizes / max(N_ROWS - undecided, 1):.2f}, worst logq error {worst:.3f} of the bound")
    assert undecided <= R.UNDECIDED_CAP * N_ROWS, undecided


def test_filtered_draw_does_not_depend_on_the_launch():
    lp, chain, index, exclude = S.table()
    kw = dict(inv_t=1.0 / 0.7, exclude=exclude, top_k=7, top_p=0.8, score="confidence")
    full = run_ex(lp, chain, index, **kw)
    pick = np.random.default_rng(2).permutation(N_ROWS)[:301]
    part = run_ex(lp[pick], chain[pick], index[pick], **dict(kw, exclude=exclude[pick]))
    for a, b in zip(full, part):
        assert torch.equal(a[torch.from_numpy(pick)].view(torch.int32 if a.dtype == torch.float32 else a.dtype),
                           b.view(torch.int32 if b.dtype == torch.float32 else b.dtype))


def test_top_k_one_is_the_greedy_token_on_every_row():
    lp, chain, index, exclude = S.table()
    for ex in (None, exclude):
        greedy = run_ex(lp, chain, index, inv_t=0.0, exclude=ex)
        for inv_t in (1.0, 1.0 / 0.7):
            one = run_ex(lp, chain, index, inv_t=inv_t, exclude=ex, top_k=1)
            assert torch.equal(one[0], greedy[0])
            assert bool((one[1] == 0).all())  # the only kept token has probability 1
            assert bits(one[4]) == [1 << int(t) for t in one[0].tolist()]
    # greedy ignores the filters
    for kw in (dict(top_k=1), dict(top_k=3, top_p=0.2)):
        assert torch.equal(run_ex(lp, chain, index, inv_t=0.0, exclude=exclude, **kw)[0], greedy[0])


# ---- edges ----------------------------------------------------------------------------------------------------------------
def one_row(row, mask, inv_t=1.0, exclude=None, **kw):
    tok, logq, u, score, kept = run_ex(np.array([row], dtype=np.float32), [3], [11], mask=mask, inv_t=inv_t,
                                       exclude=None if exclude is None else [exclude], **kw)
    return int(tok.item()), float(logq.item()), bits(kept)[0], None if score is None else float(score.item())


def test_edge_rows():
    row = torch.log_softmax(torch.linspace(-2.0, 2.0, V), -1).numpy()
    three = (1 << 5) | (1 << 9) | (1 << 20)
    # top_k larger than the candidate count: nothing is filtered
    tok, logq, kept, _ = one_row(row, three, top_k=10)
    plain = ops.sample_rows(torch.from_numpy(row[None]).cuda(), i32([3]), i32([11]), three, 1.0, seed=SEED, step=STEP)
    assert kept == three and tok == int(plain[0].item()) and logq == float(plain[1].item())
    assert one_row(row, three, top_k=64)[2] == three and one_row(row, STANDARD, top_k=20)[2] == STANDARD
    assert one_row(row, three, top_k=2)[2] == (1 << 9) | (1 << 20)  # the row ascends: the two highest tokens
    # two equal maxima go to the lower token
    tie = [-3.0] * V
    tie[2], tie[7], tie[11], tie[20] = 0.0, -1.0, -1.0, -1.0  # token 2 is no candidate
    assert one_row(tie, STANDARD, top_k=1)[:3] == (7, 0.0, 1 << 7)
    assert one_row(tie, STANDARD, top_k=2)[2] == (1 << 7) | (1 << 11)
    assert one_row(tie, STANDARD, top_k=1, exclude=7)[:3] == (11, 0.0, 1 << 11)
    assert one_row(tie, STANDARD, top_k=3, score="confidence")[2] == (1 << 7) | (1 << 11) | (1 << 20)
    # a single candidate: probability 1, entropy 0
    assert one_row(row, 1 << 9, top_k=3, top_p=0.5, score="confidence") == (9, 0.0, 1 << 9, 0.0)
    assert one_row(row, 1 << 9, top_p=0.1, score="entropy") == (9, 0.0, 1 << 9, 0.0)
    assert one_row(row, (1 << 9) | (1 << 12), top_k=2, exclude=12, score="entropy") == (9, 0.0, 1 << 9, 0.0)
    # no candidate: token -1, score -inf, nothing kept
    for kw in (dict(top_k=3), dict(top_p=0.5), dict()):
        assert one_row(row, 1 << 9, exclude=9, score="confidence", **kw) == (-1, 0.0, 0, -math.inf)
        assert one_row(row, 0, score="entropy", **kw) == (-1, 0.0, 0, -math.inf)
        assert one_row(row, 1 << 40, score="entropy", **kw) == (-1, 0.0, 0, -math.inf)  # only bits below V count
    # a row of -inf candidates has no distribution: the weights are NaN, no comparison with them holds.  top_k alone keeps
    # the k lowest tokens (all tie) and draws the last of them; a nucleus keeps the best candidate only; greedy takes it
    dead = [-math.inf] * V
    tok, logq, kept, score = one_row(dead, three, top_k=2, score="confidence")
    assert (tok, kept) == (9, (1 << 5) | (1 << 9)) and math.isnan(logq) and math.isnan(score)
    assert kept == D.keep_set(np.array(dead, dtype=np.float32), three, 1.0, top_k=2)[0]
    tok, logq, kept, score = one_row(dead, three, top_p=0.5, score="entropy")
    assert (tok, kept) == (5, 1 << 5) and math.isnan(logq) and math.isnan(score)
    assert kept == D.keep_set(np.array(dead, dtype=np.float32), three, 1.0, top_p=0.5)[0]
    assert one_row(dead, three, inv_t=0.0, top_k=2)[:2] == (5, 0.0)
    # ... and one -inf among finite candidates just has weight 0 and ranks last
    part = list(row)
    part[9] = -math.inf
    assert one_row(part, three, top_k=2)[2] == (1 << 5) | (1 << 20)
    assert one_row(part, three, top_p=0.999999)[2] == (1 << 5) | (1 << 20)
    # V = 64 with bit 63 allowed
    wide = [-200.0] * 64
    wide[63], wide[0], wide[31] = -0.5, -1.0, -1.5
    assert one_row(wide, ALL64, top_k=1)[:3] == (63, 0.0, 1 << 63)
    assert one_row(wide, ALL64, top_k=2)[2] == (1 << 63) | 1
    assert one_row(wide, ALL64, top_k=64)[2] == ALL64
    assert one_row(wide, (1 << 63) | (1 << 31), top_p=0.5)[2] == 1 << 63
    tok, logq, kept, score = one_row(wide, ALL64, top_k=3, top_p=0.99, score="confidence")
    want = D.draw_ex(np.array(wide, dtype=np.float32), 0.0, ALL64, 1.0, 3, 0.99)
    assert kept == want[2] == (1 << 63) | (1 << 31) | 1 and (kept >> tok) & 1
    assert abs(score - D.score(np.array(wide, dtype=np.float32), ALL64, 1.0, D.SCORE_CONFIDENCE)) <= R.logq_bound(score)
    assert one_row(wide, ALL64, inv_t=0.0, top_k=5, score="entropy")[0] == 63


# ---- scores ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inv_t", [1.0, 1.0 / 0.7, 0.5, 0.0], ids=["plain", "t0.7", "t2", "greedy"])
@pytest.mark.parametrize("kind,name", [(D.SCORE_CONFIDENCE, "confidence"), (D.SCORE_NEG_ENTROPY, "entropy")])
def test_scores_against_fp64(kind, name, inv_t):
    lp, chain, index, exclude = S.table()
    worst = 0.0
    for ex in (None, exclude):
        got = run_ex(lp, chain, index, inv_t=inv_t, exclude=ex, score=name, top_k=4, top_p=0.9)[3].numpy()
        assert got.dtype == np.float32
        for i in range(N_ROWS):
            want = D.score(lp[i], STANDARD, inv_t, kind, -1 if ex is None else int(ex[i]))  # greedy rows: inv_t = 1
            err = abs(float(got[i]) - want)
            worst = max(worst, err / R.logq_bound(want))
            assert err <= R.logq_bound(want), (i, float(got[i]), want)
        # the score is taken before filtering: the filter does not move it
        again = run_ex(lp, chain, index, inv_t=inv_t, exclude=ex, score=name)[3].numpy()
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32))
    print(f"{name} inv_t {inv_t:.3f}: worst error {worst:.3f} of the bound")


# ---- select_rows ------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 63, 0, 64, 65, 1022)


def scores_for(total, seed=0):
    """fp32 scores with many exact ties (one decimal), +-inf and NaN sprinkled in, -0.0 next to 0.0."""
    rng = np.random.default_rng(seed)
    s = np.round(rng.standard_normal(total) * 2.0, 1).astype(np.float32)
    k = rng.random(total)
    s[k < 0.04] = np.inf
    s[(k >= 0.04) & (k < 0.08)] = -np.inf
    s[(k >= 0.08) & (k < 0.14)] = np.nan
    s[(k >= 0.14) & (k < 0.17)] = -0.0
    return s


def offsets(counts):
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    return off


def run_select(scores, row_off, sel_off, rest_off, n_sel, n_rest):
    """The kernel on outputs prefilled with -7 (what it must leave alone), and the reference on the same."""
    sel = torch.full((n_sel,), -7, dtype=torch.int32).cuda()
    rest = torch.full((n_rest,), -7, dtype=torch.int32).cuda() if n_rest else None
    got = ops.select_rows(torch.from_numpy(scores).cuda(), i32(row_off), i32(sel_off), i32(rest_off) if n_rest else None,
                          sel_out=sel, rest_out=rest)
    want = D.select(scores, row_off, sel_off, rest_off if n_rest else None, [-7] * n_sel, [-7] * n_rest)
    return (got[0].cpu().tolist(), got[1].cpu().tolist() if n_rest else []), want


@pytest.mark.parametrize("per_step", [1, 3, 64, 100])
def test_select_rows_is_the_reference(per_step):
    row_off = offsets(LENGTHS)
    scores = scores_for(row_off[-1], seed=per_step)
    sel_off = offsets([per_step] * len(LENGTHS))  # more than a short chain has: k is clamped, the slice's tail stays
    rest_off = offsets([max(n - per_step, 0) for n in LENGTHS])
    got, want = run_select(scores, row_off, sel_off, rest_off, sel_off[-1], rest_off[-1])
    assert got[0] == want[0] and got[1] == want[1]
    assert -7 in got[0] and -7 not in got[1]
    for c, n in enumerate(LENGTHS):  # every chain's rows are its selection plus its rest, each once
        mine = got[0][sel_off[c]: sel_off[c] + min(per_step, n)] + got[1][rest_off[c]: rest_off[c + 1]]
        assert sorted(mine) == list(range(row_off[c], row_off[c + 1]))
    # the chains in another order, and each chain alone: the same slices (as indices inside the chain)
    inside = [([i - row_off[c] for i in got[0][sel_off[c]: sel_off[c] + min(per_step, n)]],
               [i - row_off[c] for i in got[1][rest_off[c]: rest_off[c + 1]]]) for c, n in enumerate(LENGTHS)]
    order = [6, 2, 0, 5, 3, 1, 4]
    lens = [LENGTHS[c] for c in order]
    ro, so, eo = offsets(lens), offsets([per_step] * len(lens)), offsets([max(n - per_step, 0) for n in lens])
    moved = np.concatenate([scores[row_off[c]: row_off[c + 1]] for c in order])
    again, _ = run_select(moved, ro, so, eo, so[-1], eo[-1])
    for j, c in enumerate(order):
        n = LENGTHS[c]
        assert [i - ro[j] for i in again[0][so[j]: so[j] + min(per_step, n)]] == inside[c][0], c
        assert [i - ro[j] for i in again[1][eo[j]: eo[j + 1]]] == inside[c][1], c
    for c, n in enumerate(LENGTHS):
        if n == 0:
            continue
        alone, _ = run_select(np.ascontiguousarray(scores[row_off[c]: row_off[c + 1]]), [0, n], [0, per_step],
                              [0, max(n - per_step, 0)], per_step, max(n - per_step, 0))
        assert alone[0][: min(per_step, n)] == inside[c][0] and alone[1] == inside[c][1], c


def test_select_rows_device_data_rules():
    """Offsets are device data: row offsets clamped to [0, n], a descending pair is an empty list, k clamped to the chain,
    the rest list cut to its slice, nothing written outside [0, n_sel) / [0, n_rest) or outside the slices."""
    scores = scores_for(40, seed=9)
    cases = [
        ([-3, 12, 5, 400], [0, 4, 8, 12], [0, 8, 8, 40], 12, 40),  # clamped; [12, 5) is empty; the third chain is rows 5 .. 39
        ([0, 20, 40], [0, 30, 60], [0, 0, 0], 60, 1),  # k beyond the chain; rest slices of length 0
        ([0, 20, 40], [3, 1, 6], [0, 5, 9], 8, 9),  # a descending sel pair: k = 0, the chain goes to the rest list, cut to 5
        ([0, 20, 40], [5, 9, 13], [30, 46, 62], 9, 40),  # slices that run past the outputs: the writes stop at their end
        ([0, 20, 40], [-2, 2, 6], [-3, 13, 29], 6, 29),  # ... and in front of them
        ([10, 10, 30], [0, 2, 4], [0, 0, 18], 4, 18),
    ]
    for row_off, sel_off, rest_off, n_sel, n_rest in cases:
        got, want = run_select(scores, row_off, sel_off, rest_off, n_sel, n_rest)
        assert got[0] == want[0] and got[1] == want[1], (row_off, sel_off, rest_off)
    # no rest list at all
    got = ops.select_rows(torch.from_numpy(scores).cuda(), i32([0, 20, 40]), i32([0, 3, 6]), n_sel=6)
    assert got[1] is None and got[0].cpu().tolist() == D.select(scores, [0, 20, 40], [0, 3, 6], None, [-1] * 6)[0]
    # all scores equal, all NaN: the lower rows first
    for value in (0.25, float("nan")):
        flat = np.full(300, value, dtype=np.float32)
        got, _ = run_select(flat, [0, 300], [0, 7], [0, 293], 7, 293)
        assert got[0] == list(range(7)) and got[1] == list(range(7, 300))


def test_select_rows_many_chains():
    many = 300  # more chains than one workgroup has lanes
    scores = scores_for(5 * many, seed=4)
    row_off = offsets([5] * many)
    for k in (1, 2, 5):
        sel_off, rest_off = offsets([k] * many), offsets([5 - k] * many)
        got, want = run_select(scores, row_off, sel_off, rest_off, sel_off[-1], rest_off[-1])
        assert got[0] == want[0] and got[1] == want[1]
        assert sorted(got[0] + got[1]) == list(range(5 * many))
