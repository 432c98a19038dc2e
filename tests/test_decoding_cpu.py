"""The host side of filtered and confidence-ordered decoding without a GPU: the numpy references of tests/_decoding_ref.py
against answers worked out by hand, the argument checks of the two new C entries (refused before any HIP call, on fake
pointers as in tests/test_sampling_cpu.py), the offset tables of the ordered loop, the new refusals of the Python layer and
the three new flags of the command line."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _decoding_ref as D
import esm
from esm_amd import _native as N
from esm_amd import ops, sample, sampling

FAKE = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused first
ROW = np.log(np.array([0.1, 0.2, 0.3, 0.4], dtype=np.float32))  # weights 0.25, 0.5, 0.75, 1 of the maximum; W = 2.5


def err():
    return N.lib.esmk_last_error().decode()


# ---- the references ---------------------------------------------------------------------------------------------------------
def test_keep_set_known_answers():
    # ranks 3, 2, 1, 0 hold E = 0, 1, 1.75, 2.25
    assert D.keep_set(ROW, 0b1111, 1.0) == (0b1111, True)  # both filters off: every candidate
    assert D.keep_set(ROW, 0b1111, 1.0, top_p=0.5) == (0b1100, True)  # E < 1.25
    assert D.keep_set(ROW, 0b1111, 1.0, top_p=0.8) == (0b1110, True)  # E < 2.0
    assert D.keep_set(ROW, 0b1111, 1.0, top_p=0.01) == (0b1000, True)  # the best candidate always stays
    assert D.keep_set(ROW, 0b1111, 1.0, top_k=1) == (0b1000, True)
    assert D.keep_set(ROW, 0b1111, 1.0, top_k=3, top_p=0.5) == (0b1100, True)
    assert D.keep_set(ROW, 0b1111, 1.0, top_k=2, top_p=0.8) == (0b1100, True)
    assert D.keep_set(ROW, 0b1111, 1.0, top_k=10) == (0b1111, True)  # more than there are candidates
    assert D.keep_set(ROW, 0b1111, 1.0, top_k=1, exclude=3) == (0b0100, True)
    assert D.keep_set(ROW, 0b0111, 1.0, top_k=2) == (0b0110, True)
    assert D.keep_set(ROW, 0, 1.0, top_k=2) == (0, True)
    # a sharper distribution keeps less: weights p^2 / 0.16 = 1, 0.5625, 0.25, 0.0625, W = 1.875, E = 0, 1, 1.5625, 1.8125
    assert D.keep_set(ROW, 0b1111, 2.0, top_p=0.8) == (0b1100, True)  # E < 1.5
    # greedy counts as inverse temperature 1
    assert D.keep_set(ROW, 0b1111, 0.0, top_p=0.8) == (0b1110, True)
    # equal values: the lower token ranks first; NaN ranks last
    tie = np.array([-1.0, -0.5, -0.5, -2.0], dtype=np.float32)
    assert D.keep_set(tie, 0b1111, 1.0, top_k=1)[0] == 0b0010 and D.keep_set(tie, 0b1111, 1.0, top_k=2)[0] == 0b0110
    assert D.ranked(tie, [0, 1, 2, 3]) == [1, 2, 0, 3]
    assert D.ranked(np.array([np.nan, -1.0, -np.inf, np.nan, -2.0], dtype=np.float32), [0, 1, 2, 3, 4]) == [1, 4, 2, 0, 3]
    assert D.keep_set(np.array([np.nan, -1.0, -2.0], dtype=np.float32), 0b111, 1.0, top_k=2)[0] == 0b110
    # a boundary that sits on the threshold is undecided: E_1 = 1 = 0.5 * 2
    assert D.keep_set(np.log(np.array([0.5, 0.5], dtype=np.float32)), 0b11, 1.0, top_p=0.5)[1] is False


def test_draw_ex_known_answers():
    # kept {2, 3}: weights 0.75, 1 -> cumulative 0.75, 1.75 of 1.75
    tok, logq, kept, decided = D.draw_ex(ROW, 0.2, 0b1111, 1.0, top_p=0.5)
    assert (tok, kept, decided) == (2, 0b1100, True) and abs(logq - math.log(3.0 / 7.0)) < 1e-6
    tok, logq, kept, _ = D.draw_ex(ROW, 0.5, 0b1111, 1.0, top_p=0.5)
    assert (tok, kept) == (3, 0b1100) and abs(logq - math.log(4.0 / 7.0)) < 1e-6
    assert D.draw_ex(ROW, 0.0, 0b1111, 1.0, top_k=1)[:3] == (3, 0.0, 0b1000)
    assert D.draw_ex(ROW, 0.99, 0b1111, 0.0, top_k=2)[:3] == (3, 0.0, 0b1100)  # greedy: the argmax, whatever the filter
    assert D.draw_ex(ROW, 0.5, 0b1000, 1.0, top_k=3, exclude=3) == (-1, 0.0, 0, True)
    # filters off: the draw of tests/_sampling_ref.py
    import _sampling_ref as R

    for u in (0.0, 0.05, 0.2, 0.5, 0.95):
        assert D.draw_ex(ROW, u, 0b1111, 1.0)[:2] == R.draw(ROW, u, 0b1111, 1.0)[:2]


def test_score_known_answers():
    assert abs(D.score(ROW, 0b1111, 1.0, D.SCORE_CONFIDENCE) - math.log(0.4)) < 1e-6
    assert abs(D.score(ROW, 0b0110, 1.0, D.SCORE_CONFIDENCE) - math.log(0.6)) < 1e-6  # over the candidates only
    assert abs(D.score(ROW, 0b1111, 2.0, D.SCORE_CONFIDENCE) - math.log(16.0 / 30.0)) < 1e-6
    assert abs(D.score(ROW, 0b1111, 0.0, D.SCORE_CONFIDENCE) - math.log(0.4)) < 1e-6  # greedy: inverse temperature 1
    assert abs(D.score(ROW, 0b1111, 1.0, D.SCORE_CONFIDENCE, exclude=3) - math.log(0.5)) < 1e-6
    want = sum(p * math.log(p) for p in (0.1, 0.2, 0.3, 0.4))
    assert abs(D.score(ROW, 0b1111, 1.0, D.SCORE_NEG_ENTROPY) - want) < 1e-6
    flat = np.full(8, -3.0, dtype=np.float32)
    assert abs(D.score(flat, 0xFF, 1.0, D.SCORE_NEG_ENTROPY) + math.log(8.0)) < 1e-12
    assert abs(D.score(flat, 0x0F, 0.5, D.SCORE_NEG_ENTROPY) + math.log(4.0)) < 1e-12
    one = np.array([0.0, -np.inf, -1000.0], dtype=np.float32)  # q = 1, 0, 0: the empty terms count as 0
    assert D.score(one, 0b111, 1.0, D.SCORE_NEG_ENTROPY) == 0.0 and D.score(one, 0b111, 1.0, D.SCORE_CONFIDENCE) == 0.0
    assert D.score(ROW, 0b0100, 1.0, D.SCORE_NEG_ENTROPY) == 0.0  # a single candidate
    assert D.score(ROW, 0, 1.0, D.SCORE_CONFIDENCE) == -math.inf and D.score(ROW, 0b1000, 1.0, D.SCORE_NEG_ENTROPY, exclude=3) == -math.inf


def test_select_known_answers():
    nan, inf = float("nan"), float("inf")
    s = [0.5, nan, 0.5, inf, -inf, 1.0]
    assert D.best_first(s, 0, 6) == [3, 5, 0, 2, 4, 1]  # ties to the lower row, NaN below -inf
    assert D.best_first([nan, nan, -inf], 0, 3) == [2, 0, 1]
    assert D.select(s, [0, 6], [0, 3], [0, 3], [-1] * 3, [-1] * 3) == ([3, 5, 0], [1, 2, 4])
    assert D.select(s, [0, 6], [0, 0], [0, 6], [-1], [-1] * 6) == ([-1], [0, 1, 2, 3, 4, 5])
    assert D.select(s, [0, 6], [0, 9], [0, 2], [-1] * 9, [-1] * 2) == ([3, 5, 0, 2, 4, 1, -1, -1, -1], [-1, -1])  # k clamped
    assert D.select(s, [0, 6], [0, 1], [0, 2], [-1], [-1] * 2) == ([3], [0, 1])  # no more than the rest slice holds
    # two chains and an empty one between them; slices may lie anywhere in the outputs
    sel, rest = D.select(s, [0, 2, 2, 6], [4, 5, 5, 7], [0, 1, 1, 3], [-1] * 8, [-1] * 4)
    assert sel == [-1, -1, -1, -1, 0, 3, 5, -1] and rest == [1, 2, 4, -1]
    # offsets are clamped to [0, n]; a descending pair is an empty list (the third chain is rows 1 .. 5)
    assert D.select(s, [-3, 2, 1, 40], [0, 1, 2, 3], [0, 1, 2, 7], [-1] * 3, [-1] * 7) == ([0, -1, 3], [1, -1, 1, 2, 4, 5, -1])
    assert D.select(s, [0, 6], [0, 2], None, [-1] * 2) == ([3, 5], [])


# ---- the C entries refuse bad arguments before any HIP call -----------------------------------------------------------------
def test_decoding_op_argument_checks():
    draw, select = N.lib.esmk_op_sample_rows_ex, N.lib.esmk_op_select_rows

    def d(lp=FAKE, chain=FAKE, index=FAKE, exclude=None, mask=0xFFFFF0, inv_t=1.0, seed=1, step=0, top_k=0, top_p=1.0, kind=0,
          tok=FAKE, logq=FAKE, u=None, score=None, kept=None, n=4, V=33):
        return draw(lp, chain, index, exclude, mask, inv_t, seed, step, top_k, top_p, kind, tok, logq, u, score, kept, n, V, None)

    for kw in (dict(lp=None), dict(chain=None), dict(index=None), dict(tok=None), dict(logq=None)):
        assert d(**kw) != 0 and err() == "esmk_op_sample_rows_ex: null argument", kw
    for kw in (dict(n=0), dict(n=-2), dict(n=2 ** 24 + 1)):
        assert d(**kw) != 0 and "esmk_op_sample_rows_ex: n must be" in err(), kw
    for kw in (dict(V=0), dict(V=65), dict(V=-1)):
        assert d(**kw) != 0 and "esmk_op_sample_rows_ex: V must be in 1 .. 64" in err(), kw
    for kw in (dict(inv_t=-1.0), dict(inv_t=float("nan")), dict(inv_t=float("inf"))):
        assert d(**kw) != 0 and "esmk_op_sample_rows_ex: inv_temperature" in err(), kw
    assert d(step=-1) != 0 and "esmk_op_sample_rows_ex: step" in err()
    for kw in (dict(top_k=-1), dict(top_k=65), dict(top_k=2 ** 31 - 1)):
        assert d(**kw) != 0 and "esmk_op_sample_rows_ex: top_k must be in 0 .. 64" in err(), kw
    for kw in (dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.0000001), dict(top_p=float("nan")), dict(top_p=float("inf")),
               dict(top_p=float("-inf"))):
        assert d(**kw) != 0 and "esmk_op_sample_rows_ex: top_p must be in (0, 1]" in err(), kw
    for kw in (dict(kind=-1), dict(kind=3)):
        assert d(**kw) != 0 and "esmk_op_sample_rows_ex: score_kind must be" in err(), kw
    for kind in (1, 2):
        assert d(kind=kind, score=None) != 0 and "needs score_out_dev" in err()

    def s(score=FAKE, row_off=FAKE, sel_off=FAKE, rest_off=FAKE, sel=FAKE, rest=FAKE, n_chain=3, n=9, n_sel=4, n_rest=5):
        return select(score, row_off, sel_off, rest_off, sel, rest, n_chain, n, n_sel, n_rest, None)

    for kw in (dict(score=None), dict(row_off=None), dict(sel_off=None), dict(sel=None)):
        assert s(**kw) != 0 and err() == "esmk_op_select_rows: null argument", kw
    for kw in (dict(n_chain=0), dict(n=0), dict(n_sel=0), dict(n_chain=-1), dict(n=-5), dict(n_sel=-1), dict(n_chain=2 ** 24 + 1),
               dict(n=2 ** 24 + 1), dict(n_sel=2 ** 24 + 1)):
        assert s(**kw) != 0 and "esmk_op_select_rows: n_chain, n and n_sel must be in 1 .. 2^24" in err(), kw
    for kw in (dict(n_rest=-1), dict(n_rest=2 ** 24 + 1)):
        assert s(**kw) != 0 and "esmk_op_select_rows: n_rest must be in 0 .. 2^24" in err(), kw
    for kw in (dict(rest=None), dict(rest_off=None)):
        assert s(**kw) != 0 and "esmk_op_select_rows: n_rest > 0 needs" in err(), kw


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def test_ordered_plan_tables():
    """Chains of 5, 2 and 0 holes at per_step 2: three steps; at step s a chain has n - 2 s rows left and commits min(2, left)."""
    ids = torch.tensor([10, 11, 12], dtype=torch.int32)
    plan = sampling._OrderedPlan([5, 2, 0], 2, ids, torch.device("cpu"))
    assert plan.n_steps == 3
    assert plan.steps == [(0, 2, 7, 4, 3), (3, 1, 3, 2, 1), (5, 1, 1, 1, 0)]
    assert plan.row_off.tolist() == [0, 5, 7, 0, 3, 0, 1]
    assert plan.sel_off.tolist() == [0, 2, 4, 0, 2, 0, 1]
    assert plan.rest_off.tolist() == [0, 3, 3, 0, 1, 0, 0]
    assert plan.src.tolist() == [0, 1, 0, 0] and plan.left.tolist() == [5, 2, 3, 1] and plan.chain.tolist() == [10, 11, 10, 10]
    for s, (o0, n_active, rows, sel, rest) in enumerate(plan.steps):
        assert plan.row_off[o0 + n_active] == rows and plan.left[o0 - s: o0 - s + n_active].sum() == rows
        assert plan.sel_off[o0 + n_active] == sel and plan.rest_off[o0 + n_active] == rest and sel + rest == rows
    assert [st[4] for st in plan.steps[:-1]] == [st[2] for st in plan.steps[1:]]  # a step's rest list is the next step's rows
    assert sampling._OrderedPlan([0, 0], 3, ids[:2], torch.device("cpu")).steps == []


def test_new_refusals_of_the_python_layer():
    model = esm.ESM2(1, 128, 2)  # on the CPU: a call that passes the argument checks is refused for that
    toks, holes = torch.tensor([[0, 5, 6, 2]]), torch.tensor([[0, 32, 6, 2]])
    for order in ("confidence", "entropy"):
        with pytest.raises(ValueError, match="only inpaint"):
            model.gibbs_sample(toks, 1, order=order)
    for order in ("best", "", None, "Confidence"):
        with pytest.raises(ValueError, match="order"):
            model.gibbs_sample(toks, 1, order=order)
        with pytest.raises(ValueError, match="order"):
            model.inpaint(holes, order=order)
    for call in (lambda **kw: model.gibbs_sample(toks, 1, **kw), lambda **kw: model.inpaint(holes, **kw),
                 lambda **kw: model.inpaint(holes, order="confidence", **kw)):
        for bad in (dict(top_k=-1), dict(top_k=65), dict(top_k=2.5), dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.5),
                    dict(top_p=float("nan")), dict(top_p=float("inf"))):
            with pytest.raises(ValueError, match="top_k|top_p"):
                call(**bad)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(top_k=5, top_p=0.9)
    assert ops.check_filters(0, 1.0) == (0, 1.0) and ops.check_filters(64, 1e-3) == (64, 1e-3) and ops.check_filters(3.0, 1) == (3, 1.0)
    lp = torch.zeros((2, 33))
    two = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_rows_ex(lp, two, two, 0xFFFFF0, top_k=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.select_rows(torch.zeros(2), two, two, n_sel=1)
    assert sampling.TRAJECTORY_FIELDS == ("chain", "step", "pos", "token", "logq", "u", "logprobs")


# ---- the command line -----------------------------------------------------------------------------------------------------------
def test_cli_parses_the_three_flags():
    base = ["--model-location", "m.pt", "--sequence", "MK_AY", "--output", "o.fasta"]
    a = sample.parse_args(base)
    assert (a.top_k, a.top_p, a.order) == (0, 1.0, "random")
    a = sample.parse_args(base + ["--mode", "inpaint", "--top-k", "5", "--top-p", "0.9", "--order", "confidence"])
    assert (a.mode, a.top_k, a.top_p, a.order) == ("inpaint", 5, 0.9, "confidence")
    a = sample.parse_args(base + ["--mode", "inpaint", "--order", "entropy"])
    assert a.order == "entropy" and (a.top_k, a.top_p) == (0, 1.0)
    a = sample.parse_args(base + ["--top-k", "64", "--top-p", "0.5", "--order", "random"])  # filters apply to gibbs as well
    assert (a.mode, a.top_k, a.top_p, a.order) == ("gibbs", 64, 0.5, "random")
    for bad in (["--order", "confidence"], ["--mode", "gibbs", "--order", "entropy"],  # refused with gibbs at parse time
                ["--mode", "inpaint", "--order", "best"], ["--top-k", "-1"], ["--top-k", "65"], ["--top-k", "2.5"],
                ["--top-p", "0"], ["--top-p", "1.5"], ["--top-p", "nan"], ["--top-p", "-0.2"]):
        with pytest.raises(SystemExit):
            sample.parse_args(base + bad)
