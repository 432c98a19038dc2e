"""Free end gaps and several hits per pair, the ops one at a time against numpy, bit for bit (csrc/align.hip through
``ops.align_dp`` / ``ops.align_traceback``; tests/_align_free_ref.py): score bits, end, start, traceback bytes, columns and
n_match at the edges of the wavefront and of the panel, with NaN behind every Lb in S, 0xEE in the byte buffer and -7 in the
column slots; the Waterman-Eggert rounds against ``hits()``, and what they leave in S."""
import functools

import numpy as np
import pytest
import torch

import _align_free_ref as fr
import _align_ref as ref
from esm_amd import align as A
from esm_amd import ops

pytestmark = pytest.mark.gpu

NAMED = ["a", "b", "both"]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).reshape(-1).view(np.uint32)


def make_S(kind, La, Lb, seed):
    rng = np.random.default_rng(seed)
    if kind == "integer":  # many ties: every rule of precedence is exercised
        return rng.integers(-2, 3, size=(La, Lb)).astype(np.float32)
    if kind == "negative":
        return -rng.uniform(0.1, 1, size=(La, Lb)).astype(np.float32)
    return rng.uniform(-1, 1, size=(La, Lb)).astype(np.float32)


def run(S_list, mode, o, e, free_ends=0, K=1, ws=None, want_traceback=True):
    """The listed pairs in ONE launch of each kernel per round, K rounds on one S and one byte buffer, every round but the last
    masking: (per pair a list of K dicts(score, end, tb [La, Lb], cols, n_match, start), the pair blocks of S afterwards)."""
    la, lb = [s.shape[0] for s in S_list], [s.shape[1] for s in S_list]
    n = len(la)
    a_off = np.concatenate([[0], np.cumsum(la)])
    ld = (max(lb) + 7) // 8 * 8
    S = np.full((a_off[-1], ld), np.nan, dtype=np.float32)  # behind every Lb: NaN, which no result may depend on
    for k, s in enumerate(S_list):
        S[a_off[k]:a_off[k + 1], :lb[k]] = s
    table_np, tb_bytes = A.pair_table(a_off[:-1], la, [0] * n, lb)
    table = torch.from_numpy(table_np).cuda()
    Sd = torch.from_numpy(S).cuda()
    code = A.MODES[mode]
    mask = A.parse_free_ends(free_ends)
    tb = torch.full((tb_bytes,), 0xEE, dtype=torch.uint8, device="cuda") if want_traceback else None
    cap = np.repeat(np.array(la) + np.array(lb), K)  # slot (p, k)
    slot = np.concatenate([[0], np.cumsum(cap)])
    cols = torch.full((int(slot[-1]), 2), -7, dtype=torch.int32, device="cuda")
    out = [[] for _ in range(n)]
    for k in range(K):
        r = ops.align_dp(Sd, table, code, o, e, max(la), max(lb), want_traceback=want_traceback, tb=tb, ws=ws, free_ends=mask)
        score, end = r["score"].cpu().numpy(), r["end"].cpu().numpy()
        if not want_traceback:
            assert "tb" not in r
            for p in range(n):
                out[p].append(dict(score=score[p], end=tuple(int(v) for v in end[p])))
            continue
        sl = torch.from_numpy(slot[k:-1:K].copy()).cuda()
        t = ops.align_traceback(table, code, r["end"], tb, sl, cols, free_ends=mask, S_mask=Sd if k + 1 < K else None)
        tbh, colsh = tb.cpu().numpy(), cols.cpu().numpy()
        n_cols, n_match, start = (t[key].cpu().numpy() for key in ("n_cols", "n_match", "start"))
        for p in range(n):
            ld16 = (lb[p] + 15) // 16 * 16
            m = tbh[table_np[p, 4]:table_np[p, 4] + la[p] * ld16].reshape(la[p], ld16)
            assert not m[:, lb[p]:(lb[p] + 7) // 8 * 8].any()  # the bytes behind Lb inside the last written strip are 0
            s0, s1 = slot[p * K + k], slot[p * K + k + 1]
            assert (colsh[s0:s1 - n_cols[p]] == -7).all()  # the front of the slot is untouched
            out[p].append(dict(score=score[p], end=tuple(int(v) for v in end[p]), tb=m[:, :lb[p]].copy(),
                               cols=colsh[s1 - n_cols[p]:s1].copy(), n_match=int(n_match[p]), start=tuple(int(v) for v in start[p])))
    after = Sd.cpu().numpy()
    assert np.array_equal(np.isnan(after), np.isnan(S))  # the NaN stand where they stood: nothing outside a block is written
    return out, [after[a_off[k]:a_off[k + 1], :lb[k]] for k in range(n)]


def same(g, want, what):
    assert bits(g["score"])[0] == bits(want["score"])[0], (what, g["score"], want["score"])
    assert g["end"] == want["end"], (what, g["end"], want["end"])
    if "tb" in g:
        assert np.array_equal(g["tb"], want["tb"]), (what, np.argwhere(g["tb"] != want["tb"])[:4])
        assert np.array_equal(g["cols"], want["cols"]), what
        assert g["n_match"] == want["n_match"] and g["start"] == want["start"], (what, g["start"], want["start"])


@functools.lru_cache(maxsize=None)
def size_list():
    return tuple(ref.sizes(ops.align_panel()))


@functools.lru_cache(maxsize=None)
def matrices(kind):
    return [make_S(kind, La, Lb, 100 + k) for k, (La, Lb) in enumerate(size_list())]


SUBSET = [(1, 1), (2, 65), (65, 2), (64, 64), (129, 63), (5, "P+1"), ("P+1", 5), (3, "2P+3")]


@functools.lru_cache(maxsize=None)
def subset(kind, seed):
    P = ops.align_panel()
    val = lambda v: {"P+1": P + 1, "2P+3": 2 * P + 3}.get(v, v)
    return [make_S(kind, val(a), val(b), seed + k) for k, (a, b) in enumerate(SUBSET)]


@functools.lru_cache(maxsize=None)
def want_all(kind, mask, o, e):
    """the reference on the 44 shapes, computed once per (kind, mask)"""
    return [fr.align(S, "global", o, e, mask) for S in matrices(kind)]


@functools.lru_cache(maxsize=None)
def want_subset(kind, seed, mode, mask, o, e, K):
    return [fr.hits(S, K, mode, o, e, mask) for S in subset(kind, seed)]


# ---- free ends ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "integer"])
@pytest.mark.parametrize("name", NAMED)
def test_named_masks_at_every_edge(name, kind):
    assert len(size_list()) == 44
    o, e = (1.0, 0.125) if kind == "integer" else (1.0, 0.1)
    got, _ = run(matrices(kind), "global", o, e, name)
    for k, want in enumerate(want_all(kind, A.parse_free_ends(name), o, e)):
        same(got[k][0], want, (name, kind, size_list()[k]))


@pytest.mark.parametrize("mask", range(1, 16))
def test_every_mask_on_integer_matrices(mask):
    got, _ = run(subset("integer", 300), "global", 1.0, 0.125, mask)
    for k, (want, _) in enumerate(want_subset("integer", 300, "global", mask, 1.0, 0.125, 1)):
        same(got[k][0], want[0], (mask, SUBSET[k]))


def test_mask_zero_through_the_ex_entries_is_global_mode():
    S_list = subset("integer", 300)
    got, _ = run(S_list, "global", 1.0, 0.125, 0)
    for k, S in enumerate(S_list):
        same(got[k][0], ref.align(S, "global", 1.0, 0.125), SUBSET[k])


@pytest.mark.parametrize("o,e", [(0.5, 0.5), (1.0, 0.0), (0.0, 0.0)], ids=["o=e", "e=0", "free"])
@pytest.mark.parametrize("name", NAMED)
def test_gap_penalty_edges(name, o, e):
    mask = A.parse_free_ends(name)
    for kind in ("random", "integer"):
        got, _ = run(subset(kind, 300), "global", o, e, mask)
        for k, (want, _) in enumerate(want_subset(kind, 300, "global", mask, o, e, 1)):
            same(got[k][0], want[0], (name, kind, o, e, SUBSET[k]))


def test_all_negative_ends_in_a_cell_with_i_and_j_at_least_one():
    got, _ = run(subset("negative", 400), "global", 1.0, 0.1, "both")
    for k, (want, _) in enumerate(want_subset("negative", 400, "global", 15, 1.0, 0.1, 1)):
        g = got[k][0]
        assert g["end"][0] >= 1 and g["end"][1] >= 1 and float(g["score"]) < 0
        same(g, want[0], SUBSET[k])


def planted(La, Lb, at):
    S = -np.ones((La, Lb), dtype=np.float32)
    for c in at:
        S[np.arange(La), c + np.arange(La)] = 1
    return S


def test_planted_domain_inside_a_longer_target():
    S = planted(12, 60, [20])
    g = run([S], "global", 1.0, 0.1, "b")[0][0][0]
    assert g["start"] == (0, 20) and g["end"] == (12, 32) and g["n_match"] == 12 and float(g["score"]) == 12.0
    assert np.array_equal(g["cols"], np.stack([np.arange(12), 20 + np.arange(12)], 1))  # no gap column
    same(g, fr.align(S, "global", 1.0, 0.1, 12), "planted b")
    plain = run([S], "global", 1.0, 0.1, 0)[0][0][0]
    assert (plain["cols"] < 0).any() and plain["start"] == (0, 0) and plain["end"] == (12, 60)  # global mode pays for the flanks
    assert float(plain["score"]) < 12.0


@pytest.mark.parametrize("name", NAMED)
def test_launch_independence_and_score_only(name):
    S_list = matrices("random")[:36] + [matrices("random")[k] for k in (37, 38, 39, 43)]  # 40 mixed pairs
    assert len(S_list) == 40
    together, _ = run(S_list, "global", 1.0, 0.1, name)
    for k in (0, 17, 35, 37, 39):  # 1 x 1, 63 x 129, 129 x 129, 5 x P + 1, 2 P + 3 x 3
        alone, _ = run([S_list[k]], "global", 1.0, 0.1, name)
        same(alone[0][0], together[k][0], (name, k))
    scores, _ = run(S_list, "global", 1.0, 0.1, name, want_traceback=False)
    for a, b in zip(scores, together):
        assert bits(a[0]["score"])[0] == bits(b[0]["score"])[0] and a[0]["end"] == b[0]["end"]


def test_few_wavefronts_take_many_pairs():
    """a workspace for two wavefronts only: 9 pairs with sides b beyond one panel go through them in turn, the running best of
    row La kept across the panels"""
    P = ops.align_panel()
    S_list = [make_S("random", 4 + k, P + 1 + 9 * k, 500 + k) for k in range(9)]
    ws = torch.empty((2 * 2 * (max(s.shape[0] for s in S_list) + 1),), dtype=torch.float32, device="cuda")
    got, _ = run(S_list, "global", 1.0, 0.1, "b", ws=ws)
    for k, S in enumerate(S_list):
        same(got[k][0], fr.align(S, "global", 1.0, 0.1, 12), k)


# ---- several hits -------------------------------------------------------------------------------------------------------
HIT_MODES = [("local", 0), ("global", 12), ("global", 15)]


def check_hits(got, S_after, S_list, want_list, K, what):
    for p, S in enumerate(S_list):
        want, _ = want_list[p]
        cells = set()
        masked = np.zeros(S.shape, dtype=bool)
        for k in range(K):
            g = got[p][k]
            same(g, want[k], (what, p, k, S.shape))
            assert not np.isnan(g["score"])
            if k:
                assert float(g["score"]) <= float(got[p][k - 1]["score"]), (what, p, k)  # non-increasing
            m = g["cols"][(g["cols"][:, 0] >= 0) & (g["cols"][:, 1] >= 0)]
            mine = {(int(i), int(j)) for i, j in m}
            assert len(mine) == g["n_match"] and not (mine & cells), (what, p, k)  # the hits' match cells are disjoint
            cells |= mine
            if k + 1 < K:
                masked[m[:, 0], m[:, 1]] = True
        # S differs from the input at the match cells of the hits 0 .. K - 2 only, where it is -inf
        assert np.array_equal(bits(S_after[p][~masked]), bits(S[~masked])), (what, p)
        assert np.isneginf(S_after[p][masked]).all(), (what, p)


@pytest.mark.parametrize("K", [3, 1])
@pytest.mark.parametrize("mode,mask", HIT_MODES, ids=["local", "b", "both"])
def test_hits_against_the_reference(mode, mask, K):
    for kind, o, e in (("random", 1.0, 0.1), ("integer", 1.0, 0.125)):
        S_list = subset(kind, 300)
        got, after = run(S_list, mode, o, e, mask, K=K)
        check_hits(got, after, S_list, want_subset(kind, 300, mode, mask, o, e, K), K, (mode, mask, kind))


@pytest.mark.parametrize("K", [3, 1])
@pytest.mark.parametrize("mode,mask", HIT_MODES, ids=["local", "b", "both"])
def test_three_planted_copies_come_back_in_column_order(mode, mask, K):
    S = planted(16, 100, [5, 40, 75])
    got, after = run([S], mode, 1.0, 0.1, mask, K=K)
    check_hits(got, after, [S], [fr.hits(S, K, mode, 1.0, 0.1, mask)], K, (mode, mask, "planted"))
    if mask != 15:  # equal scores: the tie goes to the lower column, so the copies are found left to right
        for k, c in enumerate([5, 40, 75][:K]):
            g = got[0][k]
            assert bits(g["score"])[0] == bits(np.float32(16))[0] and g["start"] == (0, c) and g["end"] == (16, c + 16), (k, g)
            assert g["n_match"] == 16 and len(g["cols"]) == 16


@pytest.mark.parametrize("mode,mask", HIT_MODES, ids=["local", "b", "both"])
def test_a_pair_whose_paths_run_out(mode, mask):
    S = np.ones((1, 1), dtype=np.float32)
    got, after = run([S], mode, 1.0, 0.1, mask, K=3)
    want = fr.hits(S, 3, mode, 1.0, 0.1, mask)
    check_hits(got, after, [S], [want], 3, (mode, mask, "1 x 1"))
    assert got[0][0]["n_match"] == 1 and float(got[0][0]["score"]) == 1.0
    for k in (1, 2):  # no match is left: not a valid hit, and no NaN
        g = got[0][k]
        assert g["n_match"] == 0 and (np.isfinite(g["score"]) or np.isneginf(g["score"])) and float(g["score"]) <= 0
