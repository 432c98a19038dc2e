"""The alignment ops one at a time against numpy, bit for bit (csrc/align.hip; tests/_align_ref.py): the two operand images, the
z-score enhancement, the affine-gap DP with its traceback bytes, and the walk — at the edges of the wavefront (63, 64, 65
rows or columns), of the lane strips and of the panel (``esmk_op_align_panel()``), with the columns behind every Lb holding NaN."""
import functools

import numpy as np
import pytest
import torch

import _align_ref as ref
from esm_amd import align as A
from esm_amd import ops

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


# ---- images -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [128, 96, 1280])
@pytest.mark.parametrize("similarity", ["cosine", "dot"])
def test_images(E, similarity):
    rng = np.random.default_rng(E)
    x = (rng.standard_normal((20, E)) * rng.uniform(0.01, 30, size=(20, 1))).astype(np.float32)
    x[7] = 0  # a zero row
    x[3, ::2] = 0
    rows = np.array([5, 7, 5, 19, 0, 7, 3, -1, 12, 5], dtype=np.int32)  # repeats, the zero row, a pad row
    u = ref.operand_rows(x, similarity)
    want_rows = np.where(rows[:, None] >= 0, u[np.maximum(rows, 0)], 0).astype(np.float32)
    xd, rd = torch.from_numpy(x).cuda(), torch.from_numpy(rows).cuda()
    Ep = (E + 63) // 64 * 64
    for b_side in (False, True):
        got = ops.align_rows(xd, rd, cosine=similarity == "cosine", b_side=b_side).cpu().numpy()
        assert got.shape == (len(rows), 3 * Ep)
        assert np.array_equal(bits(got), bits(ref.image(want_rows, b_side))), (E, similarity, b_side)
        if Ep > E:  # the pad columns of the last K tile are zero in all three parts
            assert not got.reshape(len(rows), Ep // 64, 3, 64)[:, -1, :, E - Ep:].any()
        whole = ops.align_rows(xd, None, cosine=similarity == "cosine", b_side=b_side).cpu().numpy()
        assert np.array_equal(bits(whole), bits(ref.image(u, b_side)))
    if similarity == "cosine":
        assert not want_rows[1].any() and not want_rows[7].any()


def test_b_image_is_the_weight_split():
    rng = np.random.default_rng(1)
    u = rng.standard_normal((64, 128)).astype(np.float32)
    ud = torch.from_numpy(u).cuda()
    w3 = torch.zeros((64, 3 * 128), dtype=torch.float16, device="cuda")
    ops.split_weight_ex(ud, w3, 128, 3)
    assert torch.equal(w3, ops.align_rows(ud, None, cosine=False, b_side=True))


# ---- enhancement --------------------------------------------------------------------------------------------------------
def test_enhance():
    rng = np.random.default_rng(2)
    shapes = [(1, 7), (7, 1), (33, 65), (5, 9), (300, 3)]
    rows, ld = sum(s[0] for s in shapes), 72
    S = rng.standard_normal((rows, ld)).astype(np.float32)
    a_off = np.concatenate([[0], np.cumsum([s[0] for s in shapes])])[:-1]
    S[a_off[3] + 2, :9] = 0.3  # a constant row: sigma = 0 (as in every row of 7 x 1 and every column of 1 x 7)
    table, _ = A.pair_table(a_off, [s[0] for s in shapes], [0] * len(shapes), [s[1] for s in shapes])
    want = S.copy()
    for k, (la, lb) in enumerate(shapes):
        want[a_off[k]:a_off[k] + la, :lb] = ref.enhance(S[a_off[k]:a_off[k] + la, :lb])
    assert np.isfinite(want).all()
    Sd = torch.from_numpy(S).cuda()
    ops.align_enhance(Sd, torch.from_numpy(table).cuda(), 65)
    got = Sd.cpu().numpy()
    assert np.array_equal(bits(got), bits(want))  # also: nothing outside the blocks has changed
    # one workgroup for all pairs (the smallest workspace) gives the same
    Sd = torch.from_numpy(S).cuda()
    ops.align_enhance(Sd, torch.from_numpy(table).cuda(), 65, ws=torch.empty(130, dtype=torch.float32, device="cuda"))
    assert np.array_equal(bits(Sd.cpu().numpy()), bits(want))


# ---- DP and traceback ---------------------------------------------------------------------------------------------------
def make_S(kind, La, Lb, seed):
    rng = np.random.default_rng(seed)
    if kind == "integer":  # many ties: every rule of precedence is exercised
        return rng.integers(-2, 3, size=(La, Lb)).astype(np.float32)
    if kind == "negative":
        return -rng.uniform(0.1, 1, size=(La, Lb)).astype(np.float32)
    return rng.uniform(-1, 1, size=(La, Lb)).astype(np.float32)


def run(S_list, mode, o, e, want_traceback=True):
    """the listed pairs in ONE launch of each kernel: per pair dict(score, end, tb [La, Lb], cols, n_match, start)"""
    la, lb = [s.shape[0] for s in S_list], [s.shape[1] for s in S_list]
    a_off = np.concatenate([[0], np.cumsum(la)])
    ld = (max(lb) + 7) // 8 * 8
    S = np.full((a_off[-1], ld), np.nan, dtype=np.float32)  # behind every Lb: NaN, which no result may depend on
    for k, s in enumerate(S_list):
        S[a_off[k]:a_off[k + 1], :lb[k]] = s
    table_np, tb_bytes = A.pair_table(a_off[:-1], la, [0] * len(la), lb)
    table = torch.from_numpy(table_np).cuda()
    Sd = torch.from_numpy(S).cuda()
    code = A.MODES[mode]
    tb = torch.full((tb_bytes,), 0xEE, dtype=torch.uint8, device="cuda") if want_traceback else None
    r = ops.align_dp(Sd, table, code, o, e, max(la), max(lb), want_traceback=want_traceback, tb=tb)
    score, end = r["score"].cpu().numpy(), r["end"].cpu().numpy()
    out = [dict(score=score[k], end=tuple(end[k])) for k in range(len(la))]
    if not want_traceback:
        assert "tb" not in r
        return out
    cap = np.array(la) + np.array(lb)
    slot = np.concatenate([[0], np.cumsum(cap)])
    cols = torch.full((int(slot[-1]), 2), -7, dtype=torch.int32, device="cuda")
    t = ops.align_traceback(table, code, r["end"], tb, torch.from_numpy(slot[:-1].copy()).cuda(), cols)
    tbh, colsh = tb.cpu().numpy(), cols.cpu().numpy()
    n_cols, n_match, start = (t[k].cpu().numpy() for k in ("n_cols", "n_match", "start"))
    for k in range(len(la)):
        ld16 = (lb[k] + 15) // 16 * 16
        m = tbh[table_np[k, 4]:table_np[k, 4] + la[k] * ld16].reshape(la[k], ld16)
        assert not m[:, lb[k]:(lb[k] + 7) // 8 * 8].any()  # the bytes behind Lb inside the last written strip are 0
        out[k].update(tb=m[:, :lb[k]].copy(), cols=colsh[slot[k + 1] - n_cols[k]:slot[k + 1]].copy(), n_match=int(n_match[k]),
                      start=tuple(start[k]))
        assert (colsh[slot[k]:slot[k + 1] - n_cols[k]] == -7).all()  # the front of the slot is untouched
    return out


def compare(got, S_list, mode, o, e, what=""):
    for k, S in enumerate(S_list):
        want = ref.align(S, mode, o, e)
        g = got[k]
        assert bits(np.float32(g["score"]).reshape(1))[0] == bits(np.float32(want["score"]).reshape(1))[0], (what, k, S.shape, g["score"], want["score"])
        assert g["end"] == want["end"], (what, k, S.shape)
        if "tb" in g:
            assert np.array_equal(g["tb"], want["tb"]), (what, k, S.shape, np.argwhere(g["tb"] != want["tb"])[:4])
            assert np.array_equal(g["cols"], want["cols"]), (what, k, S.shape)
            assert g["n_match"] == want["n_match"] and g["start"] == want["start"], (what, k, S.shape)


@functools.lru_cache(maxsize=None)
def size_list():
    return ref.sizes(ops.align_panel())


@functools.lru_cache(maxsize=None)
def matrices(kind):
    return [make_S(kind, La, Lb, 100 + k) for k, (La, Lb) in enumerate(size_list())]


@pytest.mark.parametrize("kind", ["random", "integer"])
@pytest.mark.parametrize("mode", ["global", "local"])
def test_dp_and_traceback_at_every_edge(mode, kind):
    P = ops.align_panel()
    assert (3, 2 * P + 3) in size_list() and (P + 1, 5) in size_list() and len(size_list()) == 44
    S_list = matrices(kind)
    o, e = (1.0, 0.125) if kind == "integer" else (1.0, 0.1)
    compare(run(S_list, mode, o, e), S_list, mode, o, e, f"{mode} {kind}")


SUBSET = [(1, 1), (2, 65), (65, 2), (64, 64), (129, 63), (5, "P+1"), ("P+1", 5), (3, "2P+3")]


def subset(kind, seed):
    P = ops.align_panel()
    val = lambda v: {"P+1": P + 1, "2P+3": 2 * P + 3}.get(v, v)
    return [make_S(kind, val(a), val(b), seed + k) for k, (a, b) in enumerate(SUBSET)]


@pytest.mark.parametrize("o,e", [(0.5, 0.5), (1.0, 0.0), (0.0, 0.0)], ids=["o=e", "e=0", "free"])
@pytest.mark.parametrize("mode", ["global", "local"])
def test_gap_penalty_edges(mode, o, e):
    for kind in ("random", "integer"):
        S_list = subset(kind, 300)
        compare(run(S_list, mode, o, e), S_list, mode, o, e, f"{mode} {kind} o={o} e={e}")


def test_all_negative_local_is_empty():
    S_list = subset("negative", 400)
    got = run(S_list, "local", 1.0, 0.1)
    for g in got:
        assert g["score"] == 0 and g["end"] == (0, 0) and g["start"] == (0, 0) and len(g["cols"]) == 0 and g["n_match"] == 0
        assert not (g["tb"] & 3).any()  # every cell stops
    compare(got, S_list, "local", 1.0, 0.1)


def planted():
    """+1 on a path with one 7-long gap on each side, -1 elsewhere: 40 x 40"""
    cols = [(k, k) for k in range(10)] + [(k, -1) for k in range(10, 17)] + [(17 + k, 10 + k) for k in range(10)]
    cols += [(-1, k) for k in range(20, 27)] + [(27 + k, 27 + k) for k in range(13)]
    S = -np.ones((40, 40), dtype=np.float32)
    for i, j in cols:
        if i >= 0 and j >= 0:
            S[i, j] = 1
    return S, np.array(cols, dtype=np.int32)


@pytest.mark.parametrize("mode", ["global", "local"])
def test_planted_path_is_recovered(mode):
    S, cols = planted()
    g = run([S], mode, 1.0, 0.1)[0]
    assert np.array_equal(g["cols"], cols)
    assert g["start"] == (0, 0) and g["end"] == (40, 40) and g["n_match"] == 33
    assert abs(float(g["score"]) - (33 - 2 * (1.0 + 6 * 0.1))) < 1e-4  # 33 matches, two gaps of 7
    compare([g], [S], mode, 1.0, 0.1)


def test_one_long_gap_beats_two_short_ones():
    # residues 3 .. 6 of a have no partner.  One gap of 4 costs o + 3 e = 1.75 and keeps six matches; with linear gaps (4 o) the
    # cheaper answer would be poor matches instead.  Splitting the gap in two costs 2 o + 2 e = 2.5.
    S = np.full((10, 6), -0.6, dtype=np.float32)
    for k in range(3):
        S[k, k] = 1
        S[k + 7, k + 3] = 1
    g = run([S], "global", 1.0, 0.25)[0]
    assert float(g["score"]) == 4.25 and g["n_match"] == 6
    assert [tuple(c) for c in g["cols"]] == [(0, 0), (1, 1), (2, 2), (3, -1), (4, -1), (5, -1), (6, -1), (7, 3), (8, 4), (9, 5)]
    assert (g["tb"][4:7, 2] & 8).all() and not g["tb"][3, 2] & 8  # the vertical gap opens in cell (4, 3), three extensions follow


@pytest.mark.parametrize("mode", ["global", "local"])
def test_launch_independence_and_score_only(mode):
    S_list = matrices("random")[:36] + [matrices("random")[k] for k in (37, 38, 39, 43)]  # 40 mixed pairs
    assert len(S_list) == 40
    together = run(S_list, mode, 1.0, 0.1)
    for k in (0, 17, 35, 37, 39):  # 1 x 1, 63 x 129, 129 x 129, 5 x P + 1, 2 P + 3 x 3
        alone = run([S_list[k]], mode, 1.0, 0.1)[0]
        assert bits(np.float32(alone["score"]).reshape(1))[0] == bits(np.float32(together[k]["score"]).reshape(1))[0]
        for key in ("end", "start", "n_match"):
            assert alone[key] == together[k][key], (k, key)
        assert np.array_equal(alone["tb"], together[k]["tb"]) and np.array_equal(alone["cols"], together[k]["cols"]), k
    scores = run(S_list, mode, 1.0, 0.1, want_traceback=False)
    for a, b in zip(scores, together):
        assert bits(np.float32(a["score"]).reshape(1))[0] == bits(np.float32(b["score"]).reshape(1))[0] and a["end"] == b["end"]


def test_few_wavefronts_take_many_pairs():
    """a workspace for two wavefronts only: 9 pairs with sides b beyond one panel go through them in turn"""
    P = ops.align_panel()
    S_list = [make_S("random", 4 + k, P + 1 + 9 * k, 500 + k) for k in range(9)]
    la, lb = [s.shape[0] for s in S_list], [s.shape[1] for s in S_list]
    a_off = np.concatenate([[0], np.cumsum(la)])
    S = np.zeros((a_off[-1], (max(lb) + 7) // 8 * 8), dtype=np.float32)
    for k, s in enumerate(S_list):
        S[a_off[k]:a_off[k + 1], :lb[k]] = s
    table_np, tb_bytes = A.pair_table(a_off[:-1], la, [0] * 9, lb)
    ws = torch.empty((2 * 2 * (max(la) + 1),), dtype=torch.float32, device="cuda")
    r = ops.align_dp(torch.from_numpy(S).cuda(), torch.from_numpy(table_np).cuda(), 0, 1.0, 0.1, max(la), max(lb),
                     want_traceback=False, ws=ws)
    score = r["score"].cpu().numpy()
    for k, s in enumerate(S_list):
        assert bits(score[k:k + 1])[0] == bits(np.float32(ref.align(s, "global", 1.0, 0.1)["score"]).reshape(1))[0], k
