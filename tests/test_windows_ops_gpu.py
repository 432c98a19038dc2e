"""The three window kernels alone (csrc/windows.hip through esm_amd.ops) against the plain restatement of their contracts in
tests/_windows_ref.py: ``window_rows`` by exact integer equality, ``blend_rows`` bit for bit where a list has one entry or none
and within (K + 2) 2^-23 max_k |x_k| per element of the fp64 blend otherwise (the gamma bound of a K-term fp32 accumulation plus
one division with positive weights, doubled), ``stitch_contacts`` bit for bit with NaN exactly where no window holds the pair."""
import numpy as np
import pytest
import torch

import _windows_ref as ref
from esm_amd import ops

pytestmark = pytest.mark.gpu
MASK, CLS, EOS = 32, 0, 2
I32_MAX = 2 ** 31 - 1


def dev32(values):
    return torch.tensor(values, dtype=torch.int32).cuda()


@pytest.mark.parametrize("wrapped", [True, False], ids=["wrapped", "raw"])
@pytest.mark.parametrize("n", [1, 3, 130])
@pytest.mark.parametrize("Tw", [3, 8, 1024])
def test_window_rows(Tw, n, wrapped):
    B, T = 3, Tw + 77
    g = torch.Generator().manual_seed(100 * Tw + n)
    tokens = torch.randint(4, 30, (B, T), generator=g)
    head, tail = (CLS, EOS) if wrapped else (-1, -1)
    h = 1 if wrapped else 0
    R = Tw - 2 * h
    src = torch.randint(0, B, (n,), generator=g).tolist()
    start = torch.randint(h, T - R + 1, (n,), generator=g).tolist()
    # copies with a source row or a start the host never checked: clamped, no fault
    for i, (b, s) in enumerate([(-2, 5), (B + 4, -7), (1, T + 9), (0, -I32_MAX - 1), (2, I32_MAX)]):
        if 5 + i < n:
            src[5 + i], start[5 + i] = b, s
    if n == 3:
        src[1], start[2] = -1, T - 2  # the window runs over the end of the row: the last token repeats
    off, pos = [0], []
    for i, s in enumerate(start):
        kind = i % 6
        if kind == 1:
            pos += [s, s + R - 1]  # the first and the last body column
        elif kind == 2:
            pos += [s - 1, s + R]  # the overridden columns of a wrapped copy, the tokens next to a raw one: nothing
        elif kind == 3:
            pos += [s - 100, s + Tw + 50, I32_MAX, -I32_MAX - 1, min(s, 0) - 1]  # outside the copy: nothing
        elif kind == 4:
            pos += [s + R // 2] * 3  # repeated
        elif kind == 5:
            pos += [s + k for k in range(0, R, 3)]
        off.append(len(pos))  # kind 0: an empty list
    pos = [min(max(p, -I32_MAX - 1), I32_MAX) for p in pos]
    got = ops.window_rows(tokens.cuda(), dev32(src), dev32(start), dev32(off), dev32(pos), Tw, head, tail, MASK)
    want = ref.window_rows_ref(tokens.tolist(), src, start, off, pos, Tw, head, tail, MASK)
    assert got.dtype == torch.int64 and tuple(got.shape) == (n, Tw)
    assert got.cpu().tolist() == want
    if n > 1 and Tw > 3:
        assert want[1].count(MASK) == 2 and (want[1][h], want[1][Tw - 1 - h]) == (MASK, MASK)
    if wrapped:
        assert all(row[0] == CLS and row[-1] == EOS for row in want)
    if n > 2:
        base = ref.window_rows_ref(tokens.tolist(), src[2:3], start[2:3], [0, 0], [], Tw, head, tail, MASK)
        assert want[2] == base[0]  # masks on the overridden columns or next to the copy changed nothing


def test_window_rows_offsets_are_clamped():
    tokens = torch.arange(4, 4 + 40).view(2, 20)
    pos = [3, 4, 5, 6]
    for off in ([0, 2, 4], [-5, 2, 99], [3, 1, 4], [4, 4, 0]):  # in range; clamped to [0, total]; a descending pair is empty
        got = ops.window_rows(tokens.cuda(), dev32([0, 1]), dev32([2, 3]), dev32(off), dev32(pos), 6, -1, -1, MASK)
        assert got.cpu().tolist() == ref.window_rows_ref(tokens.tolist(), [0, 1], [2, 3], off, pos, 6, -1, -1, MASK), off
    none = torch.zeros((0,), dtype=torch.int32).cuda()
    got = ops.window_rows(tokens.cuda(), dev32([1]), dev32([1]), dev32([0, 0]), none, 5, CLS, -1, MASK)
    assert got.cpu().tolist() == [[CLS] + tokens[1, 1:5].tolist()]  # the ESM-1 alphabet: <cls>, no <eos>


LIST_LENGTHS = [0, 1, 2, 4, 1, 4, 2, 0, 4, 1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("E", [4, 132, 1280])
def test_blend_rows(E, dtype):
    N = 37
    g = torch.Generator().manual_seed(E)
    x = (torch.randn((N, E), generator=g) * 3).to(dtype)
    off, src, w = [0], [], []
    for r, K in enumerate(LIST_LENGTHS):
        src += torch.randint(0, N, (K,), generator=g).tolist()
        # the triangular weights of a blend (integers), and positive weights of no special form
        w += [float(min(j + 1, K - j)) for j in range(K)] if r % 2 else (torch.rand((K,), generator=g) * 3 + 0.05).tolist()
        off.append(len(src))
    src[1], src[-1] = -3, N + 5  # clamped to the first / last row
    got = ops.blend_rows(x.cuda(), dev32(off), dev32(src), torch.tensor(w, dtype=torch.float32).cuda())
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(LIST_LENGTHS), E)
    clamped = [min(max(s, 0), N - 1) for s in src]
    w32 = np.asarray(w, dtype=np.float32)
    want, bound = ref.blend_ref(x.float().numpy(), off, clamped, w32)
    got = got.cpu().numpy()
    for r, K in enumerate(LIST_LENGTHS):
        if K == 0:
            assert not got[r].any(), f"row {r}: an empty list gives zeros"
        elif K == 1:
            assert np.array_equal(got[r], x[clamped[off[r]]].float().numpy()), f"row {r}: a list of one copies the row"
        else:
            err = np.abs(got[r].astype(np.float64) - want[r])
            assert (err <= bound[r]).all(), f"row {r} (K = {K}): error {err.max():.3e}, bound {bound[r][err.argmax()]:.3e}"
    assert np.isfinite(got).all()


def test_blend_rows_all_lists_empty():
    x = torch.ones((3, 8)).cuda()
    none = torch.zeros((0,), dtype=torch.int32).cuda()
    got = ops.blend_rows(x, dev32([0, 0, 0]), none, torch.zeros((0,), dtype=torch.float32).cuda())
    assert tuple(got.shape) == (2, 8) and not got.any()


STITCH_CASES = [
    # (R, starts in body coordinates, Lb)
    (5, [2], 9),                    # one window inside a longer body: NaN around it
    (5, [0], 5),                    # one window that is the whole body
    (5, [0, 6], 11),                # two windows with a gap: pairs across them are NaN, residue 5 is in no window
    (6, [0, 3], 9),                 # two overlapping windows, even R: exact ties go to the lower start
    (5, [0, 2, 4, 6], 11),          # a grid of four
    (6, [0, 3, 6, 17], 23),         # four windows, the last one apart from the others
    (6, [17, 6, 0, 3], 23),         # the same windows in another order: ties go to the lower START, not the lower index
]


@pytest.mark.parametrize("body_lo", [0, 1])
@pytest.mark.parametrize("R,starts,Lb", STITCH_CASES)
def test_stitch_contacts(R, starts, Lb, body_lo):
    g = torch.Generator().manual_seed(R * 100 + Lb + len(starts))
    maps = torch.rand((len(starts), R, R), generator=g)
    tok_starts = [s + body_lo for s in starts]
    got = ops.stitch_contacts(maps.cuda(), dev32(tok_starts), Lb, body_lo=body_lo).cpu().numpy()
    want = ref.stitch_contacts_ref(maps.numpy(), tok_starts, Lb, body_lo)
    assert got.dtype == np.float32 and got.shape == (Lb, Lb)
    covered = np.zeros((Lb, Lb), dtype=bool)
    for s in starts:
        covered[s:s + R, s:s + R] = True
    assert np.array_equal(np.isnan(got), ~covered), "NaN exactly where no window holds the pair"
    assert np.array_equal(np.isnan(want), ~covered)
    assert np.array_equal(got[covered].view(np.uint32), want[covered].view(np.uint32))
    if R == 6 and sorted(starts)[:2] == [0, 3]:
        lower = starts.index(0)
        assert got[4, 4] == maps[lower, 4, 4]  # |2 s + 5 - 8| = 3 for s = 0 and s = 3: the lower start


def test_stitch_contacts_takes_any_start():
    """Starts are device data: a window far outside the body contributes nothing and nothing is read outside ``maps``."""
    maps = torch.rand((3, 5, 5))
    starts = [-40, 2, I32_MAX]
    got = ops.stitch_contacts(maps.cuda(), dev32(starts), 9, body_lo=1).cpu().numpy()
    assert np.array_equal(got, ref.stitch_contacts_ref(maps.numpy(), starts, 9, 1), equal_nan=True)
    assert np.array_equal(got[1:6, 1:6], maps[1].numpy())
