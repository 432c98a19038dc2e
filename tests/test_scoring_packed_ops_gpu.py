"""The two kernels of packed scoring, one launch at a time (esm_amd/csrc/scoring.hip through esm_amd.ops):
``mask_rows_packed`` against a plain-Python reference bit for bit (tests/_scoring_packed_ref.py), ``sum_target_rows`` against a
sequential fp64 loop on the host, equal and not close.  The output buffer of the mask builder is pre-filled with a sentinel
(a gap row the kernel does not write shows) and has a sentinel tail behind ``rows`` (a write past the row space shows)."""
import pytest
import torch

from _scoring_packed_ref import (INTERIOR_PAD, LENGTHS, MASK, PAD, aligned_starts, library, mask_rows_packed_ref,
                                 sum_target_rows_ref)
from esm_amd import ops

pytestmark = pytest.mark.gpu
SENTINEL = -7
TAIL = 64


def i32(values):
    return torch.tensor(values, dtype=torch.int32).cuda()


def run_both(tokens, src, start, length, pos_off, pos, rows):
    """(kernel, reference): the whole buffer of rows + TAIL entries as lists."""
    buf = torch.full((rows + TAIL,), SENTINEL, dtype=torch.int64).cuda()
    got = ops.mask_rows_packed(tokens.cuda(), i32(src), i32(start), i32(length), i32(pos_off), i32(pos), rows, MASK, PAD, out=buf)
    assert got.data_ptr() == buf.data_ptr()
    want = mask_rows_packed_ref(tokens.tolist(), src, start, length, pos_off, pos, [SENTINEL] * (rows + TAIL), rows)
    return buf.cpu().tolist(), want


def test_mask_rows_packed_on_the_length_mix():
    """Every sequence of the length mix three times: some positions masked (first, last, one repeated), none masked, every
    position masked; the last copy's gap runs over more than a row tile to ``rows``."""
    toks = library()
    src, length, pos_off, pos = [], [], [0], []
    for b, n in enumerate(LENGTHS):
        for ps in ([0, n - 1, n // 2, n // 2], [], list(range(n))):
            src.append(b)
            length.append(n)
            pos += ps
            pos_off.append(len(pos))
    start, used = aligned_starts(length)
    rows = (used + 63) // 64 * 64 + 128
    got, want = run_both(toks, src, start, length, pos_off, pos, rows)
    assert got == want
    assert got[rows:] == [SENTINEL] * TAIL and SENTINEL not in got[:rows]  # every row written, nothing behind the row space
    # what the reference says, spelled out for one copy: sequence 5 (64 tokens, an interior <pad>), its first copy
    i = 3 * 5
    seg = got[start[i]:start[i] + 64]
    assert seg[0] == MASK and seg[63] == MASK and seg[32] == MASK and seg[INTERIOR_PAD[1]] == PAD
    assert seg[1:30] == toks[5, 1:30].tolist() and got[start[i] - 2:start[i]] == [MASK, PAD]  # (behind a 63-token copy)
    j = 3 * 6 + 1  # the unmasked copy of the 65-token sequence: 15 gap rows up to the next 16-row start
    assert got[start[j]:start[j] + 65] == toks[6, :65].tolist() and got[start[j] + 65:start[j + 1]] == [PAD] * 15
    assert got[used:rows] == [PAD] * (rows - used) and rows - used >= 128


def test_mask_rows_packed_clamps_what_the_host_never_saw():
    toks = library()
    T = toks.shape[1]
    rows = 256
    # copy 0: source row -3 -> 0, start -16 -> 0; copy 1: source row 100 -> 8, length 1000 -> T, positions -1, T, 200 mask
    # nothing, 5 twice; copy 2: length -5 -> 0, its whole range is gap; copy 3: 129 tokens at row 192 are cut to the 64 rows
    # left, position 64 is then outside; copy 4: start 9999 -> rows, nothing written
    src = [-3, 100, 4, 7, 2]
    start = [-16, 16, 160, 192, 9999]
    length = [3, 1000, -5, 129, 16]
    pos = [1, -1, T, 200, 5, 5, 0, 63, 64]
    pos_off = [-4, 1, 6, 7, 9, 50]  # -4 -> 0, 50 -> total = 9: the last list is empty
    got, want = run_both(toks, src, start, length, pos_off, pos, rows)
    assert got == want
    assert got[rows:] == [SENTINEL] * TAIL and SENTINEL not in got[:rows]
    assert got[:3] == [0, MASK, 2] and got[3:16] == [PAD] * 13
    assert got[16:16 + T] == [MASK if t == 5 else v for t, v in enumerate(toks[8].tolist())]
    assert got[16 + T:192] == [PAD] * (192 - 16 - T)
    assert got[192:256] == toks[7, :63].tolist() + [MASK]
    # a descending pair of offsets is an empty list
    got, want = run_both(toks, [1, 1], [0, 16], [15, 15], [3, 1, 2], [4, 7, 9], 64)
    assert got == want and got[:15] == toks[1, :15].tolist() and got[16 + 7] == MASK and got[16 + 4] == toks[1, 4].item()
    # no position list at all
    got, want = run_both(toks, [8], [0], [130], [0, 0], [], 192)
    assert got == want and got[:130] == toks[8].tolist() and got[130:192] == [PAD] * 62


def test_mask_rows_packed_more_copies_than_the_grid():
    """8200 copies of three tokens: more than the 8192 workgroups of the launch, so the copies are strided over the grid."""
    toks = library()
    n = 8200
    src = [i % len(LENGTHS) for i in range(n)]
    start = [16 * i for i in range(n)]
    pos_off = list(range(n + 1))
    pos = [i % 4 for i in range(n)]  # position 3 is outside the copy: every fourth copy stays unmasked
    got, want = run_both(toks, src, start, [3] * n, pos_off, pos, 16 * n)
    assert (16 * n) % 64 == 0 and got == want
    assert got[16 * 8199:16 * 8200] == toks[8199 % 9, :3].tolist() + [PAD] * 13  # 8199 % 4 == 3
    assert got[16 * 8198 + 2] == MASK


def test_mask_rows_packed_refusals():
    toks = library().cuda()
    one, off = i32([0]), i32([0, 0])
    with pytest.raises(RuntimeError, match="rows % 64"):
        ops.mask_rows_packed(toks, one, one, one, off, i32([]), 100)
    with pytest.raises(RuntimeError, match="rows"):
        ops.mask_rows_packed(toks, one, one, one, off, i32([]), 0, out=torch.zeros(64, dtype=torch.int64).cuda())


# ---- sum_target_rows ---------------------------------------------------------------------------------------------------
def table(n_rows, V=33, seed=3):
    """fp32 [n_rows, V]: magnitudes from 1e-6 to 1e2, both signs — terms 27 binary orders of magnitude apart, whose sum depends
    on the accumulator's width and, past a few thousand terms, on their order."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(10.0, torch.rand((n_rows, V), generator=g, dtype=torch.float64) * 8 - 6)
    sign = torch.randint(0, 2, (n_rows, V), generator=g) * 2 - 1
    return (mag * sign).float()


def test_sum_target_rows_is_the_sequential_fp64_sum():
    lp = table(1200)
    g = torch.Generator().manual_seed(4)
    target = torch.randint(0, 33, (1200,), generator=g).tolist()
    off = [0, 0, 1, 1001, 1001, 1200]  # ranges of 0, 1, 1000, 0 and 199 rows
    got = ops.sum_target_rows(lp.cuda(), i32(target), i32(off))
    assert got.dtype == torch.float64 and got.shape == (5,)
    want = sum_target_rows_ref(lp.tolist(), target, off)
    assert got.tolist() == want  # equal, not close
    assert want[0] == 0.0 and want[3] == 0.0 and want[1] == float(lp[0, target[0]])
    # the accumulator is fp64: the same 1000 terms added one after the other in fp32 give another number
    acc32 = torch.zeros((), dtype=torch.float32)
    for r in range(1, 1001):
        acc32 = acc32 + lp[r, target[r]]
    assert acc32.item() != want[2] and abs(acc32.item() - want[2]) < 1e-2


def test_sum_target_rows_clamps_targets_and_offsets():
    lp = table(40, seed=8)
    target = [-3, 99] * 20  # -> columns 0 and 32
    off = [-5, 10, 7, 40, 1000]  # -5 -> 0; (10, 7): descending, empty; 1000 -> 40: (40, 40) empty
    got = ops.sum_target_rows(lp.cuda(), i32(target), i32(off))
    want = sum_target_rows_ref(lp.tolist(), target, off)
    assert got.tolist() == want and want[1] == 0.0 and want[3] == 0.0
    by_hand = 0.0
    for r in range(10):
        by_hand += lp[r, 0 if r % 2 == 0 else 32].item()
    assert want[0] == by_hand
