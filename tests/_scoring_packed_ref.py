"""Plain-Python references of the packed scoring kernels (esm_amd/csrc/scoring.hip: mask_rows_packed_kernel,
sum_target_rows_kernel) and the mixed-length token batch the packed scoring tests share.  No torch arithmetic: lists of Python
ints, Python floats (IEEE fp64) added one after the other."""
import torch

PAD, MASK = 1, 32
# token counts with <cls> / <eos>: one residue; around the 16-row segment start; around the 64-row total and key tile; into a
# second 128-query block
LENGTHS = [3, 15, 16, 17, 63, 64, 65, 129, 130]
INTERIOR_PAD = (5, 30)  # (sequence, position): one <pad> inside the 64-token sequence


def clamp(v, lo, hi):
    return min(max(v, lo), hi)


def mask_rows_packed_ref(tokens, src_row, seg_start, seg_len, pos_off, pos, out, rows, mask_idx=MASK, pad_idx=PAD):
    """``out`` (a list of at least ``rows`` ints, whatever it holds) after the kernel: copy i = the first seg_len[i] tokens of
    tokens[src_row[i]] at out[seg_start[i] ...], its listed positions masked, the gap up to seg_start[i + 1] (``rows`` behind
    the last copy) filled with pad_idx.  Rules for lists the host never checked: source row clamped to [0, B), start to
    [0, rows], length to [0, T] and to the rows left, offsets to [0, total] (hi < lo: empty), a position outside [0, length)
    masks nothing.  The copies are applied in order; with disjoint row ranges (what the kernel requires) the order is
    immaterial."""
    B, T, n, total = len(tokens), len(tokens[0]), len(src_row), len(pos)
    for i in range(n):
        row = tokens[clamp(src_row[i], 0, B - 1)]
        start = clamp(seg_start[i], 0, rows)
        length = min(clamp(seg_len[i], 0, T), rows - start)
        end = clamp(seg_start[i + 1], start, rows) if i + 1 < n else rows
        for t in range(length):
            out[start + t] = row[t]
        for r in range(start + length, end):
            out[r] = pad_idx
        for j in range(clamp(pos_off[i], 0, total), clamp(pos_off[i + 1], 0, total)):
            if 0 <= pos[j] < length:
                out[start + pos[j]] = mask_idx
    return out


def sum_target_rows_ref(lp, target, off):
    """[n_seq] Python floats: the rows r of off[s] : off[s + 1], ascending, lp[r][clamp(target[r])] added one after the other in
    fp64.  ``lp``: nested lists of Python floats holding fp32 values exactly."""
    n_rows, V = len(lp), len(lp[0])
    out = []
    for s in range(len(off) - 1):
        acc = 0.0
        for r in range(clamp(off[s], 0, n_rows), clamp(off[s + 1], 0, n_rows)):
            acc += lp[r][clamp(target[r], 0, V - 1)]
        out.append(acc)
    return out


def library(cls=0, eos=2, seed=21):
    """int64 [9, 130] on the host: right-padded sequences of LENGTHS tokens (<cls>, residues 4..23, <eos>), one with an
    interior <pad>."""
    g = torch.Generator().manual_seed(seed)
    toks = torch.full((len(LENGTHS), max(LENGTHS)), PAD, dtype=torch.int64)
    for b, n in enumerate(LENGTHS):
        toks[b, :n] = torch.randint(4, 24, (n,), generator=g)
        toks[b, 0] = cls
        toks[b, n - 1] = eos
    toks[INTERIOR_PAD] = PAD
    return toks


def aligned_starts(lengths, align=16):
    """Back-to-back segment starts, each a multiple of ``align``; and the first free aligned row behind them."""
    starts, at = [], 0
    for n in lengths:
        starts.append(at)
        at += (n + align - 1) // align * align
    return starts, at
