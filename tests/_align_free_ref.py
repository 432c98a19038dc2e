"""numpy restatement of alignment with free end gaps and of several hits per pair (esm_amd/align.py, csrc/align.hip), on top of
tests/_align_ref.py: the recurrence with the free-end mask over the FULL (La + 1) x (Lb + 1) grid, the end-cell rule, the walk,
the Waterman-Eggert rounds on a copy of S, and a brute-force enumeration of every path a mask allows.  Every fp32 step is one
numpy float32 operation, so the kernels are compared with this bit for bit.

The mask (global mode only; 0 is plain global mode): 1 a_start, 2 a_end, 4 b_start, 8 b_end.
    a_start   H[i][0] = 0 for all i (choice "stop");  b_start   on row 0 the stop candidate is 0, so H[0][j] = 0 (choice "stop")
    E and F on the borders are what they are in global mode
    end cell  the candidates are (La, Lb), the cells (i, Lb), i = 1 .. La, with a_end and the cells (La, j), j = 1 .. Lb, with
              b_end; the largest H wins, ties go to the lower row, then the lower column
    walk      on row 0 (j > 0) it stops with b_start, on column 0 (i > 0) with a_start; otherwise it emits the gaps
"""
import numpy as np

import _align_ref as ref

F32 = ref.F32
NEG = ref.NEG
A_START, A_END, B_START, B_END = 1, 2, 4, 8
NAMED = {"a": A_START | A_END, "b": B_START | B_END, "both": 15}


def dp(S, mode="global", o=1.0, e=0.1, free_ends=0):
    """H, E, F fp32 and the traceback bytes uint8, all [La + 1, Lb + 1], by anti-diagonals: ``_align_ref.dp`` with the stop
    candidate of the border cells set by the mask."""
    assert 0 <= free_ends <= 15 and (free_ends == 0 or mode == "global")
    S = np.ascontiguousarray(S, dtype=F32)
    La, Lb = S.shape
    o, e = F32(o), F32(e)
    local = mode == "local"
    H = np.full((La + 1, Lb + 1), NEG, dtype=F32)
    E = H.copy()
    F = H.copy()
    tb = np.zeros((La + 1, Lb + 1), dtype=np.uint8)
    H[0, 0] = 0
    with np.errstate(invalid="ignore"):
        for d in range(1, La + Lb + 1):
            i = np.arange(max(0, d - Lb), min(La, d) + 1)
            j = d - i
            ex, ey = H[i, j - 1] - o, E[i, j - 1] - e
            eb = (ey > ex) & (j > 0)
            Ev = np.where(j > 0, np.where(eb, ey, ex), NEG).astype(F32)
            fx, fy = H[i - 1, j] - o, F[i - 1, j] - e
            fb = (fy > fx) & (i > 0)
            Fv = np.where(i > 0, np.where(fb, fy, fx), NEG).astype(F32)
            Dv = np.where((i > 0) & (j > 0), S[i - 1, j - 1] + H[i - 1, j - 1], NEG).astype(F32)
            free = ((j == 0) & bool(free_ends & A_START)) | ((i == 0) & bool(free_ends & B_START))
            best = np.where(free | local, F32(0), NEG).astype(F32)
            ch = np.zeros(len(i), dtype=np.uint8)
            for code, v in ((1, Dv), (2, Fv), (3, Ev)):
                take = v > best
                best = np.where(take, v, best)
                ch = np.where(take, np.uint8(code), ch)
            H[i, j], E[i, j], F[i, j] = best, Ev, Fv
            tb[i, j] = ch | (eb.astype(np.uint8) << 2) | (fb.astype(np.uint8) << 3)
    return H, E, F, tb


def end_candidates(La, Lb, free_ends):
    """The end-cell candidates of global mode in the order of precedence: rows ascending, then columns ascending."""
    out = []
    for i in range(1, La + 1):
        if i < La and not free_ends & A_END:
            continue
        js = range(1, Lb + 1) if (i == La and free_ends & B_END) else (Lb,)
        out += [(i, j) for j in js]
    return out


def end_cell(H, mode, free_ends=0):
    """(score, (i, j)): local: ``_align_ref.end_cell``; global: the first of the largest H among the mask's candidates."""
    if mode == "local":
        return ref.end_cell(H, mode)
    best, cell = None, None
    for i, j in end_candidates(H.shape[0] - 1, H.shape[1] - 1, free_ends):
        if best is None or H[i, j] > best:
            best, cell = H[i, j], (i, j)
    return best, cell


def walk(tb, end, mode, free_ends=0):
    """The alignment's columns, ascending, from the bytes of the cells i, j >= 1 and the border rule: (cols int32 [n, 2],
    n_match, start cell).  ``tb`` is the full grid; its border bytes are not read."""
    i, j = end
    cols, n_match, state = [], 0, 0
    for _ in range(tb.shape[0] + tb.shape[1] - 2):
        if i == 0 and j == 0:
            break
        if i == 0 or j == 0:
            if mode == "local" or free_ends & (A_START if j == 0 else B_START):
                break
            if j == 0:
                i -= 1
                cols.append((i, -1))
            else:
                j -= 1
                cols.append((-1, j))
            state = 0
            continue
        b = int(tb[i, j])
        if state == 0:
            c = b & 3
            if c == 0:
                break
            if c == 1:
                i, j = i - 1, j - 1
                cols.append((i, j))
                n_match += 1
                continue
            state = 1 if c == 2 else 2
        if state == 1:
            i -= 1
            cols.append((i, -1))
            state = 1 if b & 8 else 0
        else:
            j -= 1
            cols.append((-1, j))
            state = 2 if b & 4 else 0
    return np.array(cols[::-1], dtype=np.int32).reshape(-1, 2), n_match, (i, j)


def align(S, mode="global", o=1.0, e=0.1, free_ends=0):
    """dict(score, end, start, cols, n_match, tb, H) as ``_align_ref.align`` gives them."""
    H, _, _, tb = dp(S, mode, o, e, free_ends)
    score, end = end_cell(H, mode, free_ends)
    cols, n_match, start = walk(tb, end, mode, free_ends)
    return dict(score=F32(score), end=end, start=start, cols=cols, n_match=n_match, tb=tb[1:, 1:].copy(), H=H, tb_full=tb)


def hits(S, K, mode="local", o=1.0, e=0.1, free_ends=0):
    """(the K hits of one pair, the S the last round ran on): after hit k the match cells of its path are -inf in a copy of S
    and the DP and the walk run again; the caller's S is left alone.  The returned S is masked by the hits 0 .. K - 2."""
    S = np.array(S, dtype=F32, copy=True)
    out = []
    for k in range(K):
        if k:
            m = out[-1]["cols"]
            m = m[(m[:, 0] >= 0) & (m[:, 1] >= 0)]
            S[m[:, 0], m[:, 1]] = NEG
        out.append(align(S, mode, o, e, free_ends))
    return out, S


def brute_force(S, o, e, free_ends=0):
    """The best score, in fp64, over ALL paths the mask allows: a path starts in (0, 0), or in (i, 0) with a_start, or in (0, j)
    with b_start; it ends in (La, Lb), or in (i, Lb), i >= 1, with a_end, or in (La, j), j >= 1, with b_end; a step is a match,
    a vertical or a horizontal gap column, a gap run of k costs o + (k - 1) e."""
    La, Lb = S.shape
    ends = set(end_candidates(La, Lb, free_ends))
    best = -np.inf

    def rec(i, j, prev, total):
        nonlocal best
        if (i, j) in ends and total > best:
            best = total
        if i < La and j < Lb:
            rec(i + 1, j + 1, 0, total + float(S[i, j]))
        if i < La:
            rec(i + 1, j, 1, total - (float(e) if prev == 1 else float(o)))
        if j < Lb:
            rec(i, j + 1, 2, total - (float(e) if prev == 2 else float(o)))

    starts = [(0, 0)]
    if free_ends & A_START:
        starts += [(i, 0) for i in range(1, La + 1)]
    if free_ends & B_START:
        starts += [(0, j) for j in range(1, Lb + 1)]
    for i, j in starts:
        rec(i, j, 0, 0.0)
    return best
