"""numpy restatement of embedding-based alignment (esm_amd/align.py, csrc/align.hip): operand rows and their fp16 images, the
z-score enhancement, the affine-gap recurrence with its traceback bytes over the FULL (La + 1) x (Lb + 1) grid, the walk, and a
brute-force enumeration of global alignments.  Every fp32 step is one numpy float32 operation, so the kernels are compared with
this bit for bit."""
import itertools

import numpy as np

F32 = np.float32
NEG = F32(-np.inf)


# ---- operand rows -------------------------------------------------------------------------------------------------------
def sum_squares(x):
    """fp64 sum of squares of each row of x fp32 [n, E] in the kernel's order: thread t of 256 adds columns 4 t .. 4 t + 3,
    4 t + 1024 .., ascending; the partial sums fold as p[k] += p[k + s], s = 128 .. 1."""
    n, E = x.shape
    Ep = (E + 1023) // 1024 * 1024
    sq = np.zeros((n, Ep), dtype=np.float64)
    sq[:, :E] = x.astype(np.float64) ** 2
    sq = sq.reshape(n, Ep // 1024, 256, 4)
    part = np.zeros((n, 256), dtype=np.float64)
    for r in range(Ep // 1024):
        for e in range(4):
            part = part + sq[:, r, :, e]
    s = 128
    while s:
        part = part[:, :s] + part[:, s:2 * s]
        s >>= 1
    return part[:, 0]


def operand_rows(x, similarity="cosine"):
    """u fp32 [n, E]: cosine: x * float32(1 / sqrt(sum x^2)) (0 for a zero row), one fp32 product; dot: x."""
    x = np.ascontiguousarray(x, dtype=F32)
    if similarity == "dot":
        return x
    s = sum_squares(x)
    with np.errstate(divide="ignore"):
        r = np.where(s == 0.0, 0.0, 1.0 / np.sqrt(s)).astype(F32)
    return (x * r[:, None]).astype(F32)


def image(u, b_side=False):
    """fp16 [n, 3 Ep]: per 64-column K tile hi | hi | lo (a side) or hi | lo | hi (b side); hi = fp16(u), lo = fp16(u - hi)."""
    n, E = u.shape
    Ep = (E + 63) // 64 * 64
    up = np.zeros((n, Ep), dtype=F32)
    up[:, :E] = u
    hi = up.astype(np.float16)
    lo = (up - hi.astype(F32)).astype(np.float16)
    parts = (hi, lo, hi) if b_side else (hi, hi, lo)
    out = np.stack([p.reshape(n, Ep // 64, 64) for p in parts], 2)  # [n, tiles, 3, 64]
    return np.ascontiguousarray(out.reshape(n, 3 * Ep))


def split_product(ua, ub):
    """What the f16x3 GEMM computes, in fp64: hi hi + hi lo + lo hi of the two split operands."""
    def parts(u):
        hi = u.astype(np.float16)
        return hi.astype(np.float64), (u - hi.astype(F32)).astype(np.float16).astype(np.float64)
    ah, al = parts(ua)
    bh, bl = parts(ub)
    return ah @ bh.T + ah @ bl.T + al @ bh.T


# ---- enhancement --------------------------------------------------------------------------------------------------------
def _stats(S, axis):
    """(mu fp32, 1 / sigma fp32) along ``axis``: fp64 sums in ascending index order."""
    M = np.moveaxis(S.astype(np.float64), axis, 0)
    n = M.shape[0]
    s = np.zeros(M.shape[1], dtype=np.float64)
    for k in range(n):
        s = s + M[k]
    m = s / n
    q = np.zeros(M.shape[1], dtype=np.float64)
    for k in range(n):
        d = M[k] - m
        q = q + d * d
    sd = np.sqrt(q / n).astype(F32)
    with np.errstate(divide="ignore"):
        inv = np.where(sd == 0, F32(0), F32(1) / sd).astype(F32)
    return m.astype(F32), inv


def enhance(S):
    S = np.ascontiguousarray(S, dtype=F32)
    mu_r, inv_r = _stats(S, 1)
    mu_c, inv_c = _stats(S, 0)
    zr = ((S - mu_r[:, None]).astype(F32) * inv_r[:, None]).astype(F32)
    zc = ((S - mu_c[None, :]).astype(F32) * inv_c[None, :]).astype(F32)
    return (F32(0.5) * (zr + zc).astype(F32)).astype(F32)


# ---- the recurrence -------------------------------------------------------------------------------------------------------
def dp(S, mode="global", o=1.0, e=0.1):
    """H, E, F fp32 and the traceback bytes uint8, all [La + 1, Lb + 1], by anti-diagonals.  max(x, y) is y if y > x else x;
    H is the first of maximal value among [stop (local: 0; global: -inf), D, F, E]."""
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
            best = np.full(len(i), F32(0) if local else NEG, dtype=F32)
            ch = np.zeros(len(i), dtype=np.uint8)
            for code, v in ((1, Dv), (2, Fv), (3, Ev)):
                take = v > best
                best = np.where(take, v, best)
                ch = np.where(take, np.uint8(code), ch)
            H[i, j], E[i, j], F[i, j] = best, Ev, Fv
            tb[i, j] = ch | (eb.astype(np.uint8) << 2) | (fb.astype(np.uint8) << 3)
    return H, E, F, tb


def end_cell(H, mode):
    """(score, (i, j)): global: the last cell; local: the first largest H in row-major order — (0, 0) with score 0 when no H is
    above 0 (H[0][0] = 0 is the first cell)."""
    if mode == "global":
        return H[-1, -1], (H.shape[0] - 1, H.shape[1] - 1)
    k = int(np.argmax(H))  # the first occurrence, row-major
    return H.flat[k], (k // H.shape[1], k % H.shape[1])


def walk(tb, end, mode):
    """The alignment's columns, ascending, from the bytes alone: (cols int32 [n, 2], n_match, start cell).  At most La + Lb steps."""
    i, j = end
    cols, n_match, state = [], 0, 0
    for _ in range(tb.shape[0] + tb.shape[1] - 2):
        if i == 0 and j == 0:
            break
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


def align(S, mode="global", o=1.0, e=0.1):
    """dict(score, end, start, cols, n_match, tb): ``tb`` the bytes of the cells i, j >= 1, [La, Lb], as the kernel stores them."""
    H, _, _, tb = dp(S, mode, o, e)
    score, end = end_cell(H, mode)
    cols, n_match, start = walk(tb, end, mode)
    return dict(score=F32(score), end=end, start=start, cols=cols, n_match=n_match, tb=tb[1:, 1:].copy(), H=H)


def rescore(S, cols, o, e):
    """The score of an alignment given as columns, in fp64: matches add S, a gap run of k columns on one side costs o + (k - 1) e."""
    total, prev = 0.0, 0
    for i, j in cols:
        kind = 0 if (i >= 0 and j >= 0) else (1 if j < 0 else 2)
        if kind == 0:
            total += float(S[i, j])
        else:
            total -= float(e) if kind == prev else float(o)
        prev = kind
    return total


def brute_force_global(S, o, e):
    """The best score over ALL global alignments of La x Lb, in fp64 (every path of match / vertical / horizontal steps)."""
    La, Lb = S.shape
    best = -np.inf

    def rec(i, j, prev, total):
        nonlocal best
        if i == La and j == Lb:
            best = max(best, total)
            return
        if i < La and j < Lb:
            rec(i + 1, j + 1, 0, total + float(S[i, j]))
        if i < La:
            rec(i + 1, j, 1, total - (float(e) if prev == 1 else float(o)))
        if j < Lb:
            rec(i, j + 1, 2, total - (float(e) if prev == 2 else float(o)))

    rec(0, 0, 0, 0.0)
    return best


def sizes(panel):
    """The (La, Lb) the op tests stand on: the wavefront's edges and the panel's."""
    base = [1, 2, 63, 64, 65, 129]
    out = list(itertools.product(base, base))
    edge = [(5, panel - 1), (5, panel), (5, panel + 1), (3, 2 * panel + 3)]
    return out + edge + [(b, a) for a, b in edge]
