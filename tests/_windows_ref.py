"""A plain numpy / python restatement of the window definitions, written from the specification and not from
esm_amd/windows.py: brute force over all windows where the library uses bisection, Python lists where it uses tensors.

source row   n tokens; h = 1 if the alphabet prepends <cls>, t = 1 if it appends <eos>
wrap         R = window - h - t body tokens from source token s on, column 0 = <cls> if h, column h + R = <eos> if t, starts in
             [h, n - t - R]; raw: h = t = 0, R = window, starts in [0, n - R]
body range   [lo, hi) = [h, n - t) wrapped, [0, n) raw
s(p)         clamp(p - R // 2, lo, hi - R); a set: p = (min + max) // 2, ValueError when max - min >= R
grid         lo, lo + stride, ... while <= hi - R, plus hi - R; stride defaults to R // 2
owner of p   least |2 (p - s) - (R - 1)| among the windows that contain p, ties to the lower start
pair owner   least |2 s + R - 1 - (i + j)| among the windows that contain both, ties to the lower start; none: NaN
blend        weight of body column j: min(j + 1, R - j)
"""
import numpy as np


def geometry(n, window, wrap, h, t):
    return (window - h - t, h, n - t) if wrap else (window, 0, n)


def start_of(p, R, lo, hi):
    return min(max(p - R // 2, lo), hi - R)


def start_of_set(ps, R, lo, hi):
    """The specification's p = (min + max) // 2 leaves out max when the set spans exactly R positions and R is even; the window
    is then moved right by the one token that makes it hold the set (the only window that does)."""
    a, b = min(ps), max(ps)
    if b - a >= R:
        raise ValueError(f"set {sorted(ps)} does not fit into {R} body tokens")
    s = start_of((a + b) // 2, R, lo, hi)
    while s + R <= b:
        s += 1
    while s > a:
        s -= 1
    assert lo <= s <= hi - R
    return s


def grid(R, lo, hi, stride=None):
    stride = max(1, R // 2) if stride is None else stride
    assert 1 <= stride <= R and hi - lo >= R
    starts, s = [], lo
    while s <= hi - R:
        starts.append(s)
        s += stride
    if hi - R not in starts:
        starts.append(hi - R)
    return starts


def owner_of(p, starts, R):
    best = None
    for w, s in enumerate(starts):
        if s <= p < s + R:
            key = (abs(2 * (p - s) - (R - 1)), s)
            if best is None or key < best[0]:
                best = (key, w)
    return None if best is None else best[1]


def pair_owner_of(i, j, starts, R):
    best = None
    for w, s in enumerate(starts):
        if s <= i < s + R and s <= j < s + R:
            key = (abs(2 * s + R - 1 - (i + j)), s)
            if best is None or key < best[0]:
                best = (key, w)
    return None if best is None else best[1]


def weight(j, R):
    return float(min(j + 1, R - j))


def clamp(v, lo, hi):
    return min(max(v, lo), hi)


def window_rows_ref(tokens, src_row, start, mask_off, mask_pos, Tw, head_tok, tail_tok, mask_idx):
    """esmk_op_window_rows on lists: tokens [B][T]; every index clamped as the header says."""
    B, T = len(tokens), len(tokens[0])
    total = len(mask_pos)
    h = 1 if head_tok >= 0 else 0
    body_end = Tw - 1 if tail_tok >= 0 else Tw
    out = []
    for i in range(len(src_row)):
        b = clamp(src_row[i], 0, B - 1)
        row = [tokens[b][clamp(start[i] + c - h, 0, T - 1)] for c in range(Tw)]
        if tail_tok >= 0:
            row[Tw - 1] = tail_tok
        if head_tok >= 0:
            row[0] = head_tok
        a, e = clamp(mask_off[i], 0, total), clamp(mask_off[i + 1], 0, total)
        for k in range(a, e):
            c = mask_pos[k] - start[i] + h
            if h <= c < body_end:
                row[c] = mask_idx
        out.append(row)
    return out


def window_copy(tokens_row, s, window, wrap, h, t, cls_idx, eos_idx):
    """The window copy of a source row (a list of ints) at start s, unmasked."""
    R = window - h - t if wrap else window
    body = list(tokens_row[s:s + R])
    assert len(body) == R
    if not wrap:
        return body
    return ([cls_idx] if h else []) + body + ([eos_idx] if t else [])


def blend_ref(x, off, src, w):
    """esmk_op_blend_rows in fp64: x [N, E] (any float array), lists per output row.  Returns (out fp64 [n_out, E], bound
    [n_out, E]: (K + 2) 2^-23 max_k |x_k| per element, 0 for K <= 1)."""
    x = np.asarray(x, dtype=np.float64)
    n_out = len(off) - 1
    out = np.zeros((n_out, x.shape[1]))
    bound = np.zeros((n_out, x.shape[1]))
    for r in range(n_out):
        ks = list(range(off[r], off[r + 1]))
        if not ks:
            continue
        if len(ks) == 1:
            out[r] = x[src[ks[0]]]
            continue
        num = sum(np.float64(w[k]) * x[src[k]] for k in ks)
        out[r] = num / sum(np.float64(w[k]) for k in ks)
        bound[r] = (len(ks) + 2) * 2.0 ** -23 * np.max(np.abs(np.stack([x[src[k]] for k in ks])), axis=0)
    return out, bound


def stitch_contacts_ref(maps, starts, Lb, body_lo):
    """esmk_op_stitch_contacts: maps fp32 [n_w, R, R]; NaN where no window holds the pair."""
    maps = np.asarray(maps, dtype=np.float32)
    R = maps.shape[1]
    body = [s - body_lo for s in starts]
    out = np.full((Lb, Lb), np.nan, dtype=np.float32)
    for i in range(Lb):
        for j in range(Lb):
            w = pair_owner_of(i, j, body, R)
            if w is not None:
                out[i, j] = maps[w, i - body[w], j - body[w]]
    return out
