"""numpy references of the decoding kernels (esm_amd/csrc/sampling.hip: ``sample_rows_kernel``, ``select_rows_kernel``):
the top-k / nucleus filter in front of the draw, the per-row confidence scores and the per-chain choice of the best rows.
Rank and selection are comparison logic on the fp32 inputs and are exact; the cumulative weights of the nucleus filter and the
draw are taken in fp64, with the rule that says which rows a comparison may count ("decided": every boundary the fp32 kernel
compares against is farther than DECIDED_MARGIN of the total from its threshold).  Philox, the uniforms and the draw itself are
those of tests/_sampling_ref.py.  No torch, no engine."""
import math

import numpy as np

import _sampling_ref as R

SCORE_NONE, SCORE_CONFIDENCE, SCORE_NEG_ENTROPY = 0, 1, 2


def ranked(row, cand):
    """The candidates best first: larger fp32 log-probability first, equal ones by the lower token, NaN last."""
    row = np.asarray(row, dtype=np.float32)

    def key(v):
        x = float(row[v])
        return (1, 0.0, v) if math.isnan(x) else (0, -x, v)

    return sorted(cand, key=key)


def keep_set(row, allowed_mask, inv_temperature, top_k=0, top_p=1.0, exclude=-1):
    """(kept bitset, decided) of one row.  Rank r is kept when (top_k == 0 or r < top_k) and (top_p >= 1 or E_r < top_p * W),
    E_r the sum of the weights exp(z - max z) of the ranks before r, W the sum over all candidates, z = row * inv_temperature
    (inv_temperature rounded to fp32 as the kernel receives it; 0, greedy, counts as 1); rank 0 is always kept.  Both filters
    off: every candidate, no arithmetic.  ``decided``: every E_r is farther than DECIDED_MARGIN * W from top_p * W."""
    row = np.asarray(row, dtype=np.float32)
    cand = R.candidates(row.shape[0], allowed_mask, exclude)
    if not cand:
        return 0, True
    if top_k == 0 and top_p >= 1.0:
        return sum(1 << v for v in cand), True
    order = ranked(row, cand)
    inv_t = float(np.float32(inv_temperature))
    z = row[order].astype(np.float64) * (inv_t if inv_t > 0.0 else 1.0)
    with np.errstate(invalid="ignore"):
        w = np.exp(z - z[0])
    before = np.concatenate(([0.0], np.cumsum(w)[:-1]))  # E_r
    total = float(np.sum(w))
    p = float(np.float32(top_p))
    kept, decided = 0, True
    for r, v in enumerate(order):
        ok = top_k == 0 or r < top_k
        if p < 1.0:
            ok = ok and bool(before[r] < p * total)
            decided = decided and bool(abs(before[r] - p * total) > R.DECIDED_MARGIN * total)
        if ok or r == 0:
            kept |= 1 << v
    return kept, decided


def draw_ex(row, u, allowed_mask, inv_temperature, top_k=0, top_p=1.0, exclude=-1):
    """(token, logq, kept, decided): the filter, then the draw of tests/_sampling_ref.py over the kept set."""
    kept, decided_keep = keep_set(row, allowed_mask, inv_temperature, top_k, top_p, exclude)
    if kept == 0:
        return -1, 0.0, 0, True
    inv_t = float(np.float32(inv_temperature))
    if inv_t == 0.0:  # greedy ignores the filters: the argmax is always kept
        tok, logq, _ = R.draw(row, u, allowed_mask, 0.0, exclude)
        return tok, logq, kept, True
    tok, logq, decided = R.draw(row, u, kept, inv_temperature)
    return tok, logq, kept, decided_keep and decided


def score(row, allowed_mask, inv_temperature, kind, exclude=-1):
    """The fp64 score of one row over its candidates BEFORE filtering, q = softmax(row * inv_temperature) (0, greedy, counts
    as 1): kind 1 = max log q, kind 2 = sum q log q (terms with q = 0 count as 0).  No candidate: -inf."""
    row = np.asarray(row, dtype=np.float32)
    cand = R.candidates(row.shape[0], allowed_mask, exclude)
    if not cand:
        return -math.inf
    inv_t = float(np.float32(inv_temperature))
    z = row[cand].astype(np.float64) * (inv_t if inv_t > 0.0 else 1.0)
    m = z.max()
    e = np.exp(z - m)
    s = e.sum()
    if kind == SCORE_CONFIDENCE:
        return float(-np.log(s))
    assert kind == SCORE_NEG_ENTROPY
    logq = z - m - np.log(s)
    q = e / s
    return float(np.sum(np.where(q > 0.0, q * np.where(q > 0.0, logq, 0.0), 0.0)))


def best_first(scores, lo, hi):
    """The rows lo .. hi - 1 best first: larger fp32 score first, equal scores by the lower row, NaN below everything (-inf
    included), among NaNs the lower row first."""
    scores = np.asarray(scores, dtype=np.float32)

    def key(i):
        x = float(scores[i])
        return (1, 0.0, i) if math.isnan(x) else (0, -x, i)

    return sorted(range(lo, hi), key=key)


def select(scores, row_off, sel_off, rest_off=None, sel_init=None, rest_init=None):
    """(sel_out, rest_out) of ``esmk_op_select_rows`` as lists; ``sel_init`` / ``rest_init``: what the outputs held before
    (elements outside every slice are left untouched).  rest_off None: no rest list."""
    n = len(scores)
    sel = list(sel_init)
    rest = list(rest_init) if rest_init is not None else []
    for c in range(len(row_off) - 1):
        lo, hi = min(max(row_off[c], 0), n), min(max(row_off[c + 1], 0), n)
        length = max(hi - lo, 0)
        k = min(max(sel_off[c + 1] - sel_off[c], 0), length)
        order = best_first(scores, lo, lo + length)
        for j, i in enumerate(order[:k]):
            if 0 <= sel_off[c] + j < len(sel):
                sel[sel_off[c] + j] = i
        if rest_off is not None:
            room = rest_off[c + 1] - rest_off[c]
            for j, i in enumerate(sorted(order[k:])):
                if j < room and 0 <= rest_off[c] + j < len(rest):
                    rest[rest_off[c] + j] = i
    return sel, rest
