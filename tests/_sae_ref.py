"""Plain numpy restatements of csrc/sae.hip (include/esmk.h: esmk_op_sae_rows ... esmk_op_sae_decode), written from the
definition in esm_amd/sae.py: nothing here calls the library."""
import numpy as np


def u_rows(x, rows, b_dec, input_scale):
    """fp32 [n, E]: u = sub(mul(input_scale, x[rows]), b_dec), each operation rounded to fp32 on its own"""
    x = np.asarray(x, dtype=np.float32)
    xr = x if rows is None else x[np.clip(np.asarray(rows), 0, x.shape[0] - 1)]
    prod = (np.float32(input_scale) * xr).astype(np.float32)
    if b_dec is None:
        b_dec = np.zeros(x.shape[1], dtype=np.float32)
    return (prod - np.asarray(b_dec, dtype=np.float32)[None, :]).astype(np.float32)


def image_rows(u):
    """fp16 [n, 3 Ep]: hi | hi | lo per 64-column K tile, hi = fp16(u), lo = fp16(u - hi); Ep = E rounded up to 64, pads zero"""
    n, E = u.shape
    Ep = (E + 63) // 64 * 64
    up = np.zeros((n, Ep), dtype=np.float32)
    up[:, :E] = u
    hi = up.astype(np.float16)
    lo = (up - hi.astype(np.float32)).astype(np.float16)  # the subtraction is exact in fp32
    t = np.stack([hi.reshape(n, Ep // 64, 64), hi.reshape(n, Ep // 64, 64), lo.reshape(n, Ep // 64, 64)], axis=2)
    return t.reshape(n, 3 * Ep)


def weight_image(w):
    """fp16 [F, 3 Kp]: hi | lo | hi per 64-column K tile of w fp32 [F, Kp] (Kp a multiple of 64)"""
    F, K = w.shape
    assert K % 64 == 0
    w = np.asarray(w, dtype=np.float32)
    hi = w.astype(np.float16)
    lo = (w - hi.astype(np.float32)).astype(np.float16)
    t = np.stack([hi.reshape(F, K // 64, 64), lo.reshape(F, K // 64, 64), hi.reshape(F, K // 64, 64)], axis=2)
    return t.reshape(F, 3 * K)


def active_mask(z, threshold):
    """z > threshold elementwise; a NaN (on either side) is never active"""
    z = np.asarray(z, dtype=np.float32)
    thr = np.broadcast_to(np.asarray(threshold, dtype=np.float32), z.shape[-1:])
    with np.errstate(invalid="ignore"):
        return z > thr[None, :]


def topk(z, threshold, k, k_sae=0):
    """(indices int32 [n, k], values fp32 [n, k], n_active int32 [n]): the k most active features of every row by a lexsort
    of (-value, index): value descending, ties to the lower index; unused slots -1 / 0.  k_sae > 0: a top-k autoencoder,
    n_active = min(k_sae, count)."""
    z = np.asarray(z, dtype=np.float32)
    n, F = z.shape
    act = active_mask(z, threshold)
    idx = np.full((n, k), -1, dtype=np.int32)
    val = np.zeros((n, k), dtype=np.float32)
    cnt = np.zeros((n,), dtype=np.int32)
    for i in range(n):
        f = np.nonzero(act[i])[0]
        v = z[i, f]
        order = np.lexsort((f, -v.astype(np.float64)))  # the last key is the primary one
        f, v = f[order], v[order]
        cnt[i] = min(k_sae, len(f)) if k_sae > 0 else len(f)
        m = min(k, len(f))
        idx[i, :m] = f[:m]
        val[i, :m] = v[:m]
    return idx, val, cnt


def kept_mask(z, threshold, k_sae=0):
    """bool [n, F]: the features whose activation is not zero — the actives, for a top-k autoencoder the k_sae best of them"""
    act = active_mask(z, threshold)
    if k_sae <= 0:
        return act
    idx, _, _ = topk(z, threshold, k_sae)
    keep = np.zeros_like(act)
    for i in range(act.shape[0]):
        keep[i, idx[i][idx[i] >= 0]] = True
    return keep


def segment_max(z, threshold, rows, B, k_sae=0):
    """(protein_max fp32 [B, F], protein_argmax int32 [B, F]): per sequence the largest activation of every feature over its
    rows and the position of the first row that reaches it; 0 / -1 where never active.  rows int [n, 2] (sequence, position)."""
    z = np.asarray(z, dtype=np.float32)
    keep = kept_mask(z, threshold, k_sae)
    F = z.shape[1]
    pmax = np.zeros((B, F), dtype=np.float32)
    parg = np.full((B, F), -1, dtype=np.int32)
    for i, (b, pos) in enumerate(np.asarray(rows)):
        better = keep[i] & (z[i] > pmax[b])
        pmax[b][better] = z[i][better]
        parg[b][better] = pos
    return pmax, parg


def decode(indices, values, w_dec, b_dec, input_scale):
    """fp32 [n, E]: mul(inv_scale, b_dec + sum_r mul(values[r], w_dec[indices[r]])), rank by rank, every product and every add
    rounded to fp32; index -1 skipped; inv_scale = float32(1 / input_scale)"""
    w_dec = np.asarray(w_dec, dtype=np.float32)
    n, k = indices.shape
    E = w_dec.shape[1]
    inv = np.float32(1.0 / input_scale)
    out = np.zeros((n, E), dtype=np.float32)
    for i in range(n):
        acc = np.zeros(E, dtype=np.float32) if b_dec is None else np.asarray(b_dec, dtype=np.float32).copy()
        for r in range(k):
            f = int(indices[i, r])
            if f < 0 or f >= w_dec.shape[0]:
                continue
            prod = (np.float32(values[i, r]) * w_dec[f]).astype(np.float32)
            acc = (acc + prod).astype(np.float32)
        out[i] = (inv * acc).astype(np.float32)
    return out


def z64(x, w_enc, b_enc, b_dec, input_scale):
    """fp64 [n, F]: the pre-activations from the fp32 u (the two stated roundings) with the product and the bias in fp64"""
    u = u_rows(x, None, b_dec, input_scale).astype(np.float64)
    return u @ np.asarray(w_enc, dtype=np.float64).T + np.asarray(b_enc, dtype=np.float64)[None, :]
