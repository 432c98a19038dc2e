"""References for the edits of the residual stream (esm_amd/csrc/interventions.hip, include/esmk.h: esmk_stream_edit).

  * the kernel in numpy float32: AXPBY one rounded operation at a time, PROJECT with its coefficient taken in fp64 and rounded
    once — what the kernel states, so x' is compared bit for bit;
  * the "decided" rule of PROJECT: the kernel sums its two fp64 dot products in another order than numpy does, so the two
    fp64 coefficients agree to ~E * 2^-53 relative to sum |x s| — a few 1e-13 of c at these widths, cancellation included.  A
    row counts when the fp64 c is farther than 1e-9 (relative) from every float32 rounding boundary: then both orders round
    to the same float32;
  * an fp32 forward of ESM-2 with edits, restated from the pieces of oracle/esm2_oracle.py (transformer_layer, layer_norm,
    FoldRows, the head's _linear / gelu).  It takes ``inject``, so ``_contract.floor_forward(..., forward=forward_edited_ref)``
    gives the floor in the engine's form; under "FOLD" an edit of a middle layer rebuilds the fold's row state of the edited
    rows from the edited stream, as the kernel does with rowstats' arithmetic.

An edit is the host dict ``esm_amd.interventions.StreamEdit.plan`` makes: layer, op (0 AXPBY, 1 PROJECT), keep, gain,
token_set or rows, src ([E] or [n, E]), src_index.
"""
import numpy as np
import torch

AXPBY, PROJECT = 0, 1
DECIDED_REL = 1e-9
UNDECIDED_CAP = 0.005  # of the projected rows of a GPU test; the committed inputs leave none (tests/test_stream_edit_cpu.py)


def axpby_rows(x, s, keep, gain):
    """x, s float32 arrays ([n, E]; s may be None): keep * x + gain * s with every product and the sum rounded on its own."""
    keep, gain = np.float32(keep), np.float32(gain)
    kx = (keep * x).astype(np.float32)
    if s is None:
        return kx
    return (kx + (gain * s).astype(np.float32)).astype(np.float32)


def decided(c64):
    """Is the fp64 coefficient farther than DECIDED_REL (relative) from the float32 rounding boundaries next to it?"""
    c64 = np.asarray(c64, dtype=np.float64)
    c32 = c64.astype(np.float32)
    up = np.nextafter(c32, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(c32, np.float32(-np.inf)).astype(np.float64)
    mid_up, mid_dn = (c32.astype(np.float64) + up) / 2, (c32.astype(np.float64) + dn) / 2
    gap = np.minimum(np.abs(c64 - mid_up), np.abs(c64 - mid_dn))
    return gap > DECIDED_REL * np.abs(c64)


def project_rows(x, s, gain):
    """(x', c64, changed): x' = x - float32(c) * s with c = gain <x, s> / <s, s> in fp64; rows with <s, s> = 0 stay."""
    xd, sd = x.astype(np.float64), s.astype(np.float64)
    ss = (sd * sd).sum(-1)
    changed = ss != 0
    c64 = np.where(changed, np.float64(np.float32(gain)) * (xd * sd).sum(-1) / np.where(changed, ss, 1.0), 0.0)
    c32 = c64.astype(np.float32)
    out = (x - (c32[:, None] * s).astype(np.float32)).astype(np.float32)
    return np.where(changed[:, None], out, x), c64, changed


def selected_rows(edit, tokens_flat):
    """(rows, source rows) the kernel edits: listed rows inside [0, N) in list order, or the rows whose token is in the set;
    rows whose source row does not exist are left out, as the kernel leaves them alone."""
    N = tokens_flat.shape[0]
    if edit.get("rows") is not None:
        rows = np.asarray(edit["rows"], dtype=np.int64)
        idx = np.arange(rows.shape[0])
    else:
        t = np.asarray(tokens_flat, dtype=np.int64)
        inset = (t >= 0) & (t < 64) & (((np.uint64(edit["token_set"]) >> np.clip(t, 0, 63).astype(np.uint64)) & np.uint64(1)) == 1)
        rows = np.nonzero(inset)[0]
        idx = rows
    src = edit.get("src")
    si = idx
    if edit.get("src_index") is not None:
        si = np.asarray(edit["src_index"], dtype=np.int64)[idx]
    ok = (rows >= 0) & (rows < N)
    if src is not None and np.asarray(src).ndim == 2:
        ok &= (si >= 0) & (si < np.asarray(src).shape[0])
    return rows[ok], si[ok]


def apply_edit(x, tokens_flat, edit):
    """x float32 [N, E] -> (x', edited rows, decided flags of those rows).  A PROJECT row with <s, s> = 0 is not edited."""
    x = np.array(x, dtype=np.float32, copy=True)
    rows, si = selected_rows(edit, tokens_flat)
    src = None if edit.get("src") is None else np.asarray(edit["src"], dtype=np.float32)
    s = None
    if src is not None:
        s = np.broadcast_to(src, (rows.shape[0], x.shape[1])) if src.ndim == 1 else src[si]
    if edit["op"] == PROJECT:
        new, c64, changed = project_rows(x[rows], s, edit["gain"])
        x[rows] = new
        return x, rows[changed], decided(c64)[changed]
    x[rows] = axpby_rows(x[rows], s, edit["keep"], edit["gain"])
    return x, rows, np.ones(rows.shape[0], dtype=bool)


def _edit_stream(x, tokens, edits, k, undecided):
    """Edits of layer k on the torch stream x [B, T, E]; returns (x', bool [B*T] rows any of them edited)."""
    B, T, E = x.shape
    hit = np.zeros(B * T, dtype=bool)
    for e in edits:
        if e["layer"] != k:
            continue
        host = dict(e, rows=None if e["rows"] is None else e["rows"].numpy(), src=None if e["src"] is None else e["src"].float().numpy(),
                    src_index=None if e["src_index"] is None else e["src_index"].numpy())
        flat, rows, ok = apply_edit(x.reshape(B * T, E).numpy(), tokens.reshape(-1).numpy(), host)
        x = torch.from_numpy(flat).reshape(B, T, E)
        hit[rows] = True
        undecided.append(int((~ok).sum()))
    return x, hit


@torch.no_grad()
def forward_edited_ref(sd, tokens, num_layers, heads, edits=(), repr_layers=(), token_dropout=True, padding_idx=1, mask_idx=32,
                       inject=None, inject_head="same", undecided=None):
    """oracle.esm2_oracle.esm2_forward (logits and representations) with ``edits`` applied to the stream after their layer and
    before that representation is taken.  ``undecided``: a list that receives the undecided PROJECT rows per edit."""
    from oracle.esm2_oracle import FoldRows, _is_fold, _linear, gelu, layer_norm, transformer_layer

    undecided = [] if undecided is None else undecided
    pad = tokens.eq(padding_idx)
    x = sd["embed_tokens.weight"][tokens]
    if token_dropout:
        x = x.masked_fill((tokens == mask_idx).unsqueeze(-1), 0.0)
        ratio = (tokens == mask_idx).sum(-1).to(x.dtype) / (~pad).sum(-1)
        x = x * (1 - 0.15 * 0.8) / (1 - ratio)[:, None, None]
    x = x * (1 - pad.unsqueeze(-1).type_as(x))
    x, _ = _edit_stream(x, tokens, edits, 0, undecided)
    wanted, reps = set(int(i) for i in repr_layers), {}
    if 0 in wanted:
        reps[0] = x
    pad_mask = pad if bool(pad.any()) else None
    fold = FoldRows(x, inject[1]) if _is_fold(inject) else None
    for i in range(num_layers):
        x, _ = transformer_layer(sd, i, x, heads, pad_mask, False, inject=inject, fold=fold, last=i + 1 == num_layers)
        x, hit = _edit_stream(x, tokens, edits, i + 1, undecided)
        if fold is not None and i + 1 < num_layers and hit.any():
            fresh = FoldRows(x, inject[1])  # the chain's entry form: the row's own mean, two-pass variance, T(x - mean)
            m = torch.from_numpy(hit).reshape(x.shape[0], x.shape[1], 1)
            fold.mean, fold.rstd, fold.rows = (torch.where(m, a, b) for a, b in
                                               ((fresh.mean, fold.mean), (fresh.rstd, fold.rstd), (fresh.rows, fold.rows)))
        if (i + 1) in wanted and i + 1 < num_layers:
            reps[i + 1] = x
    x = layer_norm(x, sd["emb_layer_norm_after.weight"], sd["emb_layer_norm_after.bias"])
    if num_layers in wanted:
        reps[num_layers] = x
    ih = inject if isinstance(inject_head, str) else inject_head
    h = gelu(_linear(x, sd["lm_head.dense.weight"], sd["lm_head.dense.bias"], ih))
    h = layer_norm(h, sd["lm_head.layer_norm.weight"], sd["lm_head.layer_norm.bias"])
    logits = _linear(h, sd["embed_tokens.weight"], None, ih) + sd["lm_head.bias"]
    return {"logits": logits, "representations": reps}


# ---- the inputs of the single-op tests (tests/test_stream_edit_ops_gpu.py; tests/test_stream_edit_cpu.py holds that none of
# their projected rows is undecided) ---------------------------------------------------------------------------------------
OPS_N = 9                                   # crosses rowstats' 2-rows-per-wave and 8-rows-per-block edges
OPS_SIZES = ((96, 128), (128, 128), (1280, 1280), (5120, 5120))   # (E, ldy)
OPS_ROW_LISTS = ([], [4], [0, 8, -1, 3, 9, 5, 2])                 # row 0, row N - 1, and the out-of-range values -1 and N
OPS_TOKENS = np.array([0, 5, 9, 1, 1, 32, 7, 2, 1], dtype=np.int64)  # <cls>, residues, <pad>s, <mask>, <eos>
OPS_TOKEN_SET = 0xFFFFFFF8                  # "residues" of the ESM-1b alphabet: no <cls>, <pad>, <eos> (0..2), no <mask> (32)


# 1e-9 of c is 1 - 3 % of the distance between two float32 values, so that share of random rows is undecided; these seeds are
# the first per width with which no projected row of ops_project_cases is (found by undecided_op_rows, counting up from 0)
OPS_SEEDS = {96: 1, 128: 0, 1280: 0, 5120: 1}
OPS_PROJECT_GAIN = 0.75


def ops_inputs(E, seed=None):
    """(x [N, E], per-row sources [N, E], one vector [E], source index [7] for the longest row list), float32 / int32."""
    g = np.random.default_rng(7000 * (OPS_SEEDS[E] if seed is None else seed) + E)
    x = (g.standard_normal((OPS_N, E)) * 3.0 + 0.5).astype(np.float32)
    src = g.standard_normal((OPS_N, E)).astype(np.float32)
    vec = g.standard_normal(E).astype(np.float32)
    index = np.array([3, 0, 1, 8, 2, 6, 6], dtype=np.int32)  # (source rows may repeat; a skipped row's entry is never read)
    return x, src, vec, index


def ops_project_cases(E, seed=None):
    """The PROJECT edits of the single-op test as reference dicts: one vector, per-row sources with and without an index on the
    longest row list; per-row sources under the token selector."""
    x, src, vec, index = ops_inputs(E, seed)
    rows = np.array(OPS_ROW_LISTS[2])
    base = dict(op=PROJECT, keep=1.0, gain=OPS_PROJECT_GAIN, token_set=0, rows=rows, src_index=None)
    return [dict(base, src=vec), dict(base, src=src), dict(base, src=src, src_index=index),
            dict(base, rows=None, token_set=OPS_TOKEN_SET, src=src), dict(base, rows=None, token_set=OPS_TOKEN_SET, src=vec)]


def undecided_op_rows(E, seed=None):
    x = ops_inputs(E, seed)[0]
    return sum(int((~apply_edit(x, OPS_TOKENS, e)[2]).sum()) for e in ops_project_cases(E, seed))
