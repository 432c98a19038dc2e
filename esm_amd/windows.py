"""Proteins longer than the model's window: score, embed and map them as model-sized windows on the MI355X engine.

ESM-1b / ESM-1v take 1024 tokens, ESM-2 was trained on no more; variant-effect benchmarks are full of proteins of 1.5k to 5k
residues.  The usual practice is to score each mutated site inside a model-sized window centred on it, and to run overlapping
windows and stitch them for embeddings.  Here the window copies are built on the device (``esmk_op_window_rows``), run as
batches that fill the GPU through the row-selected forward (``esmk_forward_rows``) or ``forward``, and the per-window outputs
are stitched into full-length outputs on the device (``esmk_op_blend_rows``, ``esmk_op_stitch_contacts``).  All windows of a
long protein have the same width, so the padded path has no padding to waste; every kernel of the forward is batch-invariant,
so every output row carries the bits the existing API gives the window alone.

Definitions

source row   the n tokens of one sequence as the alphabet makes them, up to its last non-pad token; h = 1 if the alphabet
             prepends <cls>, t = 1 if it appends <eos>.
window       tokens per window, INCLUDING the special tokens a wrapped window carries: an int >= h + t + 1, or "max" = the
             model's ``embed_positions.max_positions`` (ESM-1b / ESM-1v only).  A sequence with n <= window is not windowed:
             it takes the unwindowed path and gives its bits.
wrap=True    a window is a fragment tokenised as the alphabet tokenises the substring: R = window - h - t body tokens from
             source token s on, <cls> in column 0 if h, <eos> in column h + R if t; starts s in [h, n - t - R].
wrap=False   a raw token slice: the same formulas with h = t = 0, R = window, s in [0, n - R]; only the first window carries
             <cls> and only the last <eos>.
body range   [lo, hi) = [h, n - t) wrapped, [0, n) raw.
start of p   s(p) = clamp(p - R // 2, lo, hi - R); of a set of positions: that of p = (min + max) // 2, moved by the least
             amount that makes the window hold the whole set (only a set that spans exactly R positions with R even needs
             it); max - min >= R: the set does not fit, ValueError.
grid         starts lo, lo + stride, ... while <= hi - R, plus hi - R if it is not on the grid; stride defaults to R // 2 (at
             least 1), 1 <= stride <= R.
owner of p   among the grid windows that contain p the one with the least |2 (p - s) - (R - 1)|, ties to the lower start;
             wrapped, the source's <cls> row is column 0 of the first grid window and its <eos> row the last column of the last.
pair owner   among the grid windows that contain both i and j the one with the least |2 s + R - 1 - (i + j)|, ties to the
             lower start; none: NaN in the stitched contact map.
blend        body column j of a window weighs min(j + 1, R - j).

The planning functions (``resolve_window`` ... ``blend_lists``) are pure host functions; the orchestration below them uploads
its index tables once per call and reads nothing back between the engine calls of a chunk loop.

Not built: the MSA Transformer (``NotImplementedError``), windows under ``gibbs_sample`` / ``inpaint`` / ``design`` / the
categorical Jacobian, token-packed window copies (windows of one width have no padding to save), contacts with ``wrap=False``.
"""
import bisect

import torch

from .copies import Layout, copies_per_call, even_chunks, local_rows, run_copies, set_offsets

CONTACT_ATTN_BYTES = 8 << 30  # forward(return_contacts=True) builds [B, L, H, T, T] fp32 maps: default chunks stay below this


# ---- planning: pure host functions ---------------------------------------------------------------------------------------
def _ends(model):
    return int(bool(model.prepend_bos)), int(bool(model.append_eos))


def resolve_window(model, window):
    """``window`` as the number of tokens per window, or None (off).  "max": the model's ``embed_positions.max_positions``
    (ESM-1b / ESM-1v); other models raise ValueError and ask for an int.  An int below h + t + 1 or above the model's
    ``max_positions`` raises ValueError; the MSA Transformer raises NotImplementedError."""
    if window is None:
        return None
    from .scoring import _refuse_msa

    _refuse_msa(model)
    h, t = _ends(model)
    max_positions = getattr(getattr(model, "embed_positions", None), "max_positions", None)
    if isinstance(window, str):
        if window != "max":
            raise ValueError(f"window {window!r}: an int (tokens per window) or 'max'")
        if max_positions is None:
            raise ValueError("window='max' is the size of the learned position table of ESM-1b / ESM-1v; this model has "
                             "none: give the window as an int (tokens per window, special tokens included)")
        return int(max_positions)
    if isinstance(window, bool) or int(window) != window:
        raise ValueError(f"window {window!r}: an int (tokens per window) or 'max'")
    window = int(window)
    if window < h + t + 1:
        raise ValueError(f"window {window} is below {h + t + 1}: a window holds the special tokens and at least one residue")
    if max_positions is not None and window > max_positions:
        raise ValueError(f"window {window} above maximum  sequence length of {max_positions}")
    return window


def window_arg(text):
    """The value of a command line's ``--window``: 'max' or a positive int."""
    if text == "max":
        return text
    try:
        value = int(text)
    except ValueError:
        value = 0
    if value <= 0:
        import argparse

        raise argparse.ArgumentTypeError(f"{text!r}: a positive number of tokens per window, or 'max'")
    return value


def geometry(n, window, wrap, h, t):
    """(R, lo, hi): body tokens per window and the body range of a source row of n tokens."""
    if wrap:
        return window - h - t, h, n - t
    return window, 0, n


def optimal_start(p, R, lo, hi):
    """s(p) = clamp(p - R // 2, lo, hi - R) for a position of the body range."""
    return min(max(p - R // 2, lo), hi - R)


def set_start(positions, R, lo, hi, name=None):
    """The start of the window of a SET of body positions: ``optimal_start`` of (min + max) // 2, moved by the least amount
    that makes the window hold min and max.  ValueError naming the set when max - min >= R."""
    ps = sorted(int(p) for p in positions)
    if not ps:
        raise ValueError("an empty position set has no window")
    if ps[-1] - ps[0] >= R:
        raise ValueError(f"position set {name if name is not None else ps} spans {ps[-1] - ps[0] + 1} tokens: it does not fit "
                         f"into one window of {R} body tokens")
    s = (ps[0] + ps[-1]) // 2 - R // 2
    s = min(max(s, ps[-1] - R + 1), ps[0])
    return min(max(s, lo), hi - R)


def grid_starts(R, lo, hi, stride=None):
    """The starts of the grid windows of a body range of at least R tokens, ascending."""
    if stride is None:
        stride = max(1, R // 2)
    stride = int(stride)
    if not 1 <= stride <= R:
        raise ValueError(f"window stride {stride} is outside [1, {R}] (R = body tokens per window)")
    if hi - lo < R:
        raise ValueError(f"a body range of {hi - lo} tokens holds no window of {R}")
    starts = list(range(lo, hi - R + 1, stride))
    if starts[-1] != hi - R:
        starts.append(hi - R)
    return starts


def _nearest(starts, a, b, twice_target):
    """Index in [a, b) of the ascending ``starts`` whose start s has the least |2 s - twice_target|, ties to the lower."""
    k = bisect.bisect_left(starts, (twice_target + 1) // 2, a, b)  # first start with 2 s >= twice_target
    best = None
    for c in (k - 1, k):
        if a <= c < b:
            key = abs(2 * starts[c] - twice_target)
            if best is None or key < best[0]:
                best = (key, c)
    return best[1]


def owners(starts, R, lo, hi):
    """For every body position p of [lo, hi) the index of its owner among the ascending grid ``starts``."""
    out = []
    for p in range(lo, hi):
        a, b = bisect.bisect_left(starts, p - R + 1), bisect.bisect_right(starts, p)
        if a >= b:
            raise ValueError(f"position {p} lies in no window: the starts do not cover [{lo}, {hi})")
        out.append(_nearest(starts, a, b, 2 * p - (R - 1)))  # |2 (p - s) - (R - 1)| = |2 s - (2 p - R + 1)|
    return out


def pair_owner(starts, R, i, j):
    """The index of the window of the ascending ``starts`` that owns the pair (i, j), or None where no window holds both."""
    a, b = bisect.bisect_left(starts, max(i, j) - R + 1), bisect.bisect_right(starts, min(i, j))
    if a >= b:
        return None
    return _nearest(starts, a, b, i + j - (R - 1))  # |2 s + R - 1 - (i + j)|


def blend_lists(starts, R, lo, hi):
    """For every body position p of [lo, hi): [(window index, body column j, weight min(j + 1, R - j))] of every grid window
    that contains p, in grid order."""
    out = []
    for p in range(lo, hi):
        a, b = bisect.bisect_left(starts, p - R + 1), bisect.bisect_right(starts, p)
        out.append([(w, p - starts[w], float(min(p - starts[w] + 1, R - (p - starts[w])))) for w in range(a, b)])
    return out


def plan_sequence(n, window, wrap, h, t, stride=None):
    """(R, lo, hi, starts) of a source row of n tokens, or None where n <= window: such a sequence is not windowed."""
    if n <= window:
        return None
    R, lo, hi = geometry(n, window, wrap, h, t)
    return R, lo, hi, grid_starts(R, lo, hi, stride)


# ---- orchestration ---------------------------------------------------------------------------------------------------------
def _i32(values, dev):
    return torch.as_tensor(values, dtype=torch.int64).to(torch.int32).to(dev)


def _special(model, wrap):
    """(h, t, head_tok, tail_tok) of the window copies."""
    h, t = _ends(model) if wrap else (0, 0)
    return h, t, (model.cls_idx if h else -1), (model.eos_idx if t else -1)


def _short_batch(tok, lengths, is_long):
    """(ids int64 [S] on the host, sub [S, W] on the device): the sequences that are not windowed, cut to their own width."""
    ids = (~is_long).nonzero().view(-1)
    if ids.numel() == 0:
        return ids, None
    W = max(1, int(lengths[ids].max()))
    return ids, tok[ids.to(tok.device), :W].contiguous()


def _run_copies(model, tok, Tw, src, start, mask_off, mask_pos, sel_off, sel_col, head_tok, tail_tok, chunk, return_logits=False):
    """Window copies through the row-selected forward.  Copy i is the window of sequence ``src[i]`` at ``start[i]`` with the
    source positions ``mask_pos[mask_off[i] : mask_off[i + 1]]`` masked; the rows wanted from it are its columns
    ``sel_col[sel_off[i] : sel_off[i + 1]]``.  Host lists; uploaded once, a chunk is a slice of them.  Returns the
    log-probabilities fp32 [n_rows, V] in the order of ``sel_col`` (and the logits)."""
    from . import ops, scoring

    dev = tok.device
    n = len(src)
    chunk = int(copies_per_call(chunk, Tw))
    sel_off = torch.as_tensor(sel_off, dtype=torch.int64)
    sel32 = local_rows(sel_off, chunk, Tw, torch.as_tensor(sel_col, dtype=torch.int64), dev)
    src32, start32, off32, pos32 = (_i32(v, dev) for v in (src, start, mask_off, mask_pos))

    def build(lo, hi):
        return ops.window_rows(tok, src32[lo:hi], start32[lo:hi], off32[lo:hi + 1], pos32, Tw, head_tok, tail_tok, model.mask_idx)

    layout = Layout(even_chunks(n, chunk), build,
                    lambda copies, sel, return_logits: scoring.forward_rows(model, copies, sel, return_logits))
    return run_copies(layout, n, sel_off, sel32, model.alphabet_size, dev, return_logits)


def _masked_rows(model, tok, positions, chunk, Tw, wrap, residues_only, varlen=False, chunk_rows=None):
    """Yields (src, pos, logprobs [n, V]): device int64 vectors of scored rows and the log-softmax of the logits at ``pos`` from
    the forward in which that token alone is masked — inside the window at s(pos) for a sequence longer than the window."""
    from . import scoring

    dev = tok.device
    tok_cpu = tok.cpu()
    src, pos = scoring._position_rows(model, tok_cpu, positions, residues_only)
    lengths = scoring._token_lengths(model, tok_cpu)
    is_long = lengths > Tw
    row_long = is_long[src]
    ids, sub = _short_batch(tok, lengths, is_long)
    if sub is not None and bool((~row_long).any()):
        new_index = torch.full((tok.shape[0],), -1, dtype=torch.int64)
        new_index[ids] = torch.arange(ids.numel())
        want = torch.zeros(tuple(sub.shape), dtype=torch.bool)
        want[new_index[src[~row_long]], pos[~row_long]] = True
        c_src, c_pos, lp = scoring._masked_chunks(model, sub, want, chunk, residues_only=False, varlen=varlen, chunk_rows=chunk_rows)
        yield ids.to(dev)[c_src], c_pos, lp
    if not bool(row_long.any()):
        return
    h, t, head_tok, tail_tok = _special(model, wrap)
    R = Tw - h - t
    b, p = src[row_long], pos[row_long]
    lo, hi = h, lengths[b] - t
    before, behind = p < lo, p >= hi  # the source's <cls> / <eos>: column 0 of the first window / the last of the last
    s = torch.minimum((p - R // 2).clamp(min=lo), hi - R)
    s = torch.where(before, torch.full_like(s, lo), torch.where(behind, hi - R, s))
    col = torch.where(before, torch.zeros_like(p), torch.where(behind, torch.full_like(p, Tw - 1), p - s + h))
    body = ~(before | behind)
    # the masked <cls> / <eos> of a wrapped window is the override token itself: those copies are built with <mask> as head / tail
    for rows, head, tail, masked in ((body, head_tok, tail_tok, True), (before, model.mask_idx, tail_tok, False),
                                     (behind, head_tok, model.mask_idx, False)):
        k = int(rows.sum())
        if k == 0:
            continue
        one = torch.arange(k + 1, dtype=torch.int64)
        lp = _run_copies(model, tok, Tw, b[rows], s[rows], one if masked else torch.zeros_like(one), p[rows] if masked else [],
                         one, col[rows], head, tail, chunk)
        yield b[rows].to(dev), p[rows].to(dev), lp


@torch.no_grad()
def masked_marginals(model, tokens, positions=None, chunk=None, window=None, wrap=True, varlen=False, chunk_rows=None):
    """``esm_amd.scoring.masked_marginals`` with ``window``: fp32 [B, T, V] in source coordinates; row (b, p) of a sequence
    longer than the window comes from the window copy at s(p) with p alone masked, row p - s(p) + h of it."""
    from . import scoring

    Tw = resolve_window(model, window)
    tok = scoring._device_tokens(model, tokens, window=Tw)
    out = torch.zeros(tuple(tok.shape) + (model.alphabet_size,), dtype=torch.float32, device=tok.device)
    for src, pos, lp in _masked_rows(model, tok, positions, chunk, Tw, wrap, False, varlen, chunk_rows):
        out[src, pos] = lp
    return out


@torch.no_grad()
def pseudo_log_likelihood(model, tokens, positions=None, chunk=None, window=None, wrap=True, varlen=False, chunk_rows=None):
    """``esm_amd.scoring.pseudo_log_likelihood`` with ``window``: the true-token column of the windowed masked marginals,
    summed per sequence in ascending order of position by one lane (``esmk_op_sum_target_rows``)."""
    from . import ops, scoring

    Tw = resolve_window(model, window)
    tok = scoring._device_tokens(model, tokens, window=Tw)
    B, T = tok.shape
    src, pos = scoring._position_rows(model, tok.cpu(), positions, residues_only=True)
    if src.numel() == 0:
        return torch.zeros((B,), dtype=torch.float64, device=tok.device)
    want = torch.zeros((B, T), dtype=torch.bool)
    want[src, pos] = True
    table = masked_marginals(model, tok, want, chunk, Tw, wrap, varlen, chunk_rows)
    seq_off = torch.zeros((B + 1,), dtype=torch.int64)
    seq_off[1:] = torch.bincount(src, minlength=B).cumsum(0)  # rows are in (sequence, position) order
    src, pos = src.to(tok.device), pos.to(tok.device)
    return ops.sum_target_rows(table[src, pos].contiguous(), tok[src, pos].to(torch.int32), _i32(seq_off, tok.device))


@torch.no_grad()
def wt_marginals(model, tokens, window=None, wrap=True, stride=None, chunk=None, varlen=False, chunk_rows=None):
    """``esm_amd.scoring.wt_marginals`` with ``window``: a sequence longer than the window runs as its grid windows, and every
    source row is taken from its owner."""
    from . import scoring

    Tw = resolve_window(model, window)
    tok = scoring._device_tokens(model, tokens, window=Tw)
    dev = tok.device
    B, T = tok.shape
    out = torch.zeros((B, T, model.alphabet_size), dtype=torch.float32, device=dev)
    tok_cpu = tok.cpu()
    lengths = scoring._token_lengths(model, tok_cpu)
    is_long = lengths > Tw
    ids, sub = _short_batch(tok, lengths, is_long)
    if sub is not None:
        kw = dict(varlen=True, chunk_rows=chunk_rows) if varlen else {}
        out[ids.to(dev), :sub.shape[1]] = scoring.wt_marginals(model, sub, **kw)
    h, t, head_tok, tail_tok = _special(model, wrap)
    real = tok_cpu.ne(model.padding_idx)
    src, start, sel_off, sel_col, dst_b, dst_p = [], [], [0], [], [], []
    for b in is_long.nonzero().view(-1).tolist():
        n = int(lengths[b])
        R, lo, hi, starts = plan_sequence(n, Tw, wrap, h, t, stride)
        cols = [[] for _ in starts]  # (column, source position) per window, ascending
        if lo > 0:
            cols[0].append((0, 0))
        for p, w in zip(range(lo, hi), owners(starts, R, lo, hi)):
            cols[w].append((p - starts[w] + h, p))
        if hi < n:
            cols[-1].append((Tw - 1, n - 1))
        for s, rows in zip(starts, cols):
            rows = [(c, p) for c, p in rows if bool(real[b, p])]  # interior <pad> rows stay zero, as without a window
            src.append(b)
            start.append(s)
            sel_col += [c for c, _ in rows]
            dst_b += [b] * len(rows)
            dst_p += [p for _, p in rows]
            sel_off.append(len(sel_col))
    if src:
        lp = _run_copies(model, tok, Tw, src, start, [0] * (len(src) + 1), [], sel_off, sel_col, head_tok, tail_tok, chunk)
        out[torch.tensor(dst_b).to(dev), torch.tensor(dst_p).to(dev)] = lp
    return out


@torch.no_grad()
def masked_joint(model, tokens, position_sets, src=None, chunk=None, return_logits=False, window=None, wrap=True, varlen=False,
                 chunk_rows=None):
    """``esm_amd.scoring.masked_joint`` with ``window``: a position set of a sequence longer than the window is masked in ONE
    window copy placed by the set rule (``set_start``); a set that spans R or more tokens, or that names the <cls> / <eos> of
    a wrapped long sequence, raises ValueError."""
    from . import scoring

    Tw = resolve_window(model, window)
    tok = scoring._device_tokens(model, tokens, window=Tw)
    dev = tok.device
    V = model.alphabet_size
    sets, src = scoring._parse_sets(tok, position_sets, src)
    copies_per_call(chunk, Tw)  # a chunk that is not positive is refused before the sets are looked at
    scoring._validate_sets(model, tok, sets, src)
    offsets, pos = set_offsets(sets)
    n_rows = int(offsets[-1])
    lp = torch.empty((n_rows, V), dtype=torch.float32, device=dev)
    logits = torch.empty((n_rows, V), dtype=torch.float32, device=dev) if return_logits else None
    lengths = scoring._token_lengths(model, tok.cpu())
    is_long = lengths > Tw
    h, t, head_tok, tail_tok = _special(model, wrap)

    def place(which, got):
        rows = torch.tensor([r for i in which for r in range(int(offsets[i]), int(offsets[i + 1]))], dtype=torch.int64).to(dev)
        lp[rows] = got[0] if return_logits else got
        if return_logits:
            logits[rows] = got[1]

    short = [i for i, b in enumerate(src) if not bool(is_long[b])]
    if short:
        ids, sub = _short_batch(tok, lengths, is_long)
        new_index = {int(b): j for j, b in enumerate(ids.tolist())}
        kw = dict(varlen=True, chunk_rows=chunk_rows) if varlen else {}
        got = scoring.masked_joint(model, sub, [sets[i] for i in short], src=[new_index[src[i]] for i in short], chunk=chunk,
                                   return_logits=return_logits, **kw)
        place(short, got[2:] if return_logits else got[2])
    wide = [i for i, b in enumerate(src) if bool(is_long[b])]
    if wide:
        c_start, c_off, c_pos, c_col = [], [0], [], []
        for i in wide:
            n = int(lengths[src[i]])
            R, lo, hi = geometry(n, Tw, wrap, h, t)
            for p in sets[i]:
                if not lo <= p < hi:
                    raise ValueError(f"position set {i} of sequence {src[i]}: position {p} is the <cls> / <eos> token of a "
                                     "windowed sequence, which belongs to no position set (score it with masked_marginals)")
            s = set_start(sets[i], R, lo, hi, name=f"{i} {sets[i]} of sequence {src[i]}")
            c_start.append(s)
            c_pos += sets[i]
            c_col += [p - s + h for p in sets[i]]
            c_off.append(len(c_pos))
        got = _run_copies(model, tok, Tw, [src[i] for i in wide], c_start, c_off, c_pos, c_off, c_col, head_tok, tail_tok, chunk,
                          return_logits=return_logits)
        place(wide, got)
    return (offsets, pos.to(dev), lp) + ((logits,) if return_logits else ())


@torch.no_grad()
def forward_windows(model, tokens, repr_layers=[], window=None, stride=None, wrap=True, stitch="owner", return_contacts=False,
                    chunk=None):
    """``forward``'s dict (``logits`` [B, T, V], ``representations`` {layer: [B, T, E]}, ``contacts`` [B, T - h - t, T - h - t]) in
    source coordinates for sequences of any length: a sequence longer than ``window`` runs as its grid windows (``stride``,
    default R // 2) through ``model.forward`` in chunks of ``chunk`` windows (default ``max(1, 65536 // window)``; with
    ``return_contacts`` at most what keeps the attention maps ``forward(return_contacts=True)`` builds below 8 GiB) and is
    stitched; a sequence that fits runs unwindowed and gives those bits.

    logits           always stitched by the owner rule
    representations  ``stitch="owner"``: every row from its owner window, exactly; ``"blend"``: the triangular-weight mean of
                     the rows of all grid windows that contain the position (``esmk_op_blend_rows``, fp32 accumulation); rows
                     of special tokens are never blended in, the source's <cls> / <eos> rows are owner rows
    contacts         per sequence by ``esmk_op_stitch_contacts``: every pair from its owner window, NaN where no window holds
                     both residues, 0 beyond a sequence's own length; needs ``wrap=True``
    Rows behind a sequence's last non-pad token are zero."""
    from . import ops, scoring

    if window is None:
        raise ValueError("forward_windows: give window= (tokens per window, or 'max')")
    if stitch not in ("owner", "blend"):
        raise ValueError(f"unknown stitch {stitch!r}: 'owner' or 'blend'")
    Tw = resolve_window(model, window)
    if return_contacts and not wrap:
        raise ValueError("forward_windows: contact maps are stitched from wrapped windows; return_contacts needs wrap=True")
    tok = scoring._device_tokens(model, tokens, window=Tw)
    dev = tok.device
    B, T = tok.shape
    lengths = scoring._token_lengths(model, tok.cpu())
    is_long = lengths > Tw
    h, t, head_tok, tail_tok = _special(model, wrap)
    eh, et = _ends(model)
    if chunk is None and return_contacts:
        chunk = max(1, min(copies_per_call(None, Tw), CONTACT_ATTN_BYTES // (4 * model.num_layers * model.attention_heads * Tw * Tw)))
    chunk = int(copies_per_call(chunk, Tw))
    kw = dict(return_contacts=True) if return_contacts else {}
    out = {}

    def room(name, like, shape):
        if name not in out:
            out[name] = torch.zeros(shape + tuple(like.shape[2:]), dtype=like.dtype, device=dev)
        return out[name]

    def contact_room(like):
        S = max(T - eh - et, 0)
        if "contacts" not in out:
            out["contacts"] = torch.zeros((B, S, S), dtype=like.dtype, device=dev)
        return out["contacts"]

    # the sequences that fit: the unwindowed forward on a batch of their own width
    ids, sub = _short_batch(tok, lengths, is_long)
    for lo in range(0, ids.numel(), chunk):
        part = ids[lo:lo + chunk].tolist()
        got = model.forward(sub[lo:lo + chunk], repr_layers=repr_layers, **kw)
        for j, b in enumerate(part):
            n = int(lengths[b])
            room("logits", got["logits"], (B, T))[b, :n] = got["logits"][j, :n]
            for l, r in got["representations"].items():
                room(("repr", l), r, (B, T))[b, :n] = r[j, :n]
            if return_contacts:
                Lb = max(n - eh - et, 0)
                contact_room(got["contacts"])[b, :Lb, :Lb] = got["contacts"][j, :Lb, :Lb]
    # the long ones: grid windows, sequence-major
    w_src, w_start, seq_windows = [], [], []
    dst_b, dst_p, own_row = [], [], []  # every source row and the flat window row that owns it
    b_off, b_row, b_w = [0], [], []  # per source row the list of (flat window row, weight) to blend
    for b in is_long.nonzero().view(-1).tolist():
        n = int(lengths[b])
        R, lo, hi, starts = plan_sequence(n, Tw, wrap, h, t, stride)
        w0 = len(w_src)
        seq_windows.append((b, w0, w0 + len(starts), hi - lo))
        w_src += [b] * len(starts)
        w_start += starts
        own = owners(starts, R, lo, hi)
        lists = blend_lists(starts, R, lo, hi) if stitch == "blend" else None
        for p in range(n):
            if p < lo:
                w, col = 0, 0
            elif p >= hi:
                w, col = len(starts) - 1, Tw - 1
            else:
                w = own[p - lo]
                col = p - starts[w] + h
            dst_b.append(b)
            dst_p.append(p)
            own_row.append((w0 + w) * Tw + col)
            if lists is not None and lo <= p < hi:
                b_row += [(w0 + w) * Tw + j + h for w, j, _ in lists[p - lo]]
                b_w += [wt for _, _, wt in lists[p - lo]]
            else:
                b_row.append(own_row[-1])
                b_w.append(1.0)
            b_off.append(len(b_row))
    if w_src:
        nW = len(w_src)
        src32, start32, none32 = _i32(w_src, dev), _i32(w_start, dev), torch.zeros((nW + 1,), dtype=torch.int32, device=dev)
        nopos = torch.zeros((0,), dtype=torch.int32, device=dev)
        db, dp, own32 = torch.tensor(dst_b).to(dev), torch.tensor(dst_p).to(dev), torch.tensor(own_row).to(dev)
        off32, row32, w32 = _i32(b_off, dev), _i32(b_row, dev), torch.tensor(b_w, dtype=torch.float32).to(dev)
        parts = []
        for lo in range(0, nW, chunk):
            hi = min(lo + chunk, nW)
            win = ops.window_rows(tok, src32[lo:hi], start32[lo:hi], none32[lo:hi + 1], nopos, Tw, head_tok, tail_tok, model.mask_idx)
            got = model.forward(win, repr_layers=repr_layers, **kw)
            parts.append({k: got[k] for k in ("logits", "representations") + (("contacts",) if return_contacts else ())})
        cat = lambda ts: ts[0] if len(ts) == 1 else torch.cat(ts)
        logits = cat([g["logits"] for g in parts])
        room("logits", logits, (B, T))[db, dp] = logits.view(nW * Tw, -1)[own32]
        for l in parts[0]["representations"]:
            x = cat([g["representations"][l] for g in parts])
            rows = ops.blend_rows(x.view(nW * Tw, -1).contiguous(), off32, row32, w32)
            room(("repr", l), x, (B, T))[db, dp] = rows.to(x.dtype)
        if return_contacts:
            maps = cat([g["contacts"] for g in parts])
            for b, w0, w1, Lb in seq_windows:
                ct = ops.stitch_contacts(maps[w0:w1].float().contiguous(), start32[w0:w1], Lb, body_lo=h)
                contact_room(maps)[b, :Lb, :Lb] = ct.to(maps.dtype)
    result = {"logits": out["logits"], "representations": {k[1]: v for k, v in out.items() if isinstance(k, tuple)}}
    if return_contacts:
        result["contacts"] = out["contacts"]
    return result
