"""Zero-shot variant scoring on the MI355X engine: the three strategies of the reference's
``examples/variant-prediction/predict.py`` (wt-marginals, masked-marginals, pseudo-ppl) on top of ONE engine call,
``esmk_forward_rows`` (include/esmk.h): a batch of sequences plus a list of (sequence, position) rows in, fp32
log-probabilities ``[n_rows, V]`` of exactly those rows out.

The reference scores a protein of T tokens with T forwards at B = 1, builds ``[1, T, V]`` logits in each and keeps one row
(predict.py:205-215, :138-143).  Here the masked copies of a sequence are built on the device (``esmk_op_mask_rows``), run as
batches that fill the GPU, and the head of the model — final LayerNorm, LM head, vocabulary GEMM, log-softmax — runs on the
one masked row of every copy only.  Every kernel of the forward is batch-invariant bit for bit, so row (b, i) carries the
bits of the reference's loop run on this model's own ``forward``.

Variants with several substitutions ('A42G:K50R') take the masked-marginal score of the ESM-1v paper: ALL mutated
positions of the variant are masked in one forward (``masked_joint``, ``esmk_op_mask_rows_multi``) and
log p(mutant) - log p(wild type) is summed over them (``score_variants``, ``esmk_op_score_rows``: fp32 terms added in fp64
in a fixed order).

Libraries of sequences of DIFFERENT lengths (ranking designs by pseudo-log-likelihood, insertion / deletion variants,
wt-marginals over a FASTA file) can run token-packed: ``varlen=True`` lays the masked copies back to back in one row space
(``esmk_op_mask_rows_packed``, chunks planned by ``plan_packed_chunks``) and runs ``esmk_forward_packed_rows``
(``forward_rows_packed``), so the layer stack does no work on padding.  The packed forward gives every segment the bits of
that sequence alone: the tables are those of the padded path bit for bit, and the pseudo-log-likelihood is summed in a fixed
order (``esmk_op_sum_target_rows``).  ``python -m esm_amd.score_sequences`` scores a FASTA or CSV file that way.

A protein LONGER than the model's window (``window=N`` or ``window="max"``) is scored inside model-sized windows: every site in
the window copy centred on it, built on the device (``esmk_op_window_rows``), the rows again those of the existing call on the
window alone (``esm_amd.windows``, which also stitches embeddings and contact maps: ``forward_windows``).  Without ``window``
every call is what it was, the length check of ESM-1b / ESM-1v included.

Padded, token-packed, windowed and MSA copies all run through one loop, ``esm_amd.copies.run_copies``: a path uploads its
lists once and says how its copies fall into chunks, how a chunk is built and how it is run (``_padded_copies``,
``_packed_copies``, ``windows._run_copies``, ``msa_scoring.msa_masked_joint``).

The functions are also methods of ``ESM2`` / ``ProteinBertModel`` (``model.masked_marginals(tokens)`` ...).  They refuse the
MSA Transformer (``NotImplementedError``): one MSA plus a query row is another argument shape, served by
``esm_amd.msa_scoring`` under names of its own.
"""
import numbers

import torch

from .copies import CHUNK_TOKENS, Layout, copies_per_call, even_chunks, local_rows, run_copies, set_offsets


def _refuse_msa(model):
    from .msa_transformer import MSATransformer

    if isinstance(model, MSATransformer):
        raise NotImplementedError(
            "esm_amd.scoring: the MSA Transformer has no row-selected forward on the MI355X engine (esmk_forward_rows takes "
            "ESM-2, ESM-1b / ESM-1v and ESM-1 models) under the single-sequence names; one MSA plus a query row is scored by "
            "esm_amd.msa_scoring (msa_masked_marginals, msa_wt_marginals, msa_masked_joint, msa_score_variants)")


def _device_weight(model):
    w = model.embed_tokens.weight
    if not w.is_cuda:
        raise RuntimeError("esm_amd.scoring runs only on an MI355X (ROCm) device: move the model to 'cuda' first; the engine "
                           "has no CPU fallback")
    return w


def _device_tokens(model, tokens, window=None):
    """``window`` (resolved: tokens per window): the length check applies to the window copies, not to the batch's width."""
    _refuse_msa(model)
    if tokens.ndim == 1:
        tokens = tokens.unsqueeze(0)
    assert tokens.ndim == 2, "tokens: [B, T] (or [T])"
    w = _device_weight(model)
    pos_table = getattr(model, "embed_positions", None)
    max_positions = getattr(pos_table, "max_positions", None)
    width = tokens.size(1) if window is None else window
    if max_positions is not None and width > max_positions:  # ESM-1b / ESM-1v, as ProteinBertModel.forward
        raise ValueError(f"Sequence length {width} above maximum  sequence length of {max_positions}")
    return tokens.to(device=w.device, dtype=torch.int64).contiguous()


def forward_rows(model, tokens, sel_rows, return_logits=False):
    """``log_softmax(model(tokens)["logits"], -1).view(B * T, V)[sel_rows]`` as fp32 ``[n, V]``, without the ``[B, T, V]``
    tensor: the head of the model runs on the selected rows only.  ``tokens`` int64 ``[B, T]`` on the model's device,
    ``sel_rows`` int32 ``[n]`` flat row indices ``b * T + t`` on the same device (out-of-range indices are clamped by the
    engine, never read out of bounds).  ``return_logits``: also the selected fp32 logits (the bits ``forward`` gives those
    rows).  One stream: the two-stream forward (``ESM_AMD_DUAL_STREAM``) is not used here, and since every kernel is
    batch-invariant the bits do not depend on that."""
    tok = _device_tokens(model, tokens)
    dev = tok.device
    assert sel_rows.dtype == torch.int32 and sel_rows.ndim == 1 and sel_rows.device == dev and sel_rows.is_contiguous()
    return model._selected_rows(tok, sel_rows, return_logits)


def forward_rows_packed(model, tokens_flat, segments, sel_rows, return_logits=False):
    """``forward_rows`` for a token-packed batch (``esmk_forward_packed_rows``): fp32 ``[n, V]`` log-probabilities of the rows
    ``sel_rows`` of ONE packed row space.  ``tokens_flat`` int64 ``[rows]`` on the model's device (``ops.mask_rows_packed``
    builds it), rows % 64 == 0, gap rows holding the padding index; ``segments`` int32 ``[n_seg, 2]`` on the HOST (first row,
    length incl. <cls> / <eos>): the first segment starts at row 0, starts are ascending multiples of 16, segments disjoint;
    ``sel_rows`` int32 ``[n]`` flat indices into the row space, on the device (clamped by the engine to [0, rows)).  Every
    segment carries the bits of that sequence alone, so a row equals the row ``forward_rows`` gives the same sequence in a
    padded batch.  ``return_logits``: also the selected fp32 logits.  ESM-2 and ESM-1b / ESM-1v models; ESM-1 models and the
    f16x3 precision mode have no token-packed forward and are refused by the engine."""
    _refuse_msa(model)
    w = _device_weight(model)
    dev = w.device
    assert tokens_flat.dtype == torch.int64 and tokens_flat.ndim == 1 and tokens_flat.device == dev and tokens_flat.is_contiguous()
    assert sel_rows.dtype == torch.int32 and sel_rows.ndim == 1 and sel_rows.device == dev and sel_rows.is_contiguous()
    seg = torch.as_tensor(segments)
    assert seg.dtype == torch.int32 and not seg.is_cuda and seg.ndim == 2 and seg.shape[1] == 2 and seg.is_contiguous()
    return model._selected_rows(tokens_flat, sel_rows, return_logits, seg)


SEG_ALIGN = 16   # segment starts of a packed row space (esm_amd.packing, include/esmk.h)
ROWS_ALIGN = 64  # rows of a packed row space


def plan_packed_chunks(lengths_per_copy, budget=CHUNK_TOKENS):
    """The packed row spaces of a list of copies, on the host: ``[(lo, hi, starts, rows)]`` — chunk c holds the copies
    ``lo : hi`` of the input, IN INPUT ORDER, copy ``lo + j`` at rows ``starts[j] : starts[j] + length``.  Starts are ascending
    multiples of 16, the first one 0; a chunk is filled greedily until the sum of the lengths, each rounded up to 16, would
    pass ``budget`` rows (a copy that alone passes it gets a chunk of its own); ``rows`` is that sum rounded up to a multiple
    of 64.  Lengths must be positive."""
    if budget <= 0:
        raise ValueError("plan_packed_chunks: the row budget must be positive")
    chunks, lo, starts, used = [], 0, [], 0
    for i, length in enumerate(lengths_per_copy):
        length = int(length)
        if length <= 0:
            raise ValueError(f"plan_packed_chunks: copy {i} has length {length}: there is nothing to lay out")
        need = (length + SEG_ALIGN - 1) // SEG_ALIGN * SEG_ALIGN
        if starts and used + need > budget:
            chunks.append((lo, i, starts, (used + ROWS_ALIGN - 1) // ROWS_ALIGN * ROWS_ALIGN))
            lo, starts, used = i, [], 0
        starts.append(used)
        used += need
    if starts:
        chunks.append((lo, lo + len(starts), starts, (used + ROWS_ALIGN - 1) // ROWS_ALIGN * ROWS_ALIGN))
    return chunks


def _check_chunk_rows(varlen, chunk_rows):
    if chunk_rows is not None and not varlen:
        raise ValueError("chunk_rows sizes the packed row spaces of varlen=True; the padded path takes chunk")


def _token_lengths(model, tok_cpu):
    """int64 [B] on the host: 1 + the index of the last non-pad token of every sequence (0: nothing but padding) — the length
    of its copies in a packed row space; interior <pad> tokens stay inside."""
    T = tok_cpu.shape[1]
    return (tok_cpu.ne(model.padding_idx) * torch.arange(1, T + 1)).amax(dim=1)


def _packed_copies(model, tok, lengths, src, mask_off, mask_pos, sel_off, sel_pos, chunk_rows=None, return_logits=False):
    """Token-packed masked copies: copy i is the first ``lengths[src[i]]`` tokens of sequence ``src[i]`` of ``tok`` with the
    positions ``mask_pos[mask_off[i] : mask_off[i + 1]]`` replaced by <mask>, and the rows wanted from it are the positions
    ``sel_pos[sel_off[i] : sel_off[i + 1]]``.  All arguments but ``tok`` are int64 vectors on the host.  Returns the
    log-probabilities fp32 [n_rows, V] in the order of ``sel_pos`` (and the logits).  The lists of all chunks are uploaded
    once; a chunk (``plan_packed_chunks``, ``chunk_rows`` rows at most, default ``CHUNK_TOKENS``) is a slice of them."""
    from . import ops

    dev = tok.device
    copy_len = lengths[src]
    budget = CHUNK_TOKENS if chunk_rows is None else int(chunk_rows)
    chunks = plan_packed_chunks(copy_len.tolist(), budget) if src.numel() else []  # no copies: nothing is planned or refused
    rows_of = {lo: rows for lo, _, _, rows in chunks}
    start = torch.tensor([s for _, _, starts, _ in chunks for s in starts], dtype=torch.int64)
    seg_host = torch.stack([start, copy_len], dim=1).to(torch.int32).contiguous()
    sel_rows = torch.repeat_interleave(start, sel_off[1:] - sel_off[:-1]) + sel_pos  # chunk-local flat rows
    src32, start32, len32 = (t.to(torch.int32).to(dev) for t in (src, start, copy_len))
    off32, pos32, sel32 = (t.to(torch.int32).to(dev) for t in (mask_off, mask_pos, sel_rows))

    def build(lo, hi):  # the row space of the chunk and the host slice of its segment table
        flat = ops.mask_rows_packed(tok, src32[lo:hi], start32[lo:hi], len32[lo:hi], off32[lo:hi + 1], pos32, rows_of[lo],
                                    model.mask_idx, model.padding_idx)
        return flat, seg_host[lo:hi]

    layout = Layout(lambda: [(lo, hi) for lo, hi, _, _ in chunks], build,
                    lambda copies, sel, return_logits: forward_rows_packed(model, *copies, sel, return_logits=return_logits))
    return run_copies(layout, src.numel(), sel_off, sel32, model.alphabet_size, dev, return_logits)


def _padded_copies(model, tok, src32, pos32, off32, sel_off, sel_pos, chunk, return_logits=False):
    """Padded masked copies: copy i is sequence ``src32[i]`` of ``tok`` with position ``pos32[i]`` (``off32`` None) or the
    positions ``pos32[off32[i] : off32[i + 1]]`` replaced by <mask>; the rows wanted from it are the positions
    ``sel_pos[sel_off[i] : sel_off[i + 1]]``.  int32 vectors on the device, ``sel_off`` / ``sel_pos`` int64 on the host;
    ``chunk`` copies per call.  Returns what ``_packed_copies`` returns."""
    from . import ops

    T = tok.shape[1]

    def build(lo, hi):
        if off32 is None:
            return ops.mask_rows(tok, pos32[lo:hi].contiguous(), src32[lo:hi].contiguous(), model.mask_idx)
        return ops.mask_rows_multi(tok, off32[lo:hi + 1], pos32, src32[lo:hi], model.mask_idx)

    n = src32.numel()
    layout = Layout(even_chunks(n, chunk), build, lambda copies, sel, return_logits: forward_rows(model, copies, sel, return_logits))
    return run_copies(layout, n, sel_off, local_rows(sel_off, chunk, T, sel_pos, tok.device), model.alphabet_size, tok.device,
                      return_logits)


def _position_rows(model, tok_cpu, positions, residues_only):
    """(src, pos): int64 CPU vectors of the (sequence, position) rows to score, in sequence-major order.
    positions None: every non-pad position (``residues_only``: without the <cls> / <eos> tokens the alphabet adds);
    a bool mask [B, T]; one iterable of ints (the same positions in every sequence); or one iterable per sequence.
    A position outside [0, T) or on a <pad> token raises ValueError."""
    B, T = tok_cpu.shape
    real = tok_cpu.ne(model.padding_idx)
    if positions is None:
        want = real.clone()
        if residues_only:
            if model.prepend_bos:
                want[:, 0] = False
            if model.append_eos:
                want &= tok_cpu.ne(model.eos_idx)
    elif torch.is_tensor(positions) and positions.dtype == torch.bool:
        want = positions.cpu()
        if tuple(want.shape) != (B, T):
            raise ValueError(f"positions mask of shape {tuple(want.shape)} for tokens of shape {(B, T)}")
    else:
        positions = positions.tolist() if torch.is_tensor(positions) else list(positions)
        flat = not positions or isinstance(positions[0], numbers.Integral)  # (numpy integers included)
        per_seq = [positions] * B if flat else positions
        if len(per_seq) != B:
            raise ValueError(f"{len(per_seq)} position lists for {B} sequences")
        want = torch.zeros((B, T), dtype=torch.bool)
        for b, ps in enumerate(per_seq):
            for p in ps:
                if not 0 <= int(p) < T:
                    raise ValueError(f"position {p} of sequence {b} is outside [0, {T})")
                want[b, int(p)] = True
    if bool((want & ~real).any()):
        b, p = (want & ~real).nonzero()[0].tolist()
        raise ValueError(f"position {p} of sequence {b} is a <pad> token: there is nothing to score")
    src, pos = want.nonzero(as_tuple=True)
    return src, pos


def _masked_chunks(model, tokens, positions, chunk, residues_only, varlen=False, chunk_rows=None):
    """(src, pos, logprobs [n, V]): device int64 vectors of the scored rows and the log-softmax of the logits at ``pos`` from
    the forward in which that token alone is masked, the copies run in chunks.  ``varlen`` (on a model that has a
    token-packed forward): the copies run token-packed, each as long as its own sequence."""
    tok = _device_tokens(model, tokens)
    dev = tok.device
    tok_cpu = tok.cpu()
    src, pos = _position_rows(model, tok_cpu, positions, residues_only)
    one = torch.arange(src.numel() + 1, dtype=torch.int64)  # one masked position, one selected row per copy
    if varlen and model._packs():
        return src.to(dev), pos.to(dev), _packed_copies(model, tok, _token_lengths(model, tok_cpu), src, one, pos, one, pos,
                                                        chunk_rows)
    chunk = copies_per_call(chunk, tok.shape[1])
    src_d, pos_d = src.to(dev), pos.to(dev)  # one upload for all chunks: the chunks are slices of these
    return src_d, pos_d, _padded_copies(model, tok, src_d.to(torch.int32), pos_d.to(torch.int32), None, one, pos, chunk)


@torch.no_grad()
def masked_marginals(model, tokens, positions=None, chunk=None, varlen=False, chunk_rows=None, window=None, wrap=True):
    """fp32 ``[B, T, V]``: row (b, i) is ``log_softmax`` of the logits at i from the forward in which token (b, i) alone is
    replaced by <mask> — ``all_token_probs`` of the reference's masked-marginals strategy (predict.py:205-215) for every
    sequence of the batch.

    positions  None: every non-pad position including <cls> / <eos>, as predict.py:207 does; or a bool mask [B, T], one
               iterable of ints (the same positions in every sequence) or one iterable per sequence.  A position on a <pad>
               token or outside the row raises ValueError; pad tokens are never scored.
    chunk      masked copies per forward call; default what fills the GPU (about 65536 tokens).
    varlen     True: the copies run token-packed (module docstring), every copy as long as its own sequence (up to its last
               non-pad token; interior <pad> tokens stay inside) instead of the batch's width — the form for sequences of
               different lengths.  The table is the same, bit for bit.  ``chunk_rows``: rows of a packed row space (default
               65536); ``chunk`` is then not used.  ESM-1 models and the f16x3 precision mode have no token-packed forward:
               the padded path runs, as ``forward_varlen`` falls back to ``forward``.
    window     None: off.  An int (tokens per window, special tokens included) or "max" (ESM-1b / ESM-1v: the size of the
               position table): a sequence LONGER than the window is scored position by position inside the window copy
               centred on the position (``esm_amd.windows``: ``esmk_op_window_rows``; ``wrap``: the copies are tokenised
               fragments with <cls> / <eos> of their own, or raw token slices) — the row the existing call gives that
               window alone, bit for bit.  A sequence that fits takes the unwindowed path.  With ``varlen=True`` the short
               sequences go packed, the long ones through the padded window path.
    Rows that were not asked for are zero.  ``tokens`` may live on the CPU or the device; the result is on the model's device."""
    _check_chunk_rows(varlen, chunk_rows)
    if window is not None:
        from . import windows

        return windows.masked_marginals(model, tokens, positions, chunk, window, wrap, varlen, chunk_rows)
    tok = _device_tokens(model, tokens)
    out = torch.zeros(tuple(tok.shape) + (model.alphabet_size,), dtype=torch.float32, device=tok.device)
    src, pos, lp = _masked_chunks(model, tok, positions, chunk, residues_only=False, varlen=varlen, chunk_rows=chunk_rows)
    out[src, pos] = lp
    return out


@torch.no_grad()
def wt_marginals(model, tokens, varlen=False, chunk_rows=None, window=None, wrap=True):
    """fp32 ``[B, T, V]``: ``log_softmax(model(tokens)["logits"], -1)`` on the non-pad rows (the wt-marginals strategy,
    predict.py:192-194), zero on <pad> rows: one forward per batch that fills the GPU, the head on the real rows only.
    ``varlen`` / ``chunk_rows``: token-packed, as in ``masked_marginals``; the same table bit for bit.
    ``window`` / ``wrap``: a sequence longer than the window runs as overlapping grid windows (stride R // 2) and every row is
    taken from the window that owns it — the one it is most central in (``esm_amd.windows``)."""
    _check_chunk_rows(varlen, chunk_rows)
    if window is not None:
        from . import windows

        return windows.wt_marginals(model, tokens, window, wrap, varlen=varlen, chunk_rows=chunk_rows)
    tok = _device_tokens(model, tokens)
    B, T = tok.shape
    out = torch.zeros((B, T, model.alphabet_size), dtype=torch.float32, device=tok.device)
    if varlen and model._packs():
        tok_cpu = tok.cpu()
        lengths = _token_lengths(model, tok_cpu)
        real = tok_cpu.ne(model.padding_idx)
        src = lengths.nonzero().view(-1)  # a sequence of padding only contributes no segment
        sel_off = torch.zeros((src.numel() + 1,), dtype=torch.int64)
        sel_off[1:] = real.sum(1)[src].cumsum(0)
        none = torch.zeros((src.numel() + 1,), dtype=torch.int64)  # nothing is masked
        lp = _packed_copies(model, tok, lengths, src, none, torch.zeros((0,), dtype=torch.int64), sel_off,
                            real.nonzero(as_tuple=True)[1], chunk_rows)
        out[real.to(tok.device)] = lp  # both in (sequence, position) order
        return out
    step = copies_per_call(None, T)
    for lo in range(0, B, step):
        part = tok[lo:lo + step]
        real = part.ne(model.padding_idx)
        sel = real.view(-1).nonzero().view(-1).to(torch.int32)
        out[lo:lo + step][real] = forward_rows(model, part, sel)
    return out


@torch.no_grad()
def pseudo_log_likelihood(model, tokens, positions=None, chunk=None, varlen=False, chunk_rows=None, window=None, wrap=True):
    """fp64 ``[B]``: the sum over the scored positions of the masked-marginal log-probability of the TRUE token — the
    pseudo-log-likelihood of every sequence of the batch.

    positions  None: all residues, i.e. every non-pad token except the <cls> / <eos> the alphabet adds; otherwise as in
               ``masked_marginals``.
    The reference's ``compute_pppl`` (predict.py:138) iterates ``range(1, len(sequence) - 1)`` over the TOKEN positions
    (residue k sits at token position k + 1 behind <cls>) and so leaves out the end of the sequence: token positions
    len(sequence) - 1 and len(sequence).  The default here scores every residue; ``positions=range(1, len(sequence) - 1)``
    scores the reference's positions.  The value summed is always the log-probability of the token that was masked
    (predict.py:143 looks it up as ``sequence[i]``, the residue one behind token position i).  The per-row values are
    fp32, summed in fp64 as the reference sums Python floats.
    ``varlen`` / ``chunk_rows``: token-packed, as in ``masked_marginals``.  The sum then runs through
    ``esmk_op_sum_target_rows``: the rows of a sequence in ascending order of position, added by one lane — the sequential
    fp64 sum of the true-token column of ``masked_marginals``, exactly, where the padded path's ``index_add_`` adds through
    atomics in no fixed order.
    ``window`` / ``wrap``: the windowed masked marginals (``masked_marginals``), summed through ``esmk_op_sum_target_rows`` too."""
    from . import ops

    _check_chunk_rows(varlen, chunk_rows)
    if window is not None:
        from . import windows

        return windows.pseudo_log_likelihood(model, tokens, positions, chunk, window, wrap, varlen, chunk_rows)
    tok = _device_tokens(model, tokens)
    src, pos, lp = _masked_chunks(model, tok, positions, chunk, residues_only=True, varlen=varlen, chunk_rows=chunk_rows)
    if varlen and model._packs():
        if src.numel() == 0:
            return torch.zeros((tok.shape[0],), dtype=torch.float64, device=tok.device)
        seq_off = torch.zeros((tok.shape[0] + 1,), dtype=torch.int64, device=tok.device)
        seq_off[1:] = torch.bincount(src, minlength=tok.shape[0]).cumsum(0)  # rows are in (sequence, position) order
        return ops.sum_target_rows(lp, tok[src, pos].to(torch.int32), seq_off.to(torch.int32))
    out = torch.zeros((tok.shape[0],), dtype=torch.float64, device=tok.device)
    return out.index_add_(0, src, lp.gather(1, tok[src, pos].unsqueeze(1)).squeeze(1).double())


def _parse_sets(tok, position_sets, src):
    """(sets, src): every position set sorted and without repeats, and the sequence of every set as a list of ints."""
    B = tok.shape[0]
    sets = [sorted({int(p) for p in ps}) for ps in position_sets]
    if src is None:
        if B != 1:
            raise ValueError(f"masked_joint: tokens hold {B} sequences: say which one every position set refers to (src)")
        src = [0] * len(sets)
    src = [int(b) for b in (src.tolist() if torch.is_tensor(src) else src)]
    if len(src) != len(sets):
        raise ValueError(f"{len(src)} source sequences for {len(sets)} position sets")
    return sets, src


def _validate_sets(model, tok, sets, src):
    B, T = tok.shape
    real = tok.ne(model.padding_idx).cpu()
    for s, (b, ps) in enumerate(zip(src, sets)):
        if not 0 <= b < B:
            raise ValueError(f"position set {s}: sequence {b} is outside [0, {B})")
        if not ps:
            raise ValueError(f"position set {s} of sequence {b} is empty: there is nothing to score")
        for p in ps:
            if not 0 <= p < T:
                raise ValueError(f"position {p} of sequence {b} is outside [0, {T})")
            if not bool(real[b, p]):
                raise ValueError(f"position {p} of sequence {b} is a <pad> token: there is nothing to score")


@torch.no_grad()
def masked_joint(model, tokens, position_sets, src=None, chunk=None, return_logits=False, varlen=False, chunk_rows=None,
                 window=None, wrap=True):
    """Joint masks: for every set s of ``position_sets`` (an iterable of token positions of sequence ``src[s]``; ``src`` None:
    sequence 0, and then B must be 1) ONE forward with all positions of the set replaced by <mask>, and the log-probabilities
    at those positions.  Returns ``(offsets, pos, logprobs)``:

    offsets   int64 [n_sets + 1] on the host: set s owns rows offsets[s] : offsets[s + 1]
    pos       int64 [n_rows] on the device: the token position of every row, ascending inside a set
    logprobs  fp32 [n_rows, V] on the device: log_softmax of the logits at that position
    ``return_logits``: a fourth value, the selected fp32 logits (the bits ``forward`` of the masked sequence gives those rows).

    An empty set, a position outside [0, T) or on a <pad> token raises ValueError.  ``chunk``: masked copies (sets) per
    forward call; default what fills the GPU (about 65536 tokens).  The position lists are uploaded once for all chunks.
    ``varlen`` / ``chunk_rows``: token-packed, as in ``masked_marginals`` (sets of sequences of different lengths); the same
    rows bit for bit.
    ``window`` / ``wrap``: a set of a sequence longer than the window is masked in ONE window copy, placed so that the set sits
    in its middle (``esm_amd.windows.set_start``); a set that spans as many tokens as a window has body tokens, or more, does
    not fit and raises ValueError."""
    _check_chunk_rows(varlen, chunk_rows)
    if window is not None:
        from . import windows

        return windows.masked_joint(model, tokens, position_sets, src, chunk, return_logits, window, wrap, varlen, chunk_rows)
    tok = _device_tokens(model, tokens)
    B, T = tok.shape
    dev = tok.device
    sets, src = _parse_sets(tok, position_sets, src)
    chunk = copies_per_call(chunk, T)
    _validate_sets(model, tok, sets, src)
    offsets, pos = set_offsets(sets)
    pos_d = pos.to(dev)  # one upload for all chunks: the offsets index the whole position list, the chunks are slices of these
    if varlen and model._packs():
        got = _packed_copies(model, tok, _token_lengths(model, tok.cpu()), torch.tensor(src, dtype=torch.int64), offsets, pos,
                             offsets, pos, chunk_rows, return_logits=return_logits)
    else:
        got = _padded_copies(model, tok, torch.tensor(src, dtype=torch.int32).to(dev), pos_d.to(torch.int32),
                             offsets.to(device=dev, dtype=torch.int32), offsets, pos, chunk, return_logits=return_logits)
    return (offsets, pos_d) + (got if return_logits else (got,))


def parse_mutation(mutation, offset_idx=0):
    """'A42G' -> ('A', 42 - offset_idx, 'G'): wild type, 0-based index into the sequence, mutant."""
    mutation = mutation.strip()
    if len(mutation) < 3 or not mutation[1:-1].lstrip("-").isdigit():
        raise ValueError(f"mutation {mutation!r} is not of the form <wild type><position><mutant>, e.g. A42G")
    return mutation[0], int(mutation[1:-1]) - offset_idx, mutation[-1]


def score_mutations(token_logprobs, sequence, mutations, alphabet, offset_idx=0):
    """Scores of single-residue substitutions (``label_row`` of predict.py:107-115), on the host.

    token_logprobs  [T, V] or [1, T, V] log-probabilities of the tokenised sequence (``wt_marginals`` /
                    ``masked_marginals``); T counts the <cls> token when the alphabet prepends one
    sequence        the wild-type sequence the mutations refer to
    mutations       'A42G' or an iterable of such strings: wild type, position, mutant; the position is ``offset_idx``-based
    Returns the float log p(mutant) - log p(wild type) at the mutated position (a list for an iterable).  Raises ValueError
    where the listed wild type does not match the sequence or the position is outside it."""
    lp = token_logprobs[0] if token_logprobs.ndim == 3 else token_logprobs
    shift = 1 if alphabet.prepend_bos else 0  # row of residue idx: behind <cls>
    single = isinstance(mutations, str)
    scores = []
    for mutation in ([mutations] if single else mutations):
        wt, idx, mt = parse_mutation(mutation, offset_idx)
        if not 0 <= idx < len(sequence):
            raise ValueError(f"{mutation}: position {idx + offset_idx} is outside the sequence (offset {offset_idx}, "
                             f"length {len(sequence)})")
        if sequence[idx] != wt:
            raise ValueError(f"{mutation}: the listed wild type {wt!r} does not match the sequence, which has "
                             f"{sequence[idx]!r} at that position")
        row = lp[shift + idx]
        scores.append((row[alphabet.get_idx(mt)] - row[alphabet.get_idx(wt)]).item())
    return scores[0] if single else scores


def parse_variant(variant, offset_idx=0, sep=":"):
    """'A42G:K50R' -> [('A', 42 - offset_idx, 'G'), ('K', 50 - offset_idx, 'R')]: one ``parse_mutation`` per substitution of
    the variant, in the order written.  A position named twice raises ValueError."""
    parts = [parse_mutation(m, offset_idx) for m in variant.split(sep)]
    seen = set()
    for _, idx, _ in parts:
        if idx in seen:
            raise ValueError(f"variant {variant!r} names position {idx + offset_idx} twice")
        seen.add(idx)
    return parts


def _checked_variant(variant, sequence, offset_idx, sep):
    """``parse_variant`` plus the checks of ``score_mutations`` against the sequence, sorted by position."""
    parts = parse_variant(variant, offset_idx, sep)
    for wt, idx, _ in parts:
        if not 0 <= idx < len(sequence):
            raise ValueError(f"{variant}: position {idx + offset_idx} is outside the sequence (offset {offset_idx}, "
                             f"length {len(sequence)})")
        if sequence[idx] != wt:
            raise ValueError(f"{variant}: the listed wild type {wt!r} does not match the sequence, which has "
                             f"{sequence[idx]!r} at that position")
    return sorted(parts, key=lambda part: part[1])


@torch.no_grad()
def score_variants(model, alphabet, sequence, variants, strategy="masked-marginals", offset_idx=0, sep=":", chunk=None, window=None,
                   wrap=True):
    """Zero-shot scores of variants with one OR MORE substitutions ('A42G', 'A42G:K50R'; positions ``offset_idx``-based,
    joined by ``sep``) of ``sequence``: a list of Python floats, one per variant.

    masked-marginals  the ESM-1v paper's score: all mutated positions of the variant masked at once, one forward, the sum over
                      them of log p(mutant) - log p(wild type).  Variants that share a position set share one forward (the
                      distinct sets run in order of first appearance, ``chunk`` of them per engine call).
    wt-marginals      the same sum read from ONE table of the unmasked wild-type sequence.
    pseudo-ppl        the pseudo-log-likelihood of every mutated sequence over the reference's positions, as
                      ``esm_amd.predict.score_table`` does for single substitutions.
    The marginal strategies sum on the device (``esmk_op_score_rows``): each term is the fp32 difference ``score_mutations``
    gives a single substitution, the terms of a variant are added in fp64 in ascending order of position by one lane — a
    single mutant's score is the float ``score_mutations`` returns, and the order in which a variant lists its substitutions
    does not matter.  Raises ValueError where a listed wild type does not match the sequence, a position is outside it or
    named twice, or a substitution is not of the form 'A42G'.
    ``window`` / ``wrap``: for a sequence longer than the window, as in ``masked_joint`` / ``wt_marginals`` /
    ``pseudo_log_likelihood``; a variant whose sites do not fit into one window raises ValueError."""
    from . import ops

    _refuse_msa(model)
    win = {} if window is None else dict(window=window, wrap=wrap)
    if strategy not in ("masked-marginals", "wt-marginals", "pseudo-ppl"):
        raise ValueError(f"unknown scoring strategy {strategy!r}")
    parsed = [_checked_variant(v, sequence, offset_idx, sep) for v in variants]
    convert = alphabet.get_batch_converter()
    if strategy == "pseudo-ppl":
        mutated = []
        for variant, parts in zip(variants, parsed):
            residues = list(sequence)
            for _, idx, mt in parts:
                residues[idx] = mt
            mutated.append((variant, "".join(residues)))
        scores = []
        per_call = 256  # mutants per call; their masked copies are chunked to the GPU's size inside
        for lo in range(0, len(mutated), per_call):
            _, _, tokens = convert(mutated[lo:lo + per_call])
            scores += pseudo_log_likelihood(model, tokens, positions=range(1, len(sequence) - 1), chunk=chunk, **win).tolist()
        return scores
    _, _, tokens = convert([("protein1", sequence)])
    if window is not None:
        from .windows import resolve_window

        tok = _device_tokens(model, tokens, window=resolve_window(model, window))
    else:
        tok = _device_tokens(model, tokens)
    if not parsed:
        return []
    shift = 1 if alphabet.prepend_bos else 0  # token position of residue idx: behind <cls>
    if strategy == "masked-marginals":
        first_row = {}  # position set -> its first row in the joint-mask table; distinct sets in order of first appearance
        sets, n_rows = [], 0
        for parts in parsed:
            key = tuple(shift + idx for _, idx, _ in parts)
            if key not in first_row:
                first_row[key] = n_rows
                sets.append(key)
                n_rows += len(key)
        _, _, table = masked_joint(model, tok, sets, chunk=chunk, **win)
        rows = [first_row[tuple(shift + idx for _, idx, _ in parts)] + j for parts in parsed for j in range(len(parts))]
    else:
        table = wt_marginals(model, tok, **win)[0]
        rows = [shift + idx for parts in parsed for _, idx, _ in parts]
    dev = tok.device
    lp = table.index_select(0, torch.tensor(rows, dtype=torch.int64).to(dev))  # one row per term, variant-major
    wt = torch.tensor([alphabet.get_idx(w) for parts in parsed for w, _, _ in parts], dtype=torch.int32).to(dev)
    mt = torch.tensor([alphabet.get_idx(m) for parts in parsed for _, _, m in parts], dtype=torch.int32).to(dev)
    var_off = torch.zeros((len(parsed) + 1,), dtype=torch.int64)
    var_off[1:] = torch.tensor([len(parts) for parts in parsed]).cumsum(0)
    return ops.score_rows(lp, wt, mt, var_off.to(device=dev, dtype=torch.int32)).tolist()
