"""Zero-shot variant scoring on the MI355X engine: the three strategies of the reference's
``examples/variant-prediction/predict.py`` (wt-marginals, masked-marginals, pseudo-ppl) on top of ONE engine call,
``esmk_forward_rows`` (include/esmk.h): a batch of sequences plus a list of (sequence, position) rows in, fp32
log-probabilities ``[n_rows, V]`` of exactly those rows out.

The reference scores a protein of T tokens with T forwards at B = 1, builds ``[1, T, V]`` logits in each and keeps one row
(predict.py:205-215, :138-143).  Here the masked copies of a sequence are built on the device (``esmk_op_mask_rows``), run as
batches that fill the GPU, and the head of the model — final LayerNorm, LM head, vocabulary GEMM, log-softmax — runs on the
one masked row of every copy only.  Every kernel of the forward is batch-invariant bit for bit, so row (b, i) carries the
bits of the reference's loop run on this model's own ``forward``.

The functions are also methods of ``ESM2`` / ``ProteinBertModel`` (``model.masked_marginals(tokens)`` ...).  The MSA
Transformer has no row-selected forward: its methods raise ``NotImplementedError``.
"""
import ctypes
import numbers

import torch

CHUNK_TOKENS = 65536  # tokens per forward call that fill the GPU (the batch budget of esm_amd.extract)


def _refuse_msa(model):
    from .msa_transformer import MSATransformer

    if isinstance(model, MSATransformer):
        raise NotImplementedError(
            "esm_amd.scoring: the MSA Transformer has no row-selected forward on the MI355X engine (esmk_forward_rows takes "
            "ESM-2, ESM-1b / ESM-1v and ESM-1 models); masked marginals of an MSA are the reference's loop over model.forward")


def _device_tokens(model, tokens):
    _refuse_msa(model)
    if tokens.ndim == 1:
        tokens = tokens.unsqueeze(0)
    assert tokens.ndim == 2, "tokens: [B, T] (or [T])"
    w = model.embed_tokens.weight
    if not w.is_cuda:
        raise RuntimeError("esm_amd.scoring runs only on an MI355X (ROCm) device: move the model to 'cuda' first; the engine "
                           "has no CPU fallback")
    pos_table = getattr(model, "embed_positions", None)
    max_positions = getattr(pos_table, "max_positions", None)
    if max_positions is not None and tokens.size(1) > max_positions:  # ESM-1b / ESM-1v, as ProteinBertModel.forward
        raise ValueError(f"Sequence length {tokens.size(1)} above maximum  sequence length of {max_positions}")
    return tokens.to(device=w.device, dtype=torch.int64).contiguous()


def forward_rows(model, tokens, sel_rows, return_logits=False):
    """``log_softmax(model(tokens)["logits"], -1).view(B * T, V)[sel_rows]`` as fp32 ``[n, V]``, without the ``[B, T, V]``
    tensor: the head of the model runs on the selected rows only.  ``tokens`` int64 ``[B, T]`` on the model's device,
    ``sel_rows`` int32 ``[n]`` flat row indices ``b * T + t`` on the same device (out-of-range indices are clamped by the
    engine, never read out of bounds).  ``return_logits``: also the selected fp32 logits (the bits ``forward`` gives those
    rows).  One stream: the two-stream forward (``ESM_AMD_DUAL_STREAM``) is not used here, and since every kernel is
    batch-invariant the bits do not depend on that."""
    from . import _native as N

    tok = _device_tokens(model, tokens)
    dev = tok.device
    assert sel_rows.dtype == torch.int32 and sel_rows.ndim == 1 and sel_rows.device == dev and sel_rows.is_contiguous()
    B, T = tok.shape
    n = sel_rows.numel()
    V = model.alphabet_size
    if n == 0:
        empty = torch.empty((0, V), dtype=torch.float32, device=dev)
        return (empty, empty.clone()) if return_logits else empty
    with torch.cuda.device(dev):
        eng = model._engine_ready(dev)
        need, off = ctypes.c_size_t(), ctypes.c_size_t()
        N.check(N.lib.esmk_rows_workspace_bytes(eng.handle, B, T, n, ctypes.byref(need), ctypes.byref(off)))
        ws = eng.workspace_for_bytes(need.value)
        out = torch.empty((n, V), dtype=torch.float32, device=dev)
        N.check(N.lib.esmk_forward_rows(eng.handle, N.ptr(eng.packed), N.ptr(tok), B, T, N.ptr(sel_rows), n, N.ptr(out),
                                        N.ptr(ws), ws.numel(), N.cur_stream()))
        eng.max_T = max(eng.max_T, T)
        if return_logits:
            logits = ws[off.value: off.value + n * V * 4].view(torch.float32).view(n, V).clone()
            return out, logits
    return out


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


def _masked_chunks(model, tokens, positions, chunk, residues_only):
    """Yields (src, pos, logprobs [n, V]) per chunk: device int64 vectors of the scored rows and the log-softmax of the
    logits at ``pos`` from the forward in which that token alone is masked."""
    from . import ops

    tok = _device_tokens(model, tokens)
    B, T = tok.shape
    src, pos = _position_rows(model, tok.cpu(), positions, residues_only)
    if chunk is None:
        chunk = max(1, CHUNK_TOKENS // T)
    if chunk <= 0:
        raise ValueError("chunk must be positive")
    # one upload for all chunks: the chunks are slices of these
    src_d, pos_d = src.to(tok.device), pos.to(tok.device)
    src32, pos32 = src_d.to(torch.int32), pos_d.to(torch.int32)
    for lo in range(0, src.numel(), chunk):
        hi = min(lo + chunk, src.numel())
        masked = ops.mask_rows(tok, pos32[lo:hi].contiguous(), src32[lo:hi].contiguous(), model.mask_idx)
        sel = torch.arange(hi - lo, dtype=torch.int32, device=tok.device) * T + pos32[lo:hi]
        yield src_d[lo:hi], pos_d[lo:hi], forward_rows(model, masked, sel)


@torch.no_grad()
def masked_marginals(model, tokens, positions=None, chunk=None):
    """fp32 ``[B, T, V]``: row (b, i) is ``log_softmax`` of the logits at i from the forward in which token (b, i) alone is
    replaced by <mask> — ``all_token_probs`` of the reference's masked-marginals strategy (predict.py:205-215) for every
    sequence of the batch.

    positions  None: every non-pad position including <cls> / <eos>, as predict.py:207 does; or a bool mask [B, T], one
               iterable of ints (the same positions in every sequence) or one iterable per sequence.  A position on a <pad>
               token or outside the row raises ValueError; pad tokens are never scored.
    chunk      masked copies per forward call; default what fills the GPU (about 65536 tokens).
    Rows that were not asked for are zero.  ``tokens`` may live on the CPU or the device; the result is on the model's device."""
    tok = _device_tokens(model, tokens)
    out = torch.zeros(tuple(tok.shape) + (model.alphabet_size,), dtype=torch.float32, device=tok.device)
    for src, pos, lp in _masked_chunks(model, tok, positions, chunk, residues_only=False):
        out[src, pos] = lp
    return out


@torch.no_grad()
def wt_marginals(model, tokens):
    """fp32 ``[B, T, V]``: ``log_softmax(model(tokens)["logits"], -1)`` on the non-pad rows (the wt-marginals strategy,
    predict.py:192-194), zero on <pad> rows: one forward per batch that fills the GPU, the head on the real rows only."""
    tok = _device_tokens(model, tokens)
    B, T = tok.shape
    out = torch.zeros((B, T, model.alphabet_size), dtype=torch.float32, device=tok.device)
    step = max(1, CHUNK_TOKENS // T)
    for lo in range(0, B, step):
        part = tok[lo:lo + step]
        real = part.ne(model.padding_idx)
        sel = real.view(-1).nonzero().view(-1).to(torch.int32)
        out[lo:lo + step][real] = forward_rows(model, part, sel)
    return out


@torch.no_grad()
def pseudo_log_likelihood(model, tokens, positions=None, chunk=None):
    """fp64 ``[B]``: the sum over the scored positions of the masked-marginal log-probability of the TRUE token — the
    pseudo-log-likelihood of every sequence of the batch.

    positions  None: all residues, i.e. every non-pad token except the <cls> / <eos> the alphabet adds; otherwise as in
               ``masked_marginals``.
    The reference's ``compute_pppl`` (predict.py:138) iterates ``range(1, len(sequence) - 1)`` over the TOKEN positions
    (residue k sits at token position k + 1 behind <cls>) and so leaves out the end of the sequence: token positions
    len(sequence) - 1 and len(sequence).  The default here scores every residue; ``positions=range(1, len(sequence) - 1)``
    scores the reference's positions.  The value summed is always the log-probability of the token that was masked
    (predict.py:143 looks it up as ``sequence[i]``, the residue one behind token position i).  The per-row values are
    fp32, summed in fp64 as the reference sums Python floats."""
    tok = _device_tokens(model, tokens)
    out = torch.zeros((tok.shape[0],), dtype=torch.float64, device=tok.device)
    for src, pos, lp in _masked_chunks(model, tok, positions, chunk, residues_only=True):
        true = tok[src, pos].unsqueeze(1)
        out.index_add_(0, src, lp.gather(1, true).squeeze(1).double())
    return out


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
