"""Zero-shot variant scoring with the MSA Transformer on the MI355X engine: the MSA branch of the reference's
``examples/variant-prediction/predict.py`` (:161-184) on top of ONE engine call, ``esmk_msa_forward_rows`` (include/esmk.h): a
batch of MSAs ``[B, R, C]`` plus a list of (copy, row, column) cells in, fp32 log-probabilities ``[n_cells, V]`` of exactly
those cells out.

The reference masks column i of the first row of the MSA, runs one forward of the whole MSA at B = 1, builds ``[1, R, C, V]``
logits and keeps one cell — once per column.  Here the masked copies of the MSA are built on the device
(``esmk_op_mask_rows_multi`` on the ``[1, R * C]`` view of the tokens, positions ``row * C + column``), run as batches that
fill the GPU, and the head of the model — final LayerNorm, LM head, vocabulary GEMM, log-softmax — runs on the scored cells
only.  The entry pins the slice count of the tied-row score GEMM to the one of a B = 1 forward, so copy b of a batch is
computed with the launches and the summation order of ``model.forward`` at B = 1 on that copy: a score does not depend on the
batch it was computed in, and cell (b, row, i) carries the bits of the reference's loop run on this model's own ``forward``.

One protein's MSA has a different argument shape from a batch of sequences (``[R, C]`` plus a query row), hence names of
their own: ``msa_masked_marginals``, ``msa_wt_marginals``, ``msa_masked_joint``, ``msa_score_variants`` — also methods of
``MSATransformer``.  The single-sequence names of ``esm_amd.scoring`` keep refusing the MSA Transformer.  ``msa_wt_marginals``
is an extension: the reference refuses every strategy but masked-marginals for MSAs (predict.py:163-165); pseudo-ppl is not
offered for MSAs.
"""
import torch

from .copies import Layout, copies_per_call, even_chunks, local_rows, run_copies, set_offsets
from .scoring import _checked_variant

STRATEGIES = ("masked-marginals", "wt-marginals")


def _check_msa(model, tokens, batched=False):
    """The shape checks, on whatever device the tokens live: ``[B, R, C]`` (``batched``) or one MSA ``[R, C]`` from
    ``[R, C]`` / ``[1, R, C]``."""
    from .msa_transformer import MSATransformer

    if not isinstance(model, MSATransformer):
        raise TypeError("esm_amd.msa_scoring takes an MSATransformer; esm_amd.scoring serves the single-sequence models")
    if batched:
        if tokens.ndim != 3:
            raise ValueError(f"tokens: [B, R, C], got a tensor of shape {tuple(tokens.shape)}")
    else:
        if tokens.ndim == 3 and tokens.shape[0] == 1:
            tokens = tokens[0]
        if tokens.ndim != 2:
            raise ValueError(f"tokens: one MSA, [R, C] or [1, R, C], got a tensor of shape {tuple(tokens.shape)}")
    R, C = tokens.shape[-2:]
    if model.msa_position_embedding is not None and R > 1024:  # as MSATransformer.forward
        raise RuntimeError("Using model with MSA position embedding trained on maximum MSA "
                           f"depth of 1024, but received {R} alignments.")
    if C > model.embed_positions.max_positions:
        raise ValueError(f"Sequence length {C} above maximum  sequence length of {model.embed_positions.max_positions}")
    return tokens


def _to_device(model, tokens):
    """int64 contiguous tokens on the model's device.  Argument errors (ValueError) are raised before this is asked."""
    w = model.embed_tokens.weight
    if not w.is_cuda:
        raise RuntimeError("esm_amd.msa_scoring runs only on an MI355X (ROCm) device: move the model to 'cuda' first; the "
                           "engine has no CPU fallback")
    return tokens.to(device=w.device, dtype=torch.int64).contiguous()


def msa_forward_rows(model, tokens, sel_rows, return_logits=False):
    """``log_softmax(model(tokens)["logits"], -1).view(B * R * C, V)[sel_rows]`` as fp32 ``[n, V]``, without the
    ``[B, R, C, V]`` tensor: the head of the model runs on the selected cells only.  ``tokens`` int64 ``[B, R, C]``,
    ``sel_rows`` int32 ``[n]`` flat indices ``(b * R + r) * C + c`` on the model's device (out-of-range indices are clamped by
    the engine, never read out of bounds).  ``return_logits``: also the selected fp32 logits.  When the B entries are masked
    copies of ONE MSA (what the functions below build), copy b is computed as ``model.forward`` computes it at B = 1, whatever B
    is: the slice pin of ``esmk_msa_forward_rows``.  A batch of different MSAs is served too, but the engine's pad flag is one
    per batch (with <pad> anywhere, columns padded in row 0 are masked out of the row attention of every entry): an unpadded MSA
    next to a padded one in which its row 0 has no <pad> still gets the same result, yet the bit claim is made and tested for
    copies of one MSA only."""
    tok = _to_device(model, _check_msa(model, tokens, batched=True))
    dev = tok.device
    assert sel_rows.dtype == torch.int32 and sel_rows.ndim == 1 and sel_rows.device == dev and sel_rows.is_contiguous()
    return model._selected_rows(tok, sel_rows, return_logits)


def _check_row(tok, row):
    R = tok.shape[0]
    if not 0 <= int(row) < R:
        raise ValueError(f"row {row} is outside [0, {R})")
    return int(row)


def _check_positions(model, tok_row_cpu, row, positions, what="position"):
    C = tok_row_cpu.numel()
    for p in positions:
        if not 0 <= p < C:
            raise ValueError(f"{what} {p} of row {row} is outside [0, {C})")
        if int(tok_row_cpu[p]) == model.padding_idx:
            raise ValueError(f"{what} {p} of row {row} is a <pad> token: there is nothing to score")


@torch.no_grad()
def msa_masked_joint(model, tokens, position_sets, row=0, chunk=None, return_logits=False):
    """Joint masks on one MSA: for every set s of ``position_sets`` (an iterable of columns of MSA row ``row``) ONE forward of
    the whole MSA with all columns of the set replaced by <mask> in that row, and the log-probabilities at those cells.
    Returns ``(offsets, pos, logprobs)`` as ``esm_amd.scoring.masked_joint`` does:

    offsets   int64 [n_sets + 1] on the host: set s owns rows offsets[s] : offsets[s + 1]
    pos       int64 [n_rows] on the device: the column of every row, ascending inside a set
    logprobs  fp32 [n_rows, V] on the device: log_softmax of the logits at (row, column)
    ``return_logits``: a fourth value, the selected fp32 logits (the bits ``forward`` of the masked MSA at B = 1 gives them).

    An empty set, a column outside [0, C) or on a <pad> token, or a ``row`` outside [0, R) raises ValueError.  ``chunk``: masked
    copies of the MSA per engine call; default ``max(1, 65536 // (R * C))``, what fills the GPU."""
    from . import ops

    tok = _check_msa(model, tokens)
    R, C = tok.shape
    row = _check_row(tok, row)
    sets = [sorted({int(p) for p in ps}) for ps in position_sets]
    chunk = copies_per_call(chunk, R * C)
    tok_row = tok[row].cpu()
    for s, ps in enumerate(sets):
        if not ps:
            raise ValueError(f"position set {s} is empty: there is nothing to score")
        _check_positions(model, tok_row, row, ps)
    tok = _to_device(model, tok)
    dev = tok.device
    offsets, pos = set_offsets(sets)
    # one upload for all chunks.  The MSA is one "sequence" of R * C tokens to the mask kernel: cell (row, c) is position
    # row * C + c of the [1, R * C] view, and a chunk of masked copies comes back as [n, R * C] = [n, R, C]
    flat = tok.view(1, R * C)
    pos_d = pos.to(dev)
    cell32 = (pos_d + row * C).to(torch.int32)
    off32 = offsets.to(device=dev, dtype=torch.int32)

    def build(lo, hi):
        return ops.mask_rows_multi(flat, off32[lo:hi + 1], cell32, None, model.mask_idx).view(hi - lo, R, C)

    layout = Layout(even_chunks(len(sets), chunk), build,
                    lambda copies, sel, return_logits: msa_forward_rows(model, copies, sel, return_logits))
    got = run_copies(layout, len(sets), offsets, local_rows(offsets, chunk, R * C, pos + row * C, dev), model.alphabet_size, dev,
                     return_logits)
    return (offsets, pos_d) + (got if return_logits else (got,))


def _columns(model, tok, row, positions):
    """The columns to score: every non-pad column of the row (None), or the listed ones, checked, ascending."""
    tok_row = tok[row].cpu()
    if positions is None:
        return tok_row.ne(model.padding_idx).nonzero().view(-1).tolist()
    cols = sorted({int(p) for p in (positions.tolist() if torch.is_tensor(positions) else positions)})
    _check_positions(model, tok_row, row, cols)
    return cols


@torch.no_grad()
def msa_masked_marginals(model, tokens, positions=None, row=0, chunk=None):
    """fp32 ``[C, V]``: row i is ``log_softmax`` of the logits at (``row``, i) from the forward of the MSA in which that
    token alone is replaced by <mask> — ``token_probs[0]`` of the reference's MSA branch (predict.py:167-178).

    tokens     one MSA, int64 ``[R, C]`` or ``[1, R, C]`` (on the CPU or the device)
    positions  None: every column, as predict.py:170 does (<pad> columns of the row are never scored); or an iterable of
               columns.  A column outside [0, C) or on a <pad> token raises ValueError, and so does a ``row`` outside [0, R).
    chunk      masked copies of the MSA per engine call; default ``max(1, 65536 // (R * C))``.
    Rows that were not asked for are zero; the result is on the model's device."""
    tok = _check_msa(model, tokens)
    row = _check_row(tok, row)
    cols = _columns(model, tok, row, positions)
    tok = _to_device(model, tok)
    out = torch.zeros((tok.shape[1], model.alphabet_size), dtype=torch.float32, device=tok.device)
    if cols:
        _, pos, lp = msa_masked_joint(model, tok, [[c] for c in cols], row=row, chunk=chunk)
        out[pos] = lp
    return out


@torch.no_grad()
def msa_wt_marginals(model, tokens, row=0):
    """fp32 ``[C, V]``: ``log_softmax(model(tokens[None])["logits"], -1)[0, row]`` on the non-pad columns of the row, zero
    on <pad> columns: ONE forward of the unmasked MSA, the head on that row only.  An extension: the reference refuses the
    wt-marginals strategy for the MSA Transformer (predict.py:163-165)."""
    tok = _check_msa(model, tokens)
    R, C = tok.shape
    row = _check_row(tok, row)
    tok = _to_device(model, tok)
    cols = tok[row].ne(model.padding_idx).nonzero().view(-1)
    out = torch.zeros((C, model.alphabet_size), dtype=torch.float32, device=tok.device)
    if cols.numel():
        out[cols] = msa_forward_rows(model, tok.view(1, R, C), (cols + row * C).to(torch.int32).contiguous())
    return out


@torch.no_grad()
def msa_score_variants(model, alphabet, msa, variants, strategy="masked-marginals", offset_idx=0, sep=":", chunk=None):
    """Zero-shot scores of variants with one or more substitutions ('A42G', 'A42G:K50R'; positions ``offset_idx``-based, joined
    by ``sep``) of the first sequence of ``msa``: a list of Python floats, one per variant.

    msa               ``[(label, aligned sequence)]`` (``esm_amd.fasta.read_msa``); the wild type is ``msa[0][1]``
    masked-marginals  all mutated positions of the variant masked in the first row of the MSA at once, one forward of the
                      MSA, the sum over them of log p(mutant) - log p(wild type).  For a single substitution that is the
                      reference's score (predict.py:167-184).  Variants that share a position set share one forward (the
                      distinct sets run in order of first appearance, ``chunk`` of them per engine call).
    wt-marginals      the same sum read from ONE forward of the unmasked MSA (an extension, see ``msa_wt_marginals``).
    The sum runs on the device (``esmk_op_score_rows``): fp32 terms added in fp64 in ascending order of position by one lane —
    a single mutant's score is the float ``score_mutations`` returns from the ``[C, V]`` table, and the order in which a
    variant lists its substitutions does not matter.  Raises ValueError where a listed wild type does not match the first
    sequence, a position is outside it or named twice, or a substitution is not of the form 'A42G'."""
    from . import ops

    if strategy not in STRATEGIES:
        raise ValueError(f"unknown scoring strategy {strategy!r} for an MSA (one of {', '.join(STRATEGIES)})")
    msa = list(msa)
    if not msa:
        raise ValueError("msa is empty")
    sequence = msa[0][1]
    parsed = [_checked_variant(v, sequence, offset_idx, sep) for v in variants]
    _, _, tokens = alphabet.get_batch_converter()(msa)
    tok = _to_device(model, _check_msa(model, tokens))
    if not parsed:
        return []
    shift = 1 if alphabet.prepend_bos else 0  # column of residue idx: behind <cls>
    if strategy == "masked-marginals":
        first_row = {}  # position set -> its first row in the joint-mask table; distinct sets in order of first appearance
        sets, n_rows = [], 0
        for parts in parsed:
            key = tuple(shift + idx for _, idx, _ in parts)
            if key not in first_row:
                first_row[key] = n_rows
                sets.append(key)
                n_rows += len(key)
        _, _, table = msa_masked_joint(model, tok, sets, chunk=chunk)
        rows = [first_row[tuple(shift + idx for _, idx, _ in parts)] + j for parts in parsed for j in range(len(parts))]
    else:
        table = msa_wt_marginals(model, tok)
        rows = [shift + idx for parts in parsed for _, idx, _ in parts]
    dev = tok.device
    lp = table.index_select(0, torch.tensor(rows, dtype=torch.int64).to(dev))  # one row per term, variant-major
    wt = torch.tensor([alphabet.get_idx(w) for parts in parsed for w, _, _ in parts], dtype=torch.int32).to(dev)
    mt = torch.tensor([alphabet.get_idx(m) for parts in parsed for _, _, m in parts], dtype=torch.int32).to(dev)
    var_off = torch.zeros((len(parsed) + 1,), dtype=torch.int64)
    var_off[1:] = torch.tensor([len(parts) for parts in parsed]).cumsum(0)
    return ops.score_rows(lp, wt, mt, var_off.to(device=dev, dtype=torch.int32)).tolist()


@torch.no_grad()
def msa_score_variants_ensemble(model, alphabet, msa, variants, num_seqs, n_subsamples=5, subsample="weighted", theta=0.2, seed=0,
                                strategy="masked-marginals", offset_idx=0, sep=":", chunk=None):
    """``msa_score_variants`` averaged over subsamples of a deep MSA, as the ESM-1v paper scores with the MSA Transformer:
    ``(mean, per_subsample)``.  Subsample s = 0 .. n_subsamples - 1 is ``esm_amd.msa_select.subsample_msa(msa, num_seqs,
    subsample, theta, seed, s)`` — "weighted" (sequence reweighting at ``theta``) or "uniform"; the query always stays row 0 —
    and is scored by ``msa_score_variants`` with the remaining arguments.  The neighbour counts of the full MSA are computed
    once.  ``per_subsample`` is the fp64 ``[n_subsamples, n_variants]`` matrix of those scores on the host; ``mean`` the list of
    Python floats ``sum over s ascending of per_subsample[s] / n_subsamples`` in fp64."""
    from . import msa_select

    if subsample not in msa_select.STRATEGIES:
        raise ValueError(f"unknown subsampling strategy {subsample!r} (one of {', '.join(msa_select.STRATEGIES)})")
    if int(n_subsamples) != n_subsamples or int(n_subsamples) < 1:
        raise ValueError(f"n_subsamples {n_subsamples!r} must be a positive integer")
    n_subsamples = int(n_subsamples)
    msa = list(msa)
    if not msa:
        raise ValueError("msa is empty")
    variants = list(variants)
    counts = None
    if subsample == "weighted" and len(msa) > int(num_seqs):
        counts = msa_select.msa_neighbor_counts(msa, theta)
    per = torch.zeros((n_subsamples, len(variants)), dtype=torch.float64)
    for s in range(n_subsamples):
        rows = msa_select.subsample_msa(msa, num_seqs, subsample, theta, seed, s, counts=counts)
        got = msa_score_variants(model, alphabet, rows, variants, strategy, offset_idx, sep, chunk)
        per[s] = torch.tensor(got, dtype=torch.float64)
    total = torch.zeros((len(variants),), dtype=torch.float64)
    for s in range(n_subsamples):
        total += per[s]
    return (total / n_subsamples).tolist(), per
