"""The categorical Jacobian of a protein language model on the MI355X engine, and the unsupervised contact map it gives.

Put each candidate residue ``t_a`` at each residue position ``p_i`` of ONE protein and record how the logits at every other
position move:

    J[i, a, j, b] = logits(copy(i, a))[p_j, t_b] - logits(x)[p_j, t_b]          fp32 [L, nA, L, nA]

(the fp32 difference of two fp32 logits; the copy whose ``t_a`` is the wild type is ``x`` itself and is still run).  Centred
along its four axes, symmetrised and reduced over (a, b) it is a contact map that needs no regression head and reads no
attention maps — it also serves checkpoints that ship without ``contact-regression`` weights — and the tensor itself is the
pairwise epistasis table otherwise assembled from thousands of ``forward`` calls.

The ``L * nA`` copies are built on the device and run in batches that fill the GPU; a chunk is three engine calls on one
stream, and the host reads nothing in between:

    esmk_op_substitute_rows     the chunk's copies of the sequence, one token replaced in each
    esmk_forward_rows           the layer stack; the head on the L residue rows of every copy
    esmk_op_jacobian_scatter    J[copy, j, b] = logit - wild-type logit

Every kernel of the forward is batch-invariant bit for bit, so every logit carries the bits ``model(copy[None])["logits"]``
gives it at B = 1, and J does not depend on how the copies were chunked.  J stays on the device: ``esmk_op_jacobian_center``
(four in-place passes, axes b, j, a, i; fp64 means in a fixed order, one fp32 rounding per pass), ``esmk_op_jacobian_contacts``
(``S[i, j] = || 0.5 (Jc[i, :, j, :] + Jc[j, :, i, :]') ||_F``, fp64 terms) and ``esmk_op_apc`` (zero diagonal, average product
correction with fp64 sums) turn it into the ``[L, L]`` map there.

The functions are also methods of ``ESM2`` / ``ProteinBertModel``.  They refuse the MSA Transformer (``NotImplementedError``).
One sequence per call: batches of sequences and token-packed copies of several sequences are not built.
"""
import torch

from .sampling import STANDARD_RESIDUES, _residue_positions, allowed_mask
from .copies import copies_per_call
from .scoring import _device_tokens, _refuse_msa, forward_rows

MAX_CANDIDATES = 32  # esmk_op_jacobian_*: nA <= 32


def candidate_columns(model, allowed=None):
    """The candidate list ``A`` as vocabulary indices, in the order given: None = the 20 standard residues in the order of
    ``sampling.STANDARD_RESIDUES``; a string of residue letters; or an iterable of tokens (str) / token indices (int).
    ``sampling.allowed_mask``'s checks (unknown tokens, indices outside the vocabulary, an empty list), and the indices must
    be distinct and at most 32."""
    if allowed is None:
        allowed = STANDARD_RESIDUES
    allowed = list(allowed)
    allowed_mask(model, allowed)
    cols = [model.alphabet.get_idx(a) if isinstance(a, str) else int(a) for a in allowed]
    if len(set(cols)) != len(cols):
        raise ValueError("allowed: the candidate tokens must be distinct")
    if len(cols) > MAX_CANDIDATES:
        raise ValueError(f"allowed: {len(cols)} candidates; the Jacobian kernels take at most {MAX_CANDIDATES}")
    return cols


def _one_sequence(model, tokens):
    """(tokens int64 [1, T] on the device, the token positions of its residues)."""
    _refuse_msa(model)
    if tokens.ndim == 2 and tokens.shape[0] != 1:
        raise ValueError(f"the categorical Jacobian takes ONE sequence ([T] or [1, T]); tokens hold {tokens.shape[0]}")
    tok = _device_tokens(model, tokens)
    positions = _residue_positions(model, tok.cpu())[0]
    if not positions:
        raise ValueError("the sequence has no residues: there is nothing to substitute")
    return tok, positions


@torch.no_grad()
def categorical_jacobian(model, tokens, allowed=None, chunk=None, center=False, max_bytes=8 << 30):
    """fp32 ``[L, nA, L, nA]`` on the model's device: ``J[i, a, j, b]``, the change of the logit of candidate b at residue j
    when candidate a is put at residue i (module docstring).  ``tokens`` int64 ``[T]`` or ``[1, T]``, tokenised as for
    ``forward``; the L residues are its non-pad tokens without the <cls> / <eos> the alphabet adds.

    allowed    the candidate tokens (``candidate_columns``); default the 20 standard residues.
    chunk      copies per forward call; default what fills the GPU (``CHUNK_TOKENS // T``, not a multiple of nA: the copies
               of a position may straddle chunks).  The tensor is the same bit for bit whatever the chunk.
    center     the mean along each of the four axes removed in place (``ops.jacobian_center``).
    max_bytes  ValueError if the tensor (``L * L * nA * nA * 4`` bytes; 1.7 GB for 1022 residues and 20 candidates) would be
               larger."""
    from . import ops

    tok, positions = _one_sequence(model, tokens)
    cols = candidate_columns(model, allowed)
    dev = tok.device
    T, V = tok.shape[1], model.alphabet_size
    L, nA = len(positions), len(cols)
    if L * L * nA * nA * 4 > max_bytes:
        raise ValueError(f"the categorical Jacobian of {L} residues and {nA} candidates holds {L * L * nA * nA * 4} bytes, above "
                         f"max_bytes = {max_bytes}")
    n = L * nA
    chunk = min(copies_per_call(chunk if chunk is None else int(chunk), T), n)
    # one upload for all chunks: copy c = i * nA + a substitutes cols[a] at positions[i]; the chunks are slices of these
    pos32 = torch.tensor(positions, dtype=torch.int32).to(dev)
    cols32 = torch.tensor(cols, dtype=torch.int32).to(dev)
    copy_pos = pos32.repeat_interleave(nA).contiguous()
    copy_tok = cols32.repeat(L).contiguous()
    # the L residue rows of every copy of a chunk: flat rows copy * T + position
    sel = (torch.arange(chunk, dtype=torch.int32, device=dev).unsqueeze(1) * T + pos32.unsqueeze(0)).view(-1).contiguous()
    _, wt = forward_rows(model, tok, pos32, return_logits=True)
    J = torch.empty((L, nA, L, nA), dtype=torch.float32, device=dev)
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        copies = ops.substitute_rows(tok, copy_pos[lo:hi], copy_tok[lo:hi], vocab=V)
        _, logits = forward_rows(model, copies, sel[:(hi - lo) * L], return_logits=True)
        ops.jacobian_scatter(logits, wt, cols32, J, copy0=lo)
    if center:
        ops.jacobian_center(J)
    return J


@torch.no_grad()
def jacobian_contacts(model, tokens, allowed=None, chunk=None, return_jacobian=False):
    """fp32 ``[L, L]`` on the model's device: the contact map of the categorical Jacobian — the centred tensor symmetrised,
    ``S[i, j] = sqrt(sum_ab (0.5 (Jc[i, a, j, b] + Jc[j, b, i, a]))^2)``, its diagonal set to zero, the average product
    correction ``S[i, j] - r_i c_j / s`` and the diagonal zero again.  The arguments are ``categorical_jacobian``'s;
    ``return_jacobian``: also the centred tensor fp32 ``[L, nA, L, nA]`` (it is ``ops.jacobian_center`` of the raw one)."""
    from . import ops

    Jc = categorical_jacobian(model, tokens, allowed=allowed, chunk=chunk, center=True)
    C = ops.apc(ops.jacobian_contacts(Jc))
    return (C, Jc) if return_jacobian else C
