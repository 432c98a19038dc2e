"""Drawing sequences from the masked language model on the MI355X engine: Gibbs sweeps around a starting sequence
(``gibbs_sample`` — the proposal step of the reference's ``examples/lm-design``: mask a position, ``log_softmax`` of the
logits, temper and restrict them, draw a token; utils/lm.py:20-58, utils/sampling.py:138-201) and filling the <mask>
positions of a scaffold (``inpaint``).  The structure-energy term of lm-design and its Metropolis-Hastings acceptance are
not built: every draw is committed.

A sampling step is four engine calls on one stream — nothing is fetched by the host and no ``[B, T, V]`` tensor is built:

    esmk_op_mask_rows_multi    the chains still at work, this step's positions of every chain masked
    esmk_forward_rows          the layer stack; head + log-softmax on the masked rows only
    esmk_op_sample_rows        one token per row (tempered inverse-CDF draw or argmax)
    esmk_op_commit_tokens      tokens[chain, position] = token

The order in which a chain visits its positions is a shuffle of its list per epoch (``esmk_op_permute_positions``).  Every
random number is a Philox4x32-10 word addressed by the key ``seed`` and the counter (chain id, epoch or step, purpose, index):

    permutation   (chain_id, epoch, 0, i)                          i: the Fisher-Yates index
    token draw    (chain_id, epoch * STEP_STRIDE + s, 1, j)        s: step inside the epoch, j: index inside the chain's step

and every kernel of the forward is batch-invariant bit for bit, so a chain follows the same trajectory alone and inside any
batch: ``chain_ids`` names the chains, not their place in the batch.  Chains of different lengths finish an epoch at different
steps; the ones that are done leave the batch until the next epoch begins.

The functions are also methods of ``ESM2`` / ``ProteinBertModel``.  They refuse the MSA Transformer (``NotImplementedError``),
and token-packed chains, nucleus / top-p filtering and confidence-ordered unmasking are not built.
"""
import torch

from .scoring import _device_tokens, _refuse_msa, forward_rows

STEP_STRIDE = 1 << 20  # counter word 1 of a token draw = epoch * STEP_STRIDE + step inside the epoch
STANDARD_RESIDUES = "ACDEFGHIKLMNPQRSTVWY"
TRAJECTORY_FIELDS = ("chain", "step", "pos", "token", "logq", "u", "logprobs")


def allowed_mask(model, allowed=None):
    """The bitset over the vocabulary ``esmk_op_sample_rows`` takes, as a Python int.  ``allowed``: None = the 20 standard
    residues of the model's alphabet; a string of residue letters; or an iterable of tokens (str) / token indices (int)."""
    alphabet = model.alphabet
    V = model.alphabet_size
    if V > 64:
        raise ValueError(f"an alphabet of {V} tokens does not fit the 64-bit candidate set of esmk_op_sample_rows")
    if allowed is None:
        allowed = STANDARD_RESIDUES
    mask = 0
    for a in allowed:
        idx = alphabet.get_idx(a) if isinstance(a, str) else int(a)
        if isinstance(a, str) and a not in alphabet.tok_to_idx:
            raise ValueError(f"allowed: {a!r} is not a token of the model's alphabet")
        if not 0 <= idx < V:
            raise ValueError(f"allowed: token index {idx} is outside [0, {V})")
        mask |= 1 << idx
    if mask == 0:
        raise ValueError("allowed: the candidate set is empty")
    return mask


def _residue_positions(model, tok_cpu):
    """Per chain the token positions of its residues: no <cls> / <eos> the alphabet adds, no <pad>."""
    want = tok_cpu.ne(model.padding_idx)
    if model.prepend_bos:
        want[:, 0] = False
    if model.append_eos:
        want &= tok_cpu.ne(model.eos_idx)
    return [row.nonzero().view(-1).tolist() for row in want]


def _position_lists(model, tok_cpu, positions):
    """``positions`` of ``gibbs_sample`` -> one ascending list of distinct token positions per chain (host)."""
    B, T = tok_cpu.shape
    if positions is None:
        return _residue_positions(model, tok_cpu)
    if torch.is_tensor(positions) and positions.dtype == torch.bool:
        if tuple(positions.shape) != (B, T):
            raise ValueError(f"positions mask of shape {tuple(positions.shape)} for tokens of shape {(B, T)}")
        lists = [row.nonzero().view(-1).tolist() for row in positions.cpu()]
    else:
        positions = positions.tolist() if torch.is_tensor(positions) else list(positions)
        flat = not positions or not hasattr(positions[0], "__iter__")
        lists = [positions] * B if flat else positions
        if len(lists) != B:
            raise ValueError(f"{len(lists)} position lists for {B} chains")
        lists = [sorted({int(p) for p in ps}) for ps in lists]
    special = {model.padding_idx}
    if model.prepend_bos:
        special.add(model.cls_idx)
    if model.append_eos:
        special.add(model.eos_idx)
    for b, ps in enumerate(lists):
        for p in ps:
            if not 0 <= p < T:
                raise ValueError(f"position {p} of chain {b} is outside [0, {T})")
            if int(tok_cpu[b, p]) in special:
                raise ValueError(f"position {p} of chain {b} holds <cls>, <eos> or <pad>: it cannot be redesigned")
    return lists


class _Plan:
    """The index tables of one epoch, the same for every epoch (they depend on the list lengths only), built on the host and
    uploaded ONCE.  The draws of an epoch are laid out step-major, inside a step chain-major, inside a chain in the order of
    the chain's shuffled list: draw r of the epoch is element ``order[r]`` of the chain-major shuffled list."""

    def __init__(self, lengths, per_step, T, chain_ids, dev):
        k = per_step
        starts = [0]
        for n in lengths:
            starts.append(starts[-1] + n)
        self.total = starts[-1]
        self.n_steps = max((n + k - 1) // k for n in lengths) if lengths else 0
        order, slot, index, copy, src, off = [], [], [], [], [], []
        self.steps = []  # (first draw, last draw, first copy, last copy): slices of the tables below
        for s in range(self.n_steps):
            r0, c0 = len(order), len(src)
            for b, n in enumerate(lengths):
                lo, hi = s * k, min((s + 1) * k, n)
                if hi <= lo:
                    continue  # this chain has finished its epoch
                off.append(len(order))
                for j in range(hi - lo):
                    order.append(starts[b] + lo + j)
                    slot.append(b)
                    index.append(j)
                    copy.append(len(src) - c0)
                src.append(b)
            off.append(len(order))  # every step owns n_active + 1 offsets
            self.steps.append((r0, len(order), c0, len(src)))

        def i32(x):
            return torch.tensor(x, dtype=torch.int32).to(dev)

        self.pos_off = i32(starts)
        self.order = torch.tensor(order, dtype=torch.int64).to(dev)
        self.slot, self.index, self.src, self.off = i32(slot), i32(index), i32(src), i32(off)
        self.copy_row0 = i32(copy) * T  # first flat row of the draw's masked copy
        self.chain = chain_ids[self.slot.long()].contiguous()  # counter word 0 of every draw


def _check_common(per_step, temperature, chain_ids, B, dev):
    if int(per_step) <= 0:
        raise ValueError("per_step must be positive")
    temperature = float(temperature)
    if not temperature >= 0.0 or temperature == float("inf"):
        raise ValueError("temperature must be finite and not negative (0: greedy)")
    if chain_ids is None:
        ids = torch.arange(B, dtype=torch.int32)
    else:
        ids = torch.as_tensor(chain_ids).to(torch.int64).view(-1).cpu()
        if ids.numel() != B:
            raise ValueError(f"{ids.numel()} chain ids for {B} chains")
        if bool(((ids < 0) | (ids >= 2 ** 31)).any()):
            raise ValueError("chain ids must lie in [0, 2^31)")
        ids = ids.to(torch.int32)
    return int(per_step), (1.0 / temperature if temperature > 0.0 else 0.0), ids.to(dev)


def _run(model, state, lists, epochs, per_step, inv_temperature, mask, force_new, seed, chain_ids, return_trajectory):
    """The step loop: ``state`` int64 [B, T] on the device is updated in place.  Nothing inside the loop waits for the device."""
    from . import ops

    dev = state.device
    B, T = state.shape
    plan = _Plan([len(ps) for ps in lists], per_step, T, chain_ids, dev)
    if plan.n_steps > STEP_STRIDE:
        raise ValueError(f"{plan.n_steps} steps per epoch: the counter layout holds at most {STEP_STRIDE}")
    if epochs * STEP_STRIDE >= 2 ** 31:
        raise ValueError(f"{epochs} epochs: the counter layout holds fewer than {2 ** 31 // STEP_STRIDE}")
    pos_in = torch.tensor([p for ps in lists for p in ps], dtype=torch.int32).to(dev)
    flat_state = state.view(-1)
    traj = {name: [] for name in TRAJECTORY_FIELDS}
    for epoch in range(epochs if plan.total else 0):
        perm = ops.permute_positions(plan.pos_off, pos_in, chain_ids, seed=seed, epoch=epoch)
        pos = perm[plan.order]  # the epoch's draws, step-major
        for s, (r0, r1, c0, c1) in enumerate(plan.steps):
            step = epoch * STEP_STRIDE + s
            step_pos = pos[r0:r1]
            masked = ops.mask_rows_multi(state, plan.off[c0 + s: c1 + s + 1], pos, plan.src[c0:c1], model.mask_idx)
            lp = forward_rows(model, masked, plan.copy_row0[r0:r1] + step_pos)
            slot = plan.slot[r0:r1]
            exclude = None
            if force_new:  # the token this draw replaces gets no mass
                exclude = flat_state[slot.long() * T + step_pos.long()].to(torch.int32)
            token, logq, u = ops.sample_rows(lp, plan.chain[r0:r1], plan.index[r0:r1], mask, inv_temperature, seed=seed,
                                             step=step, exclude=exclude, want_u=return_trajectory)
            ops.commit_tokens(state, slot, step_pos, token)
            if return_trajectory:
                for name, value in zip(TRAJECTORY_FIELDS, (plan.chain[r0:r1], torch.full_like(token, step), step_pos, token,
                                                           logq, u, lp)):
                    traj[name].append(value)
    if not return_trajectory:
        return state
    V = model.alphabet_size
    empty = dict(chain=torch.int32, step=torch.int32, pos=torch.int32, token=torch.int32, logq=torch.float32, u=torch.float32)
    out = {}
    for name in TRAJECTORY_FIELDS:
        if traj[name]:
            out[name] = torch.cat(traj[name])
        elif name == "logprobs":
            out[name] = torch.empty((0, V), dtype=torch.float32, device=dev)
        else:
            out[name] = torch.empty((0,), dtype=empty[name], device=dev)
    return state, out


@torch.no_grad()
def gibbs_sample(model, tokens, sweeps, per_step=1, positions=None, temperature=1.0, allowed=None, force_new=False, seed=0,
                 chain_ids=None, return_trajectory=False):
    """Gibbs sampling around ``tokens`` int64 ``[B, T]`` (padded as for ``forward``; every row is a chain): the final tokens
    ``[B, T]`` on the model's device.

    sweeps       epochs: in every one each chain visits all of its designable positions once, in a fresh random order, cut
                 into steps of ``per_step`` positions.  In a step the chosen positions of every chain are masked together, ONE
                 batched forward gives their log-probabilities, one token per position is drawn and written back.
    positions    the designable token positions: None = the residues of every chain (never <cls>, <eos>, <pad>); a bool mask
                 [B, T]; one iterable of ints (the same in every chain) or one iterable per chain.
    temperature  the draw is from softmax(log_softmax(logits) / temperature) over the candidates; 0: the argmax.
    allowed      the candidate tokens (``allowed_mask``); default the 20 standard residues.
    force_new    the token a draw replaces is no candidate (the reference's ``force_propose_new_tokens``).
    seed         the Philox key, in [0, 2^64); ``chain_ids`` (default ``arange(B)``): counter word 0 of every chain.  A chain
                 draws the same trajectory whatever batch it runs in.
    return_trajectory  also a dict of device tensors, one entry per draw in the order drawn (step-major, chain-major inside a
                 step): ``chain``, ``step`` (epoch * STEP_STRIDE + step inside the epoch), ``pos``, ``token`` int32, ``logq``
                 (log-probability of the token under the distribution it was drawn from), ``u`` fp32, and ``logprobs`` fp32
                 [n, V]: the row every draw saw."""
    _refuse_msa(model)
    if int(sweeps) < 0:
        raise ValueError("sweeps must not be negative")
    tok = _device_tokens(model, tokens)
    per_step, inv_t, ids = _check_common(per_step, temperature, chain_ids, tok.shape[0], tok.device)
    lists = _position_lists(model, tok.cpu(), positions)
    return _run(model, tok.clone(), lists, int(sweeps), per_step, inv_t, allowed_mask(model, allowed), bool(force_new), seed, ids,
                return_trajectory)


@torch.no_grad()
def inpaint(model, tokens, per_step=1, temperature=1.0, allowed=None, seed=0, chain_ids=None, return_trajectory=False):
    """Fill the <mask> positions of ``tokens`` int64 ``[B, T]``: the final tokens ``[B, T]`` on the model's device.  One epoch
    over the <mask> positions of every chain in a random order, ``per_step`` at a time; positions not yet visited stay <mask>
    in the state, so every draw sees what was committed before it and the last step a fully committed context.  The other
    arguments and the trajectory are those of ``gibbs_sample``."""
    _refuse_msa(model)
    tok = _device_tokens(model, tokens)
    per_step, inv_t, ids = _check_common(per_step, temperature, chain_ids, tok.shape[0], tok.device)
    lists = [row.nonzero().view(-1).tolist() for row in tok.cpu().eq(model.mask_idx)]
    return _run(model, tok.clone(), lists, 1, per_step, inv_t, allowed_mask(model, allowed), False, seed, ids, return_trajectory)
