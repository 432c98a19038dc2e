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

``top_k`` / ``top_p`` put a filter in front of every draw (``esmk_op_sample_rows_ex``): the candidates are ranked by their
log-probability, and only the ``top_k`` best, and of those only the ranks whose preceding mass is below ``top_p`` of the total
(the nucleus), are drawn from; the best candidate always stays.  With both off (0 and 1.0, the defaults) the calls and the bits
are those of the plain draw.

``inpaint(order="confidence" | "entropy")`` unmasks the most confident positions first instead of a random order.  At step s
every chain still at work has its remaining <mask> positions in the state, and the step is

    esmk_forward_rows          head + log-softmax on ALL remaining <mask> rows of the chains still at work
    esmk_op_sample_rows_ex     a token and a score per row: max log q ("confidence") or sum q log q ("entropy")
    esmk_op_select_rows        per chain the min(per_step, remaining) rows of the largest score, best first; the others
    esmk_op_commit_tokens      the chosen rows' tokens; the others are the next step's row list

    token draw    (chain_id, s, 1, token position)      the position is the index: a draw does not depend on how many rows
                                                        a step has

The host knows every COUNT in advance (a chain of n holes has n - s * per_step left at step s) and uploads the offset tables
once; it never learns WHICH positions were chosen.  Chains that are done leave the batch.

The functions are also methods of ``ESM2`` / ``ProteinBertModel``.  They refuse the MSA Transformer (``NotImplementedError``),
and token-packed chains are not built.
"""
import torch

from .scoring import _device_tokens, _refuse_msa, forward_rows

STEP_STRIDE = 1 << 20  # counter word 1 of a token draw = epoch * STEP_STRIDE + step inside the epoch
STANDARD_RESIDUES = "ACDEFGHIKLMNPQRSTVWY"
TRAJECTORY_FIELDS = ("chain", "step", "pos", "token", "logq", "u", "logprobs")
ORDERS = ("random", "confidence", "entropy")


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


def _check_filters(top_k, top_p):
    from . import ops

    return ops.check_filters(top_k, top_p)


def _run(model, state, lists, epochs, per_step, inv_temperature, mask, force_new, seed, chain_ids, return_trajectory, top_k=0,
         top_p=1.0):
    """The step loop: ``state`` int64 [B, T] on the device is updated in place.  Nothing inside the loop waits for the device.
    A filter (``top_k`` != 0 or ``top_p`` < 1) makes the draw ``esmk_op_sample_rows_ex`` and adds ``kept`` to the trajectory."""
    from . import ops

    filtered = top_k != 0 or top_p < 1.0
    dev = state.device
    B, T = state.shape
    plan = _Plan([len(ps) for ps in lists], per_step, T, chain_ids, dev)
    if plan.n_steps > STEP_STRIDE:
        raise ValueError(f"{plan.n_steps} steps per epoch: the counter layout holds at most {STEP_STRIDE}")
    if epochs * STEP_STRIDE >= 2 ** 31:
        raise ValueError(f"{epochs} epochs: the counter layout holds fewer than {2 ** 31 // STEP_STRIDE}")
    pos_in = torch.tensor([p for ps in lists for p in ps], dtype=torch.int32).to(dev)
    flat_state = state.view(-1)
    fields = TRAJECTORY_FIELDS + (("kept",) if filtered else ())
    traj = {name: [] for name in fields}
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
            kept = None
            if filtered:
                token, logq, u, _, kept = ops.sample_rows_ex(lp, plan.chain[r0:r1], plan.index[r0:r1], mask, inv_temperature,
                                                             seed=seed, step=step, exclude=exclude, want_u=return_trajectory,
                                                             top_k=top_k, top_p=top_p, want_kept=return_trajectory)
            else:
                token, logq, u = ops.sample_rows(lp, plan.chain[r0:r1], plan.index[r0:r1], mask, inv_temperature, seed=seed,
                                                 step=step, exclude=exclude, want_u=return_trajectory)
            ops.commit_tokens(state, slot, step_pos, token)
            if return_trajectory:
                for name, value in zip(fields, (plan.chain[r0:r1], torch.full_like(token, step), step_pos, token, logq, u, lp,
                                                kept)):
                    traj[name].append(value)
    if not return_trajectory:
        return state
    return state, _joined(traj, model.alphabet_size, dev)


_FIELD_DTYPES = dict(chain=torch.int32, step=torch.int32, pos=torch.int32, token=torch.int32, logq=torch.float32,
                     u=torch.float32, score=torch.float32, kept=torch.int64)


def _joined(traj, V, dev):
    """The per-step lists of a trajectory as one tensor per field (an empty one of the field's type when nothing was drawn)."""
    out = {}
    for name, parts in traj.items():
        if parts:
            out[name] = torch.cat(parts)
        elif name == "logprobs":
            out[name] = torch.empty((0, V), dtype=torch.float32, device=dev)
        else:
            out[name] = torch.empty((0,), dtype=_FIELD_DTYPES[name], device=dev)
    return out


class _OrderedPlan:
    """The offset tables of confidence-ordered unmasking, built on the host from the hole counts alone and uploaded ONCE.  At
    step s a chain of n holes has ``n - s * per_step`` rows left, commits ``min(per_step, left)`` of them and hands the others
    on; the chains with rows left are the step's batch, in chain order.  Every step owns a slice of ``n_active + 1`` offsets in
    ``row_off`` (its rows, chain-major), ``sel_off`` (the committed ones) and ``rest_off`` (the next step's rows)."""

    def __init__(self, lengths, per_step, chain_ids, dev):
        k = per_step
        self.n_steps = max((n + k - 1) // k for n in lengths) if lengths else 0
        self.steps = []  # (first offset, n_active, rows, committed, left over)
        row_off, sel_off, rest_off, src, left = [], [], [], [], []
        for s in range(self.n_steps):
            o0 = len(row_off)
            rows = sel = rest = 0
            for b, n in enumerate(lengths):
                have = n - s * k
                if have <= 0:
                    continue  # this chain is done: it leaves the batch
                row_off.append(rows), sel_off.append(sel), rest_off.append(rest)
                src.append(b), left.append(have)
                rows, sel, rest = rows + have, sel + min(k, have), rest + have - min(k, have)
            row_off.append(rows), sel_off.append(sel), rest_off.append(rest)
            self.steps.append((o0, len(row_off) - o0 - 1, rows, sel, rest))

        def i32(x):
            return torch.tensor(x, dtype=torch.int32).to(dev)

        self.row_off, self.sel_off, self.rest_off = i32(row_off), i32(sel_off), i32(rest_off)
        self.src = torch.tensor(src, dtype=torch.int64).to(dev)  # per step its active chains: slice [o0 - s : o0 - s + n_active]
        self.left = torch.tensor(left, dtype=torch.int64).to(dev)  # ... and the rows each of them has left
        self.chain = chain_ids[self.src].contiguous()


def _run_ordered(model, state, lists, per_step, inv_temperature, mask, seed, chain_ids, return_trajectory, top_k, top_p, order):
    """Confidence-ordered unmasking: ``state`` int64 [B, T] on the device, its <mask> positions ``lists``, is filled in place.
    Nothing inside the loop waits for the device: which rows a step commits is device data from ``esmk_op_select_rows``."""
    from . import ops

    dev = state.device
    B, T = state.shape
    plan = _OrderedPlan([len(ps) for ps in lists], per_step, chain_ids, dev)
    if plan.n_steps > STEP_STRIDE:
        raise ValueError(f"{plan.n_steps} steps: the counter layout holds at most {STEP_STRIDE}")
    fields = TRAJECTORY_FIELDS + ("score", "kept")
    traj = {name: [] for name in fields}
    scored = {name: [] for name in ("chain", "step", "pos", "score")}
    pos = torch.tensor([p for ps in lists for p in ps], dtype=torch.int32).to(dev)  # the rows of step 0: chain-major, ascending
    for s, (o0, n_active, n_rows, n_sel, n_rest) in enumerate(plan.steps):
        a0 = o0 - s  # every earlier step owns one offset more than it has chains
        src, left = plan.src[a0: a0 + n_active], plan.left[a0: a0 + n_active]
        local = torch.repeat_interleave(torch.arange(n_active, device=dev), left, output_size=n_rows)  # row -> chain of the step
        batch = state if n_active == B else state.index_select(0, src)
        lp = forward_rows(model, batch, (local * T + pos).to(torch.int32))
        chain = plan.chain[a0: a0 + n_active][local].contiguous()
        token, logq, u, score, kept = ops.sample_rows_ex(lp, chain, pos, mask, inv_temperature, seed=seed, step=s,
                                                         want_u=return_trajectory, top_k=top_k, top_p=top_p, score=order,
                                                         want_kept=return_trajectory)
        sel, rest = ops.select_rows(score, plan.row_off[o0: o0 + n_active + 1], plan.sel_off[o0: o0 + n_active + 1],
                                    plan.rest_off[o0: o0 + n_active + 1], n_sel=n_sel, n_rest=n_rest)
        pick = sel.long()
        ops.commit_tokens(state, src[local[pick]].to(torch.int32), pos[pick], token[pick])
        if return_trajectory:
            for name, value in zip(fields, (chain[pick], torch.full_like(sel, s), pos[pick], token[pick], logq[pick], u[pick],
                                            lp[pick], score[pick], kept[pick])):
                traj[name].append(value)
            for name, value in zip(scored, (chain, torch.full_like(pos, s), pos, score)):
                scored[name].append(value)
        if rest is not None:
            pos = pos[rest.long()]
    if not return_trajectory:
        return state
    out = _joined(traj, model.alphabet_size, dev)
    out["scored"] = _joined(scored, model.alphabet_size, dev)
    return state, out


@torch.no_grad()
def gibbs_sample(model, tokens, sweeps, per_step=1, positions=None, temperature=1.0, allowed=None, force_new=False, seed=0,
                 chain_ids=None, return_trajectory=False, top_k=0, top_p=1.0, order="random"):
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
                 [n, V]: the row every draw saw.  With a filter also ``kept`` int64: the kept set of every draw as a bitset.
    top_k, top_p the filter in front of every draw: only the ``top_k`` most probable candidates (0: all), and of those only the
                 ranks whose preceding probability mass is below ``top_p`` (1.0: all); the best candidate always stays.  The
                 draw, and ``logq``, are relative to what is kept.
    order        only "random": between sweeps nothing is masked, so a confidence order has no meaning here (``inpaint``)."""
    _refuse_msa(model)
    if int(sweeps) < 0:
        raise ValueError("sweeps must not be negative")
    if order != "random":
        if order not in ORDERS:
            raise ValueError(f"order {order!r}: one of {ORDERS}")
        raise ValueError(f"order {order!r}: a Gibbs sweep revisits committed positions, only inpaint can unmask by confidence")
    top_k, top_p = _check_filters(top_k, top_p)
    tok = _device_tokens(model, tokens)
    per_step, inv_t, ids = _check_common(per_step, temperature, chain_ids, tok.shape[0], tok.device)
    lists = _position_lists(model, tok.cpu(), positions)
    return _run(model, tok.clone(), lists, int(sweeps), per_step, inv_t, allowed_mask(model, allowed), bool(force_new), seed, ids,
                return_trajectory, top_k, top_p)


@torch.no_grad()
def inpaint(model, tokens, per_step=1, temperature=1.0, allowed=None, seed=0, chain_ids=None, return_trajectory=False, top_k=0,
            top_p=1.0, order="random"):
    """Fill the <mask> positions of ``tokens`` int64 ``[B, T]``: the final tokens ``[B, T]`` on the model's device.  One epoch
    over the <mask> positions of every chain in a random order, ``per_step`` at a time; positions not yet visited stay <mask>
    in the state, so every draw sees what was committed before it and the last step a fully committed context.  The other
    arguments and the trajectory are those of ``gibbs_sample``.

    order        "random" (above); "confidence" / "entropy": most confident first.  Every step scores ALL remaining <mask>
                 positions of a chain — a token is drawn for each (filter and temperature as given; Philox counter (chain id,
                 step, 1, token position)) and the row's score is max log q ("confidence") or sum q log q ("entropy": the
                 negative entropy) of its tempered distribution over the candidates before filtering — and commits the
                 ``per_step`` rows of the largest score (ties: the lower position); the other draws are dropped and their
                 positions scored again in the next step's context.  ``temperature=0`` is fully deterministic.
    trajectory   with such an order: one entry per COMMITTED draw (step-major, chain-major, best first) with the fields above
                 plus ``score`` fp32 and ``kept`` int64, and ``scored``: a dict ``chain``, ``step``, ``pos``, ``score`` with
                 one entry per row scored at every step (step-major, chain-major, ascending position)."""
    _refuse_msa(model)
    if order not in ORDERS:
        raise ValueError(f"order {order!r}: one of {ORDERS}")
    top_k, top_p = _check_filters(top_k, top_p)
    tok = _device_tokens(model, tokens)
    per_step, inv_t, ids = _check_common(per_step, temperature, chain_ids, tok.shape[0], tok.device)
    lists = [row.nonzero().view(-1).tolist() for row in tok.cpu().eq(model.mask_idx)]
    if order != "random":
        return _run_ordered(model, tok.clone(), lists, per_step, inv_t, allowed_mask(model, allowed), seed, ids, return_trajectory,
                            top_k, top_p, order)
    return _run(model, tok.clone(), lists, 1, per_step, inv_t, allowed_mask(model, allowed), False, seed, ids, return_trajectory,
                top_k, top_p)
