"""Design toward a target contact map: Metropolis-Hastings on the engine.

``gibbs_sample`` and ``inpaint`` draw from the model's own conditionals.  The reference's ``examples/lm-design`` steers sequences
toward a structure instead: a uniform single-site proposal, an energy of an LM term plus a structure term, and an acceptance test
under an annealed temperature (``utils/fixedbb.py``).  lm-design's structure model needs a projection checkpoint of its own;
every ESM-2 / ESM-1b / ESM-1 checkpoint carries the contact-regression head, so the structure term here is the cross-entropy
between the predicted contact map and a target map:

    E(x) = w_contact * E_contact(x) + w_lm * E_lm(x)
    E_contact  "pos" (lm-design's choice, ``dist_cce_pos``): -mean of log p_ij over the target contacts; "bce": -mean of
               y log p + (1 - y) log(1 - p); over the pairs i < j with j - i >= min_sep whose target is not "ignore"
    E_lm       the mean negative log-probability of the sequence's own residues in that same UNMASKED forward
               (``wt_marginals``' rows).  lm-design's LM term masks the proposed site; this one costs no second forward.

The energy of the initial state is computed once; after that every step is ONE energy forward, of the proposals, and the
accepted energy stays on the device as the current one (lm-design evaluates both x and x' every step).  A step with
``proposal="uniform"`` is

    esmk_op_propose_mutations    site and token of every chain from Philox counter (chain id, step, 2, 0)
    esmk_op_substitute_rows      the proposed sequences
    esmk_forward_rows_contacts   one forward: the residue rows' log-probabilities and the contact maps, the head-group count of
                                 the contact head pinned to that of B = 1 (include/esmk.h)
    esmk_op_sum_target_rows      fp64 sum of log p(own token) per chain          (w_lm != 0)
    esmk_op_contact_energy       fp64 cross-entropy per chain, fixed order       (w_contact != 0)
    esmk_op_mh_accept            u from counter (chain id, step, 3, 0); token, current energy and components written on acceptance

and ``proposal="lm"`` draws the new token from the model's conditional at the masked site first:

    esmk_op_propose_mutations (the site) -> esmk_op_mask_rows_multi -> esmk_forward_rows -> esmk_op_sample_rows at counter
    (chain id, step, 1, site) -> esmk_op_hastings_rows

The forward and the reverse proposal share the context (the site is masked in both), so the Hastings correction is the one
difference inv_t_prop * (log q(old) - log q(new)) of two log-probabilities of that row.  With ``w_contact=0`` the energy forward is
``esmk_forward_rows`` (no contact head).  The host reads nothing inside the loop; everything is on one stream.  A chain does
the same alone and in any batch: the random numbers depend on (seed, chain id, step) alone, every kernel computes a row from
that row alone, and the contact maps carry the bits of ``predict_contacts`` on that sequence alone.

``w_ngram`` adds lm-design's third term, the n-gram term (``utils/ngram.py``): E = (w_contact * E_contact + w_lm * E_lm) + w_ngram *
E_ngram, E_ngram the sum over the background's orders of the KL divergence between the n-gram frequencies of the sequence and
the background's (``esm_amd.ngram.Background``, counted from sequences of the caller's choice; ``python -m esm_amd.ngram_table``).
It is one more op per step on the proposed sequences, ``esmk_op_ngram_energy``, and the acceptance becomes ``esmk_op_mh_accept_ex``.

``replicas=K`` runs the chains as ladders of K consecutive chains at K temperatures (replica exchange).  Chain b starts at rung b % K;
the acceptance reads every chain's temperature from its rung (``esmk_op_mh_accept_ex``), and after every ``swap_every`` steps the chains
at neighbouring rungs of a ladder exchange their rungs with probability min(1, exp((1/T_k - 1/T_k+1) * (E_x - E_y)))
(``esmk_op_replica_swap``: even pairs in even rounds, odd pairs in odd ones; u from counter (chain id of the ladder's first slot,
round, 4, k)).  Temperatures move, sequences and chain ids stay in their slots, and the forward is the one the batch ran anyway.
With ``replicas=None`` and ``w_ngram=0`` the calls, the bits and the return values are those of the loop above.

``target`` may instead be a ``DistogramTarget(bins, head)``: lm-design's own structure term ``dist_cce_pos``, the categorical
cross-entropy between the distance bins a linear projection of the attention maps predicts (``esm_amd.PairHead``, read from
lm-design's projection checkpoint; esm_amd/pair_head.py) and the target's bins over the target's contacts.  The energy forward is
then ``esmk_forward_rows_pair`` and the structure term ``esmk_op_distogram_energy``, in the slot of E_contact everywhere;
``min_sep=0`` gives lm-design's term exactly and ``contact_loss`` is not used.  With any other target nothing changes.

Not built: multi-site proposals, chains of different lengths, token-packed chains, the MSA Transformer (``NotImplementedError``).

    python -m esm_amd.design --model-location esm2_t33_650M_UR50D.pt --target-pdb 1abc.pdb --chain A --num-chains 16 \\
        --steps 2000 --anneal 1.0:0.01 --output designs.fasta --log trajectory.csv
"""
import argparse
import math
import sys

import numpy as np
import torch

from .sampling import _position_lists, allowed_mask
from .scoring import _device_tokens, _refuse_msa, forward_rows

PROPOSALS = ("uniform", "lm")
CONTACT_LOSSES = ("pos", "bce")
TRAJECTORY_FIELDS = ("site", "old", "new", "e_cur", "e_prop", "e_contact", "e_lm", "hastings", "u", "accepted")
NGRAM_FIELDS = ("e_ngram",)  # the trajectory also holds these with w_ngram != 0 ...
REPLICA_FIELDS = ("rung", "swapped", "swap_u")  # ... and these with replicas
IGNORE = 2  # target value of a pair that does not count

_THREE_TO_ONE = {"ALA": "A", "ARG": "R", "ASN": "N", "ASP": "D", "CYS": "C", "GLN": "Q", "GLU": "E", "GLY": "G", "HIS": "H",
                 "ILE": "I", "LEU": "L", "LYS": "K", "MET": "M", "PHE": "F", "PRO": "P", "SER": "S", "THR": "T", "TRP": "W",
                 "TYR": "Y", "VAL": "V", "MSE": "M", "SEC": "U", "PYL": "O"}


def _read_cb(path, chain=None):
    """``(sequence, have bool [S], xyz fp64 [S, 3])`` of one chain of a PDB file: the one-letter sequence of its residues in file
    order and the C-beta atom (C-alpha for glycine) of each, ``have`` False (and a zero position) where a residue lacks it.  Plain
    ATOM records of the first model; ``chain`` None: the first chain of the file; of alternate locations the first one seen."""
    order, atoms, names = [], {}, {}
    with open(path) as fh:
        for line in fh:
            rec = line[:6]
            if rec.startswith("ENDMDL"):
                break
            if rec != "ATOM  " or len(line) < 54:
                continue
            ch = line[21]
            if chain is None:
                chain = ch
            if ch != chain:
                continue
            key = (line[22:26], line[26])
            res = line[17:20].strip()
            if key not in names:
                names[key] = res
                order.append(key)
            atom = line[12:16].strip()
            if atom == ("CA" if res == "GLY" else "CB") and key not in atoms:
                atoms[key] = (float(line[30:38]), float(line[38:46]), float(line[46:54]))
    if not order:
        raise ValueError(f"{path}: no ATOM record of chain {chain!r}")
    S = len(order)
    seq = "".join(_THREE_TO_ONE.get(names[k], "X") for k in order)
    have = np.array([k in atoms for k in order])
    xyz = np.array([atoms.get(k, (0.0, 0.0, 0.0)) for k in order], dtype=np.float64).reshape(S, 3)
    return seq, have, xyz


def contacts_from_pdb(path, chain=None, cutoff=8.0):
    """``(sequence, target)`` of one chain of a PDB file: the one-letter sequence of its residues in file order and the uint8
    ``[S, S]`` target map — 1 where the C-beta atoms (C-alpha for glycine) of two residues are closer than ``cutoff`` angstrom, 0
    where they are not, 2 (ignore) in the row and column of a residue that lacks the atom.  Plain ATOM records of the first
    model; ``chain`` None: the first chain of the file; of alternate locations the first one seen counts.  numpy only."""
    seq, have, xyz = _read_cb(path, chain)
    dist = np.sqrt(((xyz[:, None, :] - xyz[None, :, :]) ** 2).sum(-1))
    target = (dist < float(cutoff)).astype(np.uint8)
    target[~have, :] = IGNORE
    target[:, ~have] = IGNORE
    return seq, target


def target_map(target, S=None):
    """``target`` of ``design`` as a uint8 ``[S, S]`` CPU tensor of 0 / 1 / 2: a bool array (True = contact), a uint8 / integer
    array of those three values, or a floating array of probabilities or distances-turned-scores thresholded at 0.5 (> 0.5 =
    contact) with NaN meaning ignore."""
    t = torch.as_tensor(np.asarray(target) if not torch.is_tensor(target) else target).cpu()
    if t.ndim != 2 or t.shape[0] != t.shape[1]:
        raise ValueError(f"target: a square [S, S] map, got shape {tuple(t.shape)}")
    if S is not None and t.shape[0] != S:
        raise ValueError(f"target is a map of {t.shape[0]} residues but the chains have {S}: all chains have the target's length")
    if t.dtype == torch.bool:
        return t.to(torch.uint8).contiguous()
    if t.is_floating_point():
        out = (t > 0.5).to(torch.uint8)
        out[torch.isnan(t)] = IGNORE
        return out.contiguous()
    if bool(((t < 0) | (t > 2)).any()):
        raise ValueError("target: integer maps hold 0 (no contact), 1 (contact) or 2 (ignore)")
    return t.to(torch.uint8).contiguous()


class DistogramTarget:
    """lm-design's structure term ``dist_cce_pos`` as the ``target`` of ``design`` / ``design_energy``: the categorical
    cross-entropy (examples/lm-design/utils/loss.py:10-29) between the distance bins a ``PairHead`` predicts from the attention
    maps and the target's bins, over the target's contacts — the pairs whose bin is <= ``contact_cutoff_bin``
    (struct_models.py:35; lm_design.py:254-280); every other pair, and every pair whose bin is 255, is ignored.

    bins         uint8 ``[S, S]`` distance bins (``esm_amd.distogram_bins``, ``distogram_from_pdb``)
    head         the ``esm_amd.PairHead`` (``PairHead.from_linear_projection``)
    output       the head's output that holds the distance logits
    temperature  the logits are divided by it before the softmax

    The term comes from ``esmk_forward_rows_pair`` + ``esmk_op_distogram_energy`` and takes the slot of the contact term
    everywhere: ``w_contact`` weighs it, ``e_contact`` names it in the trajectory and the log.  ``min_sep=0`` gives lm-design's
    term exactly (the mean over ALL ordered pairs that count); ``contact_loss`` is ignored with this target."""

    def __init__(self, bins, head, output="dist", contact_cutoff_bin=5, temperature=1.0):
        from .pair_head import IGNORE_BIN, PairHead

        if not isinstance(head, PairHead):
            raise TypeError("DistogramTarget: head must be an esm_amd.PairHead")
        if output not in head.outputs:
            raise ValueError(f"DistogramTarget: the head has no output {output!r} (it has {sorted(head.outputs)})")
        b = torch.as_tensor(np.asarray(bins) if not torch.is_tensor(bins) else bins).cpu()
        if b.ndim != 2 or b.shape[0] != b.shape[1] or b.is_floating_point() or b.dtype == torch.bool:
            raise ValueError(f"DistogramTarget: bins is an integer [S, S] map of distance bins, got {b.dtype} {tuple(b.shape)}")
        self.head, self.output = head, output
        self.first, hi = head.columns(output)
        self.n_bins = hi - self.first
        b = b.to(torch.int64)
        if bool(((b < 0) | ((b >= self.n_bins) & (b != IGNORE_BIN))).any()):
            raise ValueError(f"DistogramTarget: bins hold 0 .. {self.n_bins - 1} or {IGNORE_BIN} (ignore)")
        self.contact_cutoff_bin = int(contact_cutoff_bin)
        self.temperature = float(temperature)
        if not (math.isfinite(self.temperature) and self.temperature > 0.0):
            raise ValueError("DistogramTarget: temperature must be positive and finite")
        counted = torch.where(b <= self.contact_cutoff_bin, b, torch.full_like(b, IGNORE_BIN))
        self.bins = counted.to(torch.uint8).contiguous()  # what esmk_op_distogram_energy takes
        self.S = int(b.shape[0])


def batch_size(bytes_of, n_chains, max_bytes):
    """The number of chains per batch: the chains are cut into the fewest batches of (nearly) equal size whose workspace
    ``bytes_of(B)`` (growing with B) fits ``max_bytes``.  ValueError when one chain alone does not fit."""
    n_chains, max_bytes = int(n_chains), int(max_bytes)
    if n_chains <= 0:
        raise ValueError("there are no chains")
    if bytes_of(1) > max_bytes:
        raise ValueError(f"max_bytes = {max_bytes}: the energy forward of one chain alone takes {bytes_of(1)} bytes of workspace")
    lo, hi = 1, n_chains  # bytes_of(lo) fits
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if bytes_of(mid) <= max_bytes:
            lo = mid
        else:
            hi = mid - 1
    n_batches = (n_chains + lo - 1) // lo
    return (n_chains + n_batches - 1) // n_batches


def inverse_temperatures(temperature, steps):
    """Per step 1 / T as a float (``inf`` for T = 0: greedy) from a float or a length-``steps`` sequence of temperatures."""
    if isinstance(temperature, (int, float)):
        temps = [float(temperature)] * steps
    else:
        temps = [float(t) for t in (temperature.tolist() if hasattr(temperature, "tolist") else temperature)]
        if len(temps) != steps:
            raise ValueError(f"{len(temps)} temperatures for {steps} steps")
    for t in temps:
        if not t >= 0.0 or t == float("inf"):
            raise ValueError("temperatures must be finite and not negative (0: greedy)")
    return [1.0 / t if t > 0.0 else float("inf") for t in temps]


def ladder_inverse_temperatures(temperature, steps, K):
    """fp64 ``[steps, K]`` of 1 / T from a length-``K`` ladder (rung 0 first) or ``steps`` such ladders.  Every temperature is
    positive and finite: a ladder has no greedy rung."""
    t = np.asarray(temperature.tolist() if hasattr(temperature, "tolist") else temperature, dtype=np.float64)
    if t.shape == (K,):
        t = np.broadcast_to(t, (steps, K))
    elif t.shape != (steps, K):
        raise ValueError(f"temperature with replicas = {K}: a ladder of {K} temperatures or {steps} of them, got shape {t.shape}")
    if not bool((np.isfinite(t) & (t > 0.0)).all()):
        raise ValueError("the temperatures of a ladder must be positive and finite (a ladder has no greedy rung)")
    return np.ascontiguousarray(1.0 / t)


class _Setup:
    """Everything the host checks and decides before a device is asked for."""

    def __init__(self, model, tokens, target, w_contact, w_lm, contact_loss, min_sep, w_ngram=0.0, ngram=None):
        _refuse_msa(model)
        self.w_ngram = float(w_ngram)
        if not math.isfinite(self.w_ngram):
            raise ValueError("w_ngram must be finite")
        if self.w_ngram != 0.0 and ngram is None:
            raise ValueError("w_ngram != 0 needs ngram: an esm_amd.ngram.Background (Background.from_sequences, Background.load)")
        self.ngram = ngram if self.w_ngram != 0.0 else None  # (w_ngram = 0: the term does not run)
        if tokens.ndim == 1:
            tokens = tokens.unsqueeze(0)
        if tokens.ndim != 2:
            raise ValueError("tokens: [B, T] (or [T])")
        self.tok_cpu = tokens.detach().cpu().to(torch.int64)
        self.B, self.T = self.tok_cpu.shape
        self.bos, self.eos = int(bool(model.prepend_bos)), int(bool(model.append_eos))
        self.S = self.T - self.bos - self.eos
        if self.B == 0 or self.S <= 0:
            raise ValueError("tokens: no chain, or no residue between <cls> and <eos>")
        if bool(self.tok_cpu.eq(model.padding_idx).any()):
            raise ValueError("tokens hold <pad>: all chains have the target's length, padded chains are not built")
        self.w_contact, self.w_lm = float(w_contact), float(w_lm)
        if not (math.isfinite(self.w_contact) and math.isfinite(self.w_lm)):
            raise ValueError("w_contact and w_lm must be finite")
        if self.w_contact == 0.0 and self.w_lm == 0.0:
            raise ValueError("w_contact and w_lm are both 0: there is no energy")
        if contact_loss not in CONTACT_LOSSES:
            raise ValueError(f"contact_loss {contact_loss!r}: one of {CONTACT_LOSSES}")
        self.contact_loss = contact_loss
        self.min_sep = int(min_sep)
        self.disto = None
        if isinstance(target, DistogramTarget):  # the distogram term in the contact term's slot (contact_loss is not used)
            if self.min_sep < 0:
                raise ValueError("min_sep must not be negative")
            if target.S != self.S:
                raise ValueError(f"target holds bins of {target.S} residues but the chains have {self.S}: all chains have the "
                                 "target's length")
            target.head.check_model(model)
            self.target = None
            self.disto = target if self.w_contact != 0.0 else None
        elif self.min_sep < 1:
            raise ValueError("min_sep must be at least 1")
        elif target is None:
            if self.w_contact != 0.0:
                raise ValueError("target=None needs w_contact=0")
            self.target = None
        else:
            checked = target_map(target, self.S)
            self.target = checked if self.w_contact != 0.0 else None  # (w_contact = 0: no contact head runs)
        if model.alphabet_size > 64:
            raise ValueError(f"an alphabet of {model.alphabet_size} tokens does not fit the 64-bit candidate sets of the engine")


class _Energy:
    """The energy forward of a batch of equally long sequences on the device and its two terms."""

    def __init__(self, model, setup, dev):
        self.model, self.su, self.dev = model, setup, dev
        self.target = None if setup.target is None else setup.target.to(dev)
        self.bins = None if setup.disto is None else setup.disto.bins.to(dev)
        self.V = model.alphabet_size
        self._tables = {}
        self.ngram_code = self.ngram_q = None
        if setup.ngram is not None:
            code = np.full((self.V,), -1, dtype=np.int32)
            known = setup.ngram.token_codes(model.alphabet)[: self.V]
            code[: known.shape[0]] = known
            self.ngram_code = torch.from_numpy(code).to(dev)
            self.ngram_q = {n: torch.from_numpy(q).to(dev) for n, q in setup.ngram.tables.items()}

    def bytes_of(self, B):
        """Workspace of the energy forward of B chains."""
        su = self.su
        with torch.cuda.device(self.dev):
            eng = self.model._engine_ready(self.dev)
            n_sel = B * su.S if su.w_lm != 0.0 else 0
            if su.disto is not None:  # the q / k / lse of every layer, and the pair logits themselves
                eng.set_pair_head(su.disto.head)
                return eng.rows_pair_bytes(B, su.T, n_sel) + B * su.S * su.S * su.disto.head.n_out * 4
            if su.w_contact != 0.0:
                return eng.rows_contacts_bytes(B, su.T, n_sel)
            return eng._query(eng.N.lib.esmk_rows_workspace_bytes, B, su.T, n_sel, offset=True)[0]

    def tables(self, B):
        """(flat residue rows int32 [B * S], their int64 form, offsets int32 [B + 1], n_res int32 [B]) of a batch of B chains."""
        if B not in self._tables:
            su = self.su
            rows = (torch.arange(B).view(B, 1) * su.T + torch.arange(su.bos, su.bos + su.S).view(1, -1)).reshape(-1)
            sel = rows.to(torch.int32).to(self.dev)
            off = (torch.arange(B + 1) * su.S).to(torch.int32).to(self.dev)
            n_res = torch.full((B,), su.S, dtype=torch.int32).to(self.dev)
            self._tables[B] = (sel, sel.long(), off, n_res)
        return self._tables[B]

    def terms(self, tok):
        """``(e_contact fp64 [B] or None, lp_sum fp64 [B] or None, n_res int32 [B], e_ngram fp64 [B] or None)`` of ``tok`` int64
        [B, T] on the device."""
        from . import ops

        su = self.su
        B = tok.shape[0]
        sel, sel_long, off, n_res = self.tables(B)
        want_lm = su.w_lm != 0.0
        if su.disto is not None:
            dt = su.disto
            with torch.cuda.device(self.dev):
                eng = self.model._engine_ready(self.dev)
                eng.set_pair_head(dt.head)
                pair = torch.empty((B, su.S, su.S, dt.head.n_out), dtype=torch.float32, device=self.dev)
                lp = eng.forward_rows_pair(tok, sel if want_lm else None, self.V, pair)
            e_contact = ops.distogram_energy(pair, self.bins, dt.first, dt.n_bins, su.min_sep, 1.0 / dt.temperature)[0]
        elif su.w_contact != 0.0:
            with torch.cuda.device(self.dev):
                lp, maps = self.model._engine_ready(self.dev).forward_rows_contacts(tok, sel if want_lm else None, self.V, su.S)
            e_contact = ops.contact_energy(maps, self.target, su.min_sep, su.contact_loss)[0]
        else:
            lp, e_contact = forward_rows(self.model, tok, sel), None
        lp_sum = ops.sum_target_rows(lp, tok.view(-1)[sel_long].to(torch.int32), off) if want_lm else None
        e_ngram = None
        if self.ngram_q is not None:
            e_ngram = ops.ngram_energy(tok, su.bos, su.S, self.ngram_code, len(su.ngram.alphabet), self.ngram_q)
        return e_contact, lp_sum, n_res, e_ngram

    def combine(self, e_contact, lp_sum, n_res, e_ngram=None):
        """``(E, E_contact, E_lm)`` fp64 [B], with the n-gram term ``(E, E_contact, E_lm, E_ngram)``: the arithmetic of
        esmk_op_mh_accept / esmk_op_mh_accept_ex, one rounding per operation (a true division by a device tensor, a product per
        weight, one sum per further term)."""
        B = n_res.numel()
        zero = torch.zeros((B,), dtype=torch.float64, device=self.dev)
        e_c = zero if e_contact is None else e_contact
        e_lm = zero if lp_sum is None else -(lp_sum / n_res.to(torch.float64))
        e = (self.su.w_contact * e_c) + (self.su.w_lm * e_lm)
        if e_ngram is None:
            return e, e_c, e_lm
        return e + (self.su.w_ngram * e_ngram), e_c, e_lm, e_ngram


@torch.no_grad()
def design_energy(model, tokens, target, w_contact=1.0, w_lm=1.0, contact_loss="pos", min_sep=6, max_bytes=8 << 30, w_ngram=0.0,
                  ngram=None):
    """The energy ``design`` minimises, for given sequences ``tokens`` int64 ``[B, T]`` (no padding, all of the target's length),
    through the same entry and kernels: a dict of fp64 ``[B]`` device tensors ``energy`` = w_contact * ``e_contact`` + w_lm *
    ``e_lm``, with ``w_ngram != 0`` (and ``ngram``, an ``esm_amd.ngram.Background``) plus w_ngram * ``e_ngram``, which the dict
    then holds too.  A sequence gets the same bits alone and in any batch."""
    su = _Setup(model, tokens, target, w_contact, w_lm, contact_loss, min_sep, w_ngram, ngram)
    tok = _device_tokens(model, su.tok_cpu)
    en = _Energy(model, su, tok.device)
    step = batch_size(en.bytes_of, su.B, max_bytes)
    parts = [en.combine(*en.terms(tok[lo: lo + step].contiguous())) for lo in range(0, su.B, step)]
    names = ("energy", "e_contact", "e_lm") + (NGRAM_FIELDS if su.ngram is not None else ())
    return {name: torch.cat([p[i] for p in parts]) for i, name in enumerate(names)}


def _chain_ids(chain_ids, B):
    if chain_ids is None:
        return torch.arange(B, dtype=torch.int32)
    ids = torch.as_tensor(chain_ids).to(torch.int64).view(-1).cpu()
    if ids.numel() != B:
        raise ValueError(f"{ids.numel()} chain ids for {B} chains")
    if bool(((ids < 0) | (ids >= 2 ** 31)).any()):
        raise ValueError("chain ids must lie in [0, 2^31)")
    return ids.to(torch.int32)


@torch.no_grad()
def design(model, tokens, target, steps, positions=None, w_contact=1.0, w_lm=1.0, contact_loss="pos", min_sep=6, temperature=1.0,
           proposal="uniform", proposal_temperature=1.0, allowed=None, force_new=None, seed=0, chain_ids=None,
           return_trajectory=False, max_bytes=8 << 30, w_ngram=0.0, ngram=None, replicas=None, swap_every=1):
    """Metropolis-Hastings chains from ``tokens`` int64 ``[B, T]`` (every row a chain; no padding, all of the target's length)
    toward ``target``: ``(tokens [B, T], energy fp64 [B])`` on the model's device — with ``replicas`` ``(tokens, energy, rung int32
    [B])`` —, plus the trajectory when asked for.

    target       a ``DistogramTarget`` (lm-design's distance-bin term through a ``PairHead``; ``contact_loss`` is then ignored and
                 ``min_sep`` may be 0), or ``[S, S]`` bool, uint8 (0 / 1 / 2 = ignore) or float (thresholded at 0.5, NaN = ignore), S = T minus the
                 <cls> / <eos> the alphabet adds (``contacts_from_pdb`` reads one from a PDB file); None with ``w_contact=0``.
    steps        every step proposes one single-site mutation per chain and accepts it with probability min(1, exp(-dE / T) *
                 q(x | x') / q(x' | x)).
    positions    the designable token positions, as for ``gibbs_sample``; a chain without one proposes nothing.
    w_contact, w_lm, contact_loss ("pos" / "bce"), min_sep: the energy (module docstring).
    temperature  a float, or a length-``steps`` sequence: any annealing schedule is the caller's list.  0: greedy (accept iff
                 the energy does not rise).
    proposal     "uniform" (lm-design's): a uniform site, a uniform token of ``allowed`` — with ``force_new`` (default here)
                 never the current one.  "lm": a uniform site, the token drawn from the model's conditional at the masked site,
                 softmax(log_softmax(logits) / proposal_temperature) over ``allowed``, with the Hastings correction;
                 ``force_new`` is refused with it (the reverse move would have another candidate set), and so is a start token
                 outside ``allowed`` at a designable position (it could never be proposed back).
    seed, chain_ids  the Philox key and counter word 0 of every chain: a chain runs the same trajectory in any batch.
    return_trajectory  also a dict of ``[steps, B]`` device tensors: ``site``, ``old``, ``new`` int32 (-1: nothing proposed),
                 ``e_cur`` (before the step), ``e_prop``, ``e_contact``, ``e_lm`` (the proposal's energy and its terms),
                 ``hastings``, ``u`` fp64 and ``accepted`` uint8.
    max_bytes    chains run in batches whose energy forward, with the contact accumulators of the pinned head-group count, fits
                 this much workspace.  With ``replicas`` a batch holds whole ladders.
    w_ngram, ngram  the weight of the n-gram term and its background (``esm_amd.ngram.Background``); the trajectory then also
                 holds ``e_ngram`` (of the proposal).
    replicas     K >= 2: every K consecutive chains are a ladder (B a multiple of K), chain b starting at rung b % K.
                 ``temperature`` is then a length-K ladder, rung 0 first, or ``steps`` such ladders (``[steps, K]``), all positive
                 and finite.  The trajectory also holds ``rung`` int32 (the rung a step ran at), ``swapped`` uint8 and ``swap_u``
                 fp64 (-1: no swap attempted for that chain after that step).  A ladder runs the same trajectory alone and in any
                 batch.
    swap_every   after step s with (s + 1) % swap_every == 0, swap round (s + 1) // swap_every - 1 runs with the temperatures of
                 step s; 0: never."""
    from . import ops

    su = _Setup(model, tokens, target, w_contact, w_lm, contact_loss, min_sep, w_ngram, ngram)
    K = None
    if replicas is not None:
        K = int(replicas)
        if K < 2 or K > 64:
            raise ValueError("replicas: a ladder has 2 .. 64 rungs")
        if su.B % K != 0:
            raise ValueError(f"{su.B} chains are no multiple of replicas = {K}: every ladder holds one chain per rung")
    swap_every = int(swap_every)
    if swap_every < 0:
        raise ValueError("swap_every must not be negative (0: no swaps)")
    steps = int(steps)
    if steps < 0 or steps >= 2 ** 31:
        raise ValueError("steps must lie in [0, 2^31)")
    if proposal not in PROPOSALS:
        raise ValueError(f"proposal {proposal!r}: one of {PROPOSALS}")
    lm = proposal == "lm"
    if force_new is None:
        force_new = not lm
    if lm and force_new:
        raise ValueError("force_new with proposal='lm': the reverse proposal would have another candidate set")
    inv_t_prop = 1.0
    if lm:
        proposal_temperature = float(proposal_temperature)
        if not proposal_temperature > 0.0 or proposal_temperature == float("inf"):
            raise ValueError("proposal_temperature must be positive and finite")
        inv_t_prop = 1.0 / proposal_temperature
    inv_t = ladder_inverse_temperatures(temperature, steps, K) if K else inverse_temperatures(temperature, steps)
    mask = allowed_mask(model, allowed)
    lists = _position_lists(model, su.tok_cpu, positions)
    if lm:
        for b, ps in enumerate(lists):
            for p in ps:
                if not (mask >> int(su.tok_cpu[b, p])) & 1:
                    raise ValueError(f"proposal='lm': chain {b} starts with a token outside `allowed` at designable position {p}")
    ids_cpu = _chain_ids(chain_ids, su.B)
    seed = ops._seed64(seed)

    state = _device_tokens(model, su.tok_cpu).clone()
    dev = state.device
    en = _Energy(model, su, dev)
    ex = None  # the plain loop: esmk_op_mh_accept with the step's scalar temperature
    if K or su.ngram is not None:
        table = inv_t if K else np.asarray(inv_t, dtype=np.float64).reshape(steps, 1)
        ex = dict(K=K, swap_every=swap_every, inv_t_host=table,
                  inv_t=torch.from_numpy(table).to(dev) if steps else torch.zeros((0, K or 1), dtype=torch.float64, device=dev))
    if K:
        if en.bytes_of(K) > int(max_bytes):
            raise ValueError(f"max_bytes = {int(max_bytes)}: the energy forward of one ladder of {K} chains takes {en.bytes_of(K)} "
                             "bytes of workspace, and a batch holds whole ladders")
        per = K * batch_size(lambda n: en.bytes_of(n * K), su.B // K, max_bytes)
    else:
        per = batch_size(en.bytes_of, su.B, max_bytes)
    fields = TRAJECTORY_FIELDS + (NGRAM_FIELDS if su.ngram is not None else ()) + (REPLICA_FIELDS if K else ())
    energies, trajs, rungs = [], [], []
    for lo in range(0, su.B, per):
        hi = min(lo + per, su.B)
        starts = [0]
        for ps in lists[lo:hi]:
            starts.append(starts[-1] + len(ps))
        pos_off = torch.tensor(starts, dtype=torch.int32).to(dev)
        pos = torch.tensor([p for ps in lists[lo:hi] for p in ps], dtype=torch.int32).to(dev)
        part = state[lo:hi]  # a view: rows of a contiguous matrix are contiguous
        e, traj, rung = _run(model, en, part, pos_off, pos, ids_cpu[lo:hi].to(dev), steps, inv_t, lm, inv_t_prop, mask, bool(force_new),
                             seed, return_trajectory, fields, ex)
        energies.append(e)
        trajs.append(traj)
        rungs.append(rung)
    out = (state, torch.cat(energies)) + ((torch.cat(rungs),) if K else ())
    if not return_trajectory:
        return out
    return out + ({name: torch.cat([t[name] for t in trajs], dim=1) for name in fields},)


_FIELD_DTYPES = dict(site=torch.int32, old=torch.int32, new=torch.int32, accepted=torch.uint8, rung=torch.int32, swapped=torch.uint8)


def _run(model, en, state, pos_off, pos, ids, steps, inv_t, lm, inv_t_prop, mask, force_new, seed, return_trajectory, fields, ex):
    """The step loop on one batch: ``state`` int64 [n, T] (a view of the caller's matrix) is updated in place; nothing inside
    the loop waits for the device.  ``ex`` None: the plain loop.  Else the per-step tables of inverse temperatures (``inv_t`` on the
    device, ``inv_t_host`` [steps, n_rung]) of esmk_op_mh_accept_ex and, with ``K``, the ladders and their swaps."""
    from . import ops

    su = en.su
    n, T = state.shape
    dev = state.device
    e_cur, e_contact_cur, e_lm_cur, *rest = (t.clone() for t in en.combine(*en.terms(state)))
    e_ngram_cur = rest[0] if rest else None
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    row0 = rows * T
    one_each = torch.arange(n + 1, dtype=torch.int32, device=dev)
    zero = torch.zeros((n,), dtype=torch.float64, device=dev)
    K = ex["K"] if ex is not None else None
    rung = None
    if K:
        rung = (rows % K).contiguous()
        ladder_ids = ids.view(-1, K)[:, 0].contiguous()
        no_swap = torch.zeros((n,), dtype=torch.uint8, device=dev)
        no_u = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    traj = {name: [] for name in fields}
    for s in range(steps):
        site, old, new = ops.propose_mutations(state, pos_off, pos, ids, mask, force_new=force_new, seed=seed, step=s)
        hastings = None
        if lm:  # the token comes from the model's conditional at the masked site; the uniform token above is not used
            masked = ops.mask_rows_multi(state, one_each, site, rows, model.mask_idx)
            lp_site = forward_rows(model, masked, row0 + site.clamp(min=0))
            drawn = ops.sample_rows(lp_site, ids, site, mask, inv_t_prop, seed=seed, step=s, want_u=False)[0]
            new = torch.where(site >= 0, drawn, torch.full_like(drawn, -1))
            hastings = ops.hastings_rows(lp_site, old, new, inv_t_prop)
        proposed = ops.substitute_rows(state, site, new, src_rows=rows, vocab=en.V)
        e_contact, lp_sum, n_res, e_ngram = en.terms(proposed)
        before = e_cur.clone() if return_trajectory else None
        if ex is None:
            accepted, u, e_prop = ops.mh_accept(state, site, new, ids, e_cur, e_contact=e_contact, lp_sum=lp_sum, n_res=n_res,
                                                hastings=hastings, w_contact=su.w_contact, w_lm=su.w_lm, inv_temperature=inv_t[s],
                                                seed=seed, step=s, e_contact_cur=e_contact_cur, e_lm_cur=e_lm_cur)
        else:
            ran_at = rung.clone() if K and return_trajectory else None
            accepted, u, e_prop = ops.mh_accept_ex(state, site, new, ids, e_cur, ex["inv_t"][s], rung=rung, e_contact=e_contact,
                                                   lp_sum=lp_sum, n_res=n_res, hastings=hastings, e_extra=e_ngram,
                                                   w_contact=su.w_contact, w_lm=su.w_lm, w_extra=su.w_ngram, seed=seed, step=s,
                                                   e_contact_cur=e_contact_cur, e_lm_cur=e_lm_cur, e_extra_cur=e_ngram_cur)
            swapped, swap_u = (no_swap, no_u) if K else (None, None)
            if K and ex["swap_every"] > 0 and (s + 1) % ex["swap_every"] == 0:
                swapped, swap_u = ops.replica_swap(rung, e_cur, ex["inv_t"][s], ex["inv_t_host"][s], ladder_ids, seed=seed,
                                                   round=(s + 1) // ex["swap_every"] - 1)
        if return_trajectory:
            _, e_c, e_lm = en.combine(e_contact, lp_sum, n_res)
            values = dict(zip(TRAJECTORY_FIELDS, (site, old, new, before, e_prop, e_c, e_lm, zero if hastings is None else hastings,
                                                  u, accepted)))
            if e_ngram is not None:
                values["e_ngram"] = e_ngram
            if K:
                values.update(rung=ran_at, swapped=swapped, swap_u=swap_u)
            for name in fields:
                traj[name].append(values[name])
    if not return_trajectory:
        return e_cur, None, rung
    out = {}
    for name, parts in traj.items():
        out[name] = torch.stack(parts) if parts else torch.empty((0, n), dtype=_FIELD_DTYPES.get(name, torch.float64), device=dev)
    return e_cur, out, rung


# ---- python -m esm_amd.design ---------------------------------------------------------------------------------------------------
def anneal_ladder(t0, t1, steps):
    """A geometric ladder of ``steps`` temperatures from ``t0`` to ``t1`` (both positive), built on the host."""
    t0, t1 = float(t0), float(t1)
    if not (t0 > 0.0 and t1 > 0.0 and math.isfinite(t0) and math.isfinite(t1)):
        raise ValueError("--anneal t0:t1 takes two positive temperatures")
    if steps <= 1:
        return [t0] * steps
    return [t0 * (t1 / t0) ** (s / (steps - 1)) for s in range(steps)]


def _anneal(text):
    try:
        t0, t1 = text.split(":")
        anneal_ladder(t0, t1, 2)
        return float(t0), float(t1)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r}: t0:t1, two positive temperatures")


def _at_least(lo, kind=int):
    def parse(text):
        v = kind(text)
        if not v >= lo:
            raise argparse.ArgumentTypeError(f"{text!r} is below {lo}")
        return v

    return parse


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m esm_amd.design", description="Design sequences toward a target contact map: "
                                "Metropolis-Hastings chains on the MI355X engine.")
    p.add_argument("--model-location", required=True, help="checkpoint file or model name (ESM-2, ESM-1b / ESM-1v, ESM-1)")
    t = p.add_mutually_exclusive_group(required=True)
    t.add_argument("--target-pdb", help="PDB file: contacts of its C-beta atoms (C-alpha for glycine)")
    t.add_argument("--target-npy", help="[S, S] array: bool, 0 / 1 / 2 = ignore, or floats thresholded at 0.5 (NaN = ignore)")
    t.add_argument("--target-from-sequence", metavar="SEQ", help="the model's own contact map of a native sequence, at 0.5")
    t.add_argument("--no-target", action="store_true", help="LM term only (needs --length)")
    p.add_argument("--structure", choices=("contacts", "distogram"), default="contacts",
                   help="the structure term: the contact head's map against the target contacts, or (with --pair-head and "
                        "--target-pdb) lm-design's distance-bin cross-entropy on a linear projection of the attention maps")
    p.add_argument("--pair-head", metavar="CKPT", default=None, help="lm-design's linear projection checkpoint (--structure distogram)")
    p.add_argument("--chain", default=None, help="chain of --target-pdb (default: its first chain)")
    p.add_argument("--cutoff", type=_at_least(0.0, float), default=8.0, help="contact distance of --target-pdb in angstrom")
    p.add_argument("--length", type=_at_least(1), default=None, help="residues per chain with --no-target")
    i = p.add_mutually_exclusive_group()
    i.add_argument("--init-sequence", default=None, help="start every chain from this sequence")
    i.add_argument("--init", choices=("random",), default="random", help="start from uniform random residues (default)")
    p.add_argument("--num-chains", type=_at_least(1), default=1)
    p.add_argument("--steps", type=_at_least(0), default=1000)
    s = p.add_mutually_exclusive_group()
    s.add_argument("--temperature", type=_at_least(0.0, float), default=None, help="constant temperature (default 1; 0: greedy)")
    s.add_argument("--anneal", type=_anneal, default=None, metavar="T0:T1", help="geometric ladder from T0 to T1")
    s.add_argument("--ladder", type=_anneal, default=None, metavar="T0:T1",
                   help="with --replicas K: K geometric temperatures, rung 0 = T0, held for the whole run")
    p.add_argument("--replicas", type=_at_least(2), default=None, metavar="K",
                   help="replica exchange: every K consecutive chains are a ladder (needs --ladder)")
    p.add_argument("--swap-every", type=_at_least(0), default=1, metavar="N", help="steps between swap rounds (0: never)")
    p.add_argument("--w-ngram", type=float, default=0.0, help="weight of the n-gram term (needs --ngram-table)")
    p.add_argument("--ngram-table", default=None, help=".npz background of `python -m esm_amd.ngram_table`")
    p.add_argument("--proposal", choices=PROPOSALS, default="uniform")
    p.add_argument("--proposal-temperature", type=float, default=1.0)
    p.add_argument("--w-contact", type=float, default=1.0)
    p.add_argument("--w-lm", type=float, default=1.0)
    p.add_argument("--contact-loss", choices=CONTACT_LOSSES, default="pos")
    p.add_argument("--min-sep", type=_at_least(1), default=6)
    p.add_argument("--seed", type=_at_least(0), default=0)
    p.add_argument("--output", required=True, help="FASTA file of the final sequences")
    p.add_argument("--log", default=None, help="CSV file of every step of every chain")
    a = p.parse_args(argv)
    if a.no_target and a.length is None:
        p.error("--no-target needs --length")
    if not a.no_target and a.length is not None:
        p.error("--length goes with --no-target: the target sets the length")
    if a.chain is not None and a.target_pdb is None:
        p.error("--chain goes with --target-pdb")
    if a.structure == "distogram" and (a.pair_head is None or a.target_pdb is None):
        p.error("--structure distogram needs --pair-head and --target-pdb")
    if a.structure == "contacts" and a.pair_head is not None:
        p.error("--pair-head goes with --structure distogram")
    if (a.replicas is None) != (a.ladder is None):
        p.error("--replicas K and --ladder T0:T1 go together")
    if a.replicas is not None and a.num_chains % a.replicas != 0:
        p.error(f"--num-chains {a.num_chains} is no multiple of --replicas {a.replicas}")
    if a.w_ngram != 0.0 and a.ngram_table is None:
        p.error("--w-ngram needs --ngram-table")
    return a


def random_sequences(n, length, seed, residues="ACDEFGHIKLMNPQRSTVWY"):
    """``n`` uniform random sequences over ``residues`` from a host generator keyed by ``seed``."""
    rng = np.random.default_rng(int(seed))
    return ["".join(residues[i] for i in rng.integers(0, len(residues), size=length)) for _ in range(n)]


def write_fasta(path, label, chain_ids, sequences, energies, seed, rungs=None):
    with open(path, "w") as fh:
        for i, (cid, seq, e) in enumerate(zip(chain_ids, sequences, energies)):
            rung = "" if rungs is None else f"|rung={rungs[i]}"
            fh.write(f">{label}|chain={cid}|seed={seed}|energy={e:.6f}{rung}\n{seq}\n")


def write_log(path, traj, chain_ids):
    host = {k: v.cpu().numpy() for k, v in traj.items()}
    fields = [k for k in TRAJECTORY_FIELDS + NGRAM_FIELDS + REPLICA_FIELDS if k in host]
    with open(path, "w") as fh:
        fh.write("step,chain," + ",".join(fields) + "\n")
        steps, n = host["site"].shape
        for s in range(steps):
            for c in range(n):
                fh.write(f"{s},{chain_ids[c]}," + ",".join(repr(host[k][s, c].item()) for k in fields) + "\n")


def decode(alphabet, row, bos, eos):
    return "".join(alphabet.get_tok(int(t)) for t in row[bos: len(row) - eos])


def main(argv=None):
    a = parse_args(argv)
    from . import pretrained
    from .msa_transformer import MSATransformer

    model, alphabet = pretrained.load_model_and_alphabet(a.model_location)
    if isinstance(model, MSATransformer):
        raise SystemExit("esm_amd.design: the MSA Transformer is not a design model here (single-sequence models: ESM-2, "
                         "ESM-1b / ESM-1v, ESM-1)")
    model = model.eval().cuda()
    convert = alphabet.get_batch_converter()
    target, label = None, "design"
    if a.target_pdb:
        target = contacts_from_pdb(a.target_pdb, a.chain, a.cutoff)[1]
    elif a.target_npy:
        target = np.load(a.target_npy)
    elif a.target_from_sequence:
        toks = convert([("native", a.target_from_sequence)])[2].cuda()
        target = model.predict_contacts(toks)[0].float().cpu().numpy()
    if a.structure == "distogram":
        from .pair_head import PairHead, distogram_from_pdb

        target = DistogramTarget(distogram_from_pdb(a.target_pdb, a.chain)[1], PairHead.from_linear_projection(a.pair_head, model))
    length = a.length if a.no_target else target.S if a.structure == "distogram" else int(np.asarray(target).shape[0])
    if a.init_sequence is not None:
        if len(a.init_sequence) != length:
            raise SystemExit(f"--init-sequence has {len(a.init_sequence)} residues, the target {length}")
        starts = [a.init_sequence] * a.num_chains
    else:
        starts = random_sequences(a.num_chains, length, a.seed)
    tokens = convert([(str(c), s) for c, s in enumerate(starts)])[2]
    temperature = anneal_ladder(*a.anneal, a.steps) if a.anneal else (1.0 if a.temperature is None else a.temperature)
    extra = {}
    if a.replicas is not None:
        temperature = anneal_ladder(*a.ladder, a.replicas)
        extra.update(replicas=a.replicas, swap_every=a.swap_every)
    if a.w_ngram != 0.0:
        from .ngram import Background

        extra.update(w_ngram=a.w_ngram, ngram=Background.load(a.ngram_table))
    out = design(model, tokens, target, a.steps, w_contact=0.0 if a.no_target else a.w_contact, w_lm=a.w_lm,
                 contact_loss=a.contact_loss, min_sep=a.min_sep, temperature=temperature, proposal=a.proposal,
                 proposal_temperature=a.proposal_temperature, seed=a.seed, return_trajectory=a.log is not None, **extra)
    final, energy = out[0].cpu(), out[1].cpu().tolist()
    rungs = out[2].cpu().tolist() if a.replicas is not None else None
    bos, eos = int(bool(model.prepend_bos)), int(bool(model.append_eos))
    ids = list(range(a.num_chains))
    write_fasta(a.output, label, ids, [decode(alphabet, row.tolist(), bos, eos) for row in final], energy, a.seed, rungs)
    if a.log is not None:
        write_log(a.log, out[-1], ids)
    print(f"{a.num_chains} chains, {a.steps} steps: energy {min(energy):.4f} .. {max(energy):.4f} -> {a.output}", file=sys.stderr)


class _CallableModule(type(sys)):
    """``esm_amd.design`` is this module; calling it calls ``design`` (the public interface names both ``esm_amd.design(...)``
    and ``python -m esm_amd.design``)."""

    def __call__(self, *args, **kwargs):
        return design(*args, **kwargs)


if __name__ == "__main__":
    main()
else:
    sys.modules[__name__].__class__ = _CallableModule
