"""Linear pairwise heads on the attention maps, without the attention tensor (csrc/pair_head.hip).

lm-design's structure model (examples/lm-design/utils/linear_projection.py:85-135, ``LinearProjectionDistogramModel``) is two
1 x 1 convolutions over the L*H attention channels of the language model: ``conv1`` on the symmetrised maps P + P^T gives 18
distance and 18 omega bins, ``conv2`` on the maps as they are gives 18 theta and 8 phi bins; the maps are cropped to the
residues (linear_projection.py:76-82), nothing else.  ``model(tokens, need_head_weights=True)`` builds ``[B, L, H, T, T]`` for
it (2.77 GB of fp32 per 1024-token sequence at 650M dims); ``model.pair_logits(tokens, head)`` keeps every layer's q, k and row
log-sum-exp instead and runs the head as one launch over all channels after the last layer (``esmk_forward_rows_pair``).

    head = PairHead.from_linear_projection("linear_projection_model.pt", model)
    out = model.pair_logits(tokens, head)          # {"dist": [B,S,S,18], "omega": ..., "theta": ..., "phi": [B,S,S,8]}
    bins = distogram_bins(distances)               # uint8 [S,S], 255 where the distance is NaN
    e, n = ops.distogram_energy(out["dist"], bins) # lm-design's dist_cce term per sequence

Any linear head on the attention maps fits: ``PairHead(w_sym, b_sym, w_asym, b_asym)`` with at most 64 outputs in all.

Not built: token-packed batches (``varlen=True``) and windows, the MSA Transformer (``NotImplementedError``), the angle terms of
lm-design's loss, a split-precision 16-bit MFMA form of the kernel (DESIGN.md I.4c.6 prices it).

    python -m esm_amd.pair_logits --model-location esm2_t33_650M_UR50D.pt --pair-head linear_projection_model.pt \\
        --sequence MKTAYIAKQR --output-dir out/
"""
import argparse
import os

import numpy as np
import torch

IGNORE_BIN = 255  # target bin of a pair that does not count
MAX_OUTPUTS = 64  # esmk_set_pair_head: n_sym + n_asym
# linear_projection.py:94-98 with lm_design's bin counts (N_BINS 18, THETA 18, PHI 8, OMEGA 18): how forward() slices the outputs
LM_DESIGN_OUTPUTS = {"dist": ("sym", 0, 18), "omega": ("sym", 18, 36), "theta": ("asym", 0, 18), "phi": ("asym", 18, 26)}


def _block(w, b, what):
    if w is None:
        if b is not None:
            raise ValueError(f"PairHead: b_{what} without w_{what}")
        return torch.zeros((0, 0), dtype=torch.float32), torch.zeros((0,), dtype=torch.float32)
    w = torch.as_tensor(w).detach().to(device="cpu", dtype=torch.float32)
    if w.ndim == 4 and w.shape[2:] == (1, 1):  # a Conv2d(C, n, 1) weight
        w = w[:, :, 0, 0]
    if w.ndim != 2:
        raise ValueError(f"PairHead: w_{what} is [n, L*H] (or a 1 x 1 Conv2d weight [n, L*H, 1, 1]), got shape {tuple(w.shape)}")
    b = torch.zeros(w.shape[0]) if b is None else torch.as_tensor(b).detach().to(device="cpu", dtype=torch.float32)
    if tuple(b.shape) != (w.shape[0],):
        raise ValueError(f"PairHead: b_{what} has shape {tuple(b.shape)}, w_{what} has {w.shape[0]} outputs")
    return w.contiguous(), b.contiguous()


class PairHead:
    """A linear head on the L*H attention channels c = layer * H + head: ``w_sym`` fp32 ``[n_sym, L*H]`` (bias ``b_sym``) acts
    on P + P^T, ``w_asym`` ``[n_asym, L*H]`` (``b_asym``) on P; either block may be None.  ``outputs`` maps a name to
    ``(block, lo, hi)`` with block ``"sym"`` or ``"asym"``: the slice of that block ``pair_logits`` returns under the name
    (default: the whole blocks as ``"sym"`` and ``"asym"``).  n_sym + n_asym <= 64."""

    def __init__(self, w_sym, b_sym, w_asym, b_asym, outputs=None):
        self.w_sym, self.b_sym = _block(w_sym, b_sym, "sym")
        self.w_asym, self.b_asym = _block(w_asym, b_asym, "asym")
        self.n_sym, self.n_asym = self.w_sym.shape[0], self.w_asym.shape[0]
        if self.n_sym + self.n_asym == 0:
            raise ValueError("PairHead: no output (both blocks are empty)")
        if self.n_sym + self.n_asym > MAX_OUTPUTS:
            raise ValueError(f"PairHead: {self.n_sym} + {self.n_asym} outputs, the kernel takes at most {MAX_OUTPUTS}")
        if self.n_sym and self.n_asym and self.w_sym.shape[1] != self.w_asym.shape[1]:
            raise ValueError(f"PairHead: w_sym has {self.w_sym.shape[1]} channels, w_asym {self.w_asym.shape[1]}")
        self.channels = (self.w_sym if self.n_sym else self.w_asym).shape[1]
        if outputs is None:
            outputs = {name: (name, 0, n) for name, n in (("sym", self.n_sym), ("asym", self.n_asym)) if n}
        self.outputs = {}
        for name, (block, lo, hi) in outputs.items():
            if block not in ("sym", "asym"):
                raise ValueError(f"PairHead: output {name!r}: block must be 'sym' or 'asym', got {block!r}")
            n = self.n_sym if block == "sym" else self.n_asym
            if not 0 <= lo < hi <= n:
                raise ValueError(f"PairHead: output {name!r}: [{lo}, {hi}) is not a slice of the {n} {block} outputs")
            self.outputs[name] = (block, int(lo), int(hi))

    @property
    def n_out(self):
        return self.n_sym + self.n_asym

    def matrix(self):
        """fp32 ``[L*H, n_sym + n_asym]`` on the CPU: row c = the weights of channel c, symmetric outputs first."""
        return torch.cat([w for w in (self.w_sym, self.w_asym) if w.shape[0]], 0).t().contiguous()

    def bias(self):
        return torch.cat([self.b_sym, self.b_asym]).contiguous()

    def columns(self, name):
        """``(lo, hi)``: the columns of the output tensor that hold output ``name``."""
        block, lo, hi = self.outputs[name]
        off = 0 if block == "sym" else self.n_sym
        return off + lo, off + hi

    def check_model(self, model):
        C = int(model.num_layers) * int(model.attention_heads)
        if self.channels != C:
            raise ValueError(f"PairHead: the head has {self.channels} input channels, the model has num_layers * attention_heads = "
                             f"{model.num_layers} * {model.attention_heads} = {C} attention maps")

    @classmethod
    def from_linear_projection(cls, path_or_state_dict, model=None):
        """lm-design's projection checkpoint: ``state["model"]`` (or the state dict itself) with ``conv1.weight [36, C, 1, 1]``,
        ``conv1.bias``, ``conv2.weight [26, C, 1, 1]``, ``conv2.bias``; outputs ``dist``, ``omega``, ``theta``, ``phi`` as
        linear_projection.py:130-135 slices them.  A path is read with ``torch.load(..., weights_only=True)``.  ValueError when
        C is not L*H of ``model``."""
        state = path_or_state_dict
        if isinstance(state, (str, os.PathLike)):
            state = torch.load(state, map_location="cpu", weights_only=True)
        if "model" in state and "conv1.weight" not in state:
            state = state["model"]
        for key in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"):
            if key not in state:
                raise ValueError(f"PairHead.from_linear_projection: the checkpoint has no {key!r}")
        w1, w2 = state["conv1.weight"], state["conv2.weight"]
        if tuple(w1.shape[2:]) != (1, 1) or tuple(w2.shape[2:]) != (1, 1) or w1.shape[0] != 36 or w2.shape[0] != 26:
            raise ValueError("PairHead.from_linear_projection: expected conv1.weight [36, C, 1, 1] and conv2.weight [26, C, 1, 1], "
                             f"got {tuple(w1.shape)} and {tuple(w2.shape)}")
        head = cls(w1, state["conv1.bias"], w2, state["conv2.bias"], outputs=LM_DESIGN_OUTPUTS)
        if model is not None:
            head.check_model(model)
        return head


def distogram_bins(dist, d_min=2.5, d_max=20.0, n_bins=18):
    """uint8 ``[S, S]`` distance bins of lm-design's targets (examples/lm-design/utils/pdb_loader.py:243-256 with DMIN 2.5):
    ``np.digitize(dist, np.linspace(d_min, d_max, n_bins - 1))`` — bin 0 below ``d_min``, bin ``n_bins - 1`` from ``d_max`` on
    ("no contact") — and 255 (ignored by ``distogram_energy``) where the distance is NaN."""
    d = np.asarray(dist.cpu() if torch.is_tensor(dist) else dist, dtype=np.float64)
    if not 2 <= int(n_bins) <= IGNORE_BIN:
        raise ValueError(f"distogram_bins: n_bins must be 2 .. {IGNORE_BIN}")
    bins = np.digitize(d, np.linspace(float(d_min), float(d_max), int(n_bins) - 1)).astype(np.uint8)
    bins[np.isnan(d)] = IGNORE_BIN
    return bins


def distogram_from_pdb(path, chain=None, d_min=2.5, d_max=20.0, n_bins=18):
    """``(sequence, bins)`` of one chain of a PDB file, read as ``contacts_from_pdb`` reads it: ``bins`` = ``distogram_bins`` of
    the distances between the file's C-beta atoms (C-alpha for glycine), 255 in the row and column of a residue that lacks the
    atom.  This MEASURES the file's C-beta; the reference places a virtual C-beta from the backbone N, CA, C
    (pdb_loader.py:235-239, get_coords6d), so bins next to an edge can differ between the two."""
    from .design import _read_cb

    seq, have, xyz = _read_cb(path, chain)
    dist = np.sqrt(((xyz[:, None, :] - xyz[None, :, :]) ** 2).sum(-1))
    dist[~have, :] = np.nan
    dist[:, ~have] = np.nan
    return seq, distogram_bins(dist, d_min, d_max, n_bins)


def _refuse(model, varlen, window):
    from .msa_transformer import MSATransformer

    if isinstance(model, MSATransformer):
        raise NotImplementedError("pair_logits: the MSA Transformer has no pairwise head on the MI355X engine (the head is built on "
                                  "the attention maps of ESM-2, ESM-1b / ESM-1v and ESM-1 models)")
    if varlen:
        raise NotImplementedError("pair_logits(varlen=True): the pairwise head runs on padded batches only; token-packed batches are "
                                  "not built")
    if window is not None:
        raise NotImplementedError("pair_logits(window=...): the pairwise head is not built for windows of long sequences")


def pair_logits(model, tokens, head, max_bytes=8 << 30, varlen=False, window=None):
    """``{name: fp32 [B, S, S, n]}`` for the outputs of ``head`` (``PairHead``): device views of ONE ``[B, S, S, n_sym + n_asym]``
    tensor (also returned under ``"all"`` when no output has that name), S = T minus the <cls> / <eos> the alphabet adds.
    ``out[b, i, j]`` = the head on the attention probabilities of residues i, j of sequence b in every (layer, head), as the
    reference computes from ``model(tokens, need_head_weights=True)["attentions"]``; entries that involve a <pad> position hold
    the bias.  Sequences run in batches whose workspace (the forward's, plus the q / k / lse of every layer) and slice of the
    output fit ``max_bytes``; a sequence's map does not depend on the batch it ran in."""
    from .scoring import _device_tokens

    _refuse(model, varlen, window)
    if not isinstance(head, PairHead):
        raise TypeError("pair_logits: head must be an esm_amd.pair_head.PairHead")
    head.check_model(model)
    tok = _device_tokens(model, tokens)
    dev = tok.device
    B, T = tok.shape
    S = T - int(bool(model.prepend_bos)) - int(bool(model.append_eos))
    if S <= 0:
        raise ValueError("pair_logits: no residue between <cls> and <eos>")
    C_out = head.n_out
    with torch.cuda.device(dev):
        eng = model._engine_ready(dev)
        eng.set_pair_head(head)
        from .design import batch_size

        step = batch_size(lambda n: eng.rows_pair_bytes(n, T, 0) + n * S * S * C_out * 4, B, max_bytes)
        out = torch.empty((B, S, S, C_out), dtype=torch.float32, device=dev)
        for lo in range(0, B, step):
            eng.forward_rows_pair(tok[lo:lo + step], None, model.alphabet_size, out[lo:lo + step])
    result = {name: out[..., slice(*head.columns(name))] for name in head.outputs}
    result.setdefault("all", out)
    return result


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m esm_amd.pair_logits",
                                description="Pair logits of a linear head on the attention maps (lm-design's projection checkpoint)")
    p.add_argument("--model-location", required=True, help="a model name or a checkpoint file (esm_amd.pretrained)")
    p.add_argument("--pair-head", required=True, help="lm-design's linear projection checkpoint")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--sequence", help="one sequence")
    src.add_argument("--fasta", help="a FASTA file; sequences of one length run together")
    p.add_argument("--output-dir", required=True, help="receives <label>.<name>.npy per sequence and output")
    p.add_argument("--max-bytes", type=int, default=8 << 30)
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    from . import checkpoint as pretrained
    from .fasta import read_fasta

    model, alphabet = pretrained.load_model_and_alphabet(args.model_location)
    model = model.eval().cuda()
    head = PairHead.from_linear_projection(args.pair_head, model)
    records = [("sequence", args.sequence)] if args.sequence else list(read_fasta(args.fasta))
    os.makedirs(args.output_dir, exist_ok=True)
    convert = alphabet.get_batch_converter()
    by_len = {}
    for label, seq in records:
        by_len.setdefault(len(seq), []).append((label.split()[0], seq))
    for group in by_len.values():  # equal lengths: no <pad>, every entry is a residue pair
        _, _, tokens = convert(group)
        out = pair_logits(model, tokens, head, max_bytes=args.max_bytes)
        for i, (label, _) in enumerate(group):
            for name in head.outputs:
                np.save(os.path.join(args.output_dir, f"{label}.{name}.npy"), out[name][i].cpu().numpy())
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
