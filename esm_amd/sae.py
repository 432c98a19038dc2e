"""Reading the residual stream in the basis of a sparse autoencoder (SAE): per-residue top-k features and per-protein maxima.

``StreamEdit`` / ``forward_edited`` / ``stream_edits`` WRITE into the stream; this module READS it in an interpretable basis — the
other half of that workflow.  SAEs trained on ESM-2 representations are published (ReLU dictionaries of ~10 k features, top-k
SAEs of 4 k - 16 k latents); nothing is downloaded and no SAE ships with the project: ``SparseAutoencoder.from_state_dict`` reads
a checkpoint of either common key spelling.

    sae = SparseAutoencoder.from_state_dict("sae_layer24.pt")
    out = model.sae_features(tokens, sae, layer=24, top_k=32, protein_max=True)
    out["rows"]      int32 [n, 2]   (sequence, token position) of the scored rows, ascending
    out["indices"]   int32 [n, k]   the k most active features of every row, value descending, ties to the lower index; -1: unused
    out["values"]    fp32  [n, k]   their activations; 0: unused
    out["n_active"]  int32 [n]      the row's L0 before truncation to k
    out["protein_max"] fp32 [B, F], out["protein_argmax"] int32 [B, F]     per sequence, the largest activation and its position
    steer = StreamEdit(24, "add", value=sae.direction(f), gain=4.0)

Definition.  For a row x of ``forward(tokens, repr_layers=[layer])["representations"][layer]`` (fp32):
    u[e] = input_scale * x[e] - b_dec[e]          (two fp32 roundings, never fused; b_dec None: zeros)
    z[f] = <w_enc[f], u> + b_enc[f]
feature f is ACTIVE iff z[f] > threshold[f] (NaN: never; +inf: active); its activation is z[f] if active, else 0; a top-k SAE
keeps only the ``k`` largest active features of a row.  The product runs on the 16-bit matrix rate with both operands split in
fp16 parts (the f16x3 form of the dense GEMM, near-fp32 products: tests/test_precision_ops_gpu.py::test_f16x3_product), so no
[n, F] matrix beyond one chunk of scratch is ever held; selection, segment maximum and decode are exact (csrc/sae.hip).

COORDINATES.  x is the representation exactly as ``forward`` returns it — the coordinates such SAEs are trained in.  For
``layer == num_layers`` that is AFTER the final LayerNorm, while ``StreamEdit``'s layer L is the stream IN FRONT of that
LayerNorm: a direction of an SAE trained on the last representation does not live in the space ``StreamEdit(L, ...)`` writes to.
For ``layer < num_layers`` the two coincide.

Not built: stopping the layer stack at ``layer`` (the layers above still run), the MSA Transformer, windows (``window=``),
training SAEs, a "clamp feature f to c" edit, the reconstruction error over ALL active features of a ReLU SAE (``decode`` uses the
reported k), transcoders.
"""
import math

import numpy as np
import torch

MAX_FEATURES = 65536
MAX_TOP_K = 256
DEFAULT_TOP_K = 32
_CHUNK_MULTIPLE = 256


def _f32(t, what, shape=None):
    t = torch.as_tensor(t).detach().to("cpu", torch.float32).contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"SparseAutoencoder: {what} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


class SparseAutoencoder:
    """An SAE on a model's representations (module docstring: the definition and the coordinates).  w_enc [F, E], b_enc [F],
    w_dec [F, E] or None (then no ``decode`` / ``direction``), b_dec [E] or None (zeros); ``activation`` "relu" or "topk" (with
    ``k``, at most 256); ``threshold`` a float or an [F] tensor, all >= 0; ``input_scale`` the factor the SAE's training applied
    to the representation.  F is at most 65536; inside, F is padded to a multiple of 64 by features with zero weights, zero
    bias and threshold +inf, which are never active and never reported."""

    def __init__(self, w_enc, b_enc, w_dec=None, b_dec=None, activation="relu", k=None, threshold=None, input_scale=1.0):
        w_enc = torch.as_tensor(w_enc)
        if w_enc.dim() != 2:
            raise ValueError(f"SparseAutoencoder: w_enc must be [F, E], got {tuple(w_enc.shape)}")
        F, E = w_enc.shape
        if not 1 <= F <= MAX_FEATURES:
            raise ValueError(f"SparseAutoencoder: F = {F} features, at most {MAX_FEATURES} are supported")
        if E % 4 != 0:
            raise ValueError(f"SparseAutoencoder: E = {E} must be a multiple of 4")
        if activation not in ("relu", "topk"):
            raise ValueError(f"SparseAutoencoder: activation must be 'relu' or 'topk', got {activation!r}")
        if activation == "topk":
            if k is None or not 1 <= int(k) <= MAX_TOP_K:
                raise ValueError(f"SparseAutoencoder: a top-k SAE needs k in 1 .. {MAX_TOP_K}, got {k}")
            k = int(k)
        elif k is not None:
            raise ValueError("SparseAutoencoder: k goes with activation='topk'")
        input_scale = float(input_scale)
        if not math.isfinite(input_scale) or input_scale == 0.0:
            raise ValueError("SparseAutoencoder: input_scale must be finite and not 0")
        self.F, self.E, self.activation, self.k, self.input_scale = int(F), int(E), activation, k, input_scale
        self.Fp = (self.F + 63) // 64 * 64
        self.w_enc = _f32(w_enc, "w_enc")
        self.b_enc = _f32(b_enc, "b_enc", (F,))
        self.w_dec = None if w_dec is None else _f32(w_dec, "w_dec", (F, E))
        self.b_dec = None if b_dec is None else _f32(b_dec, "b_dec", (E,))
        if threshold is None:
            threshold = 0.0
        if isinstance(threshold, (int, float)):
            thr = torch.full((F,), float(threshold), dtype=torch.float32)
        else:
            thr = _f32(threshold, "threshold", (F,))
        if not bool((thr >= 0).all()):  # (also refuses NaN)
            raise ValueError("SparseAutoencoder: thresholds must be >= 0 (active values are then positive floats, which the "
                             "selection's integer keys rely on)")
        self.threshold = thr
        self.inv_scale = float(np.float32(1.0 / input_scale))  # rounded once, on the host
        self._dev = {}

    # ---- checkpoints ----------------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, path_or_state_dict, **overrides):
        """An SAE from a checkpoint of one of two key spellings (a path is read with ``torch.load(weights_only=True)``):
        ``encoder.weight [F,E]``, ``encoder.bias``, ``decoder.weight [E,F]``, ``bias [E]``;  or  ``W_enc [E,F]``, ``b_enc``,
        ``W_dec [F,E]``, ``b_dec``.  ``overrides``: constructor keywords (activation, k, threshold, input_scale)."""
        sd = path_or_state_dict
        if not isinstance(sd, dict):
            sd = torch.load(sd, map_location="cpu", weights_only=True)
        keys = set(sd)
        if {"encoder.weight", "encoder.bias", "decoder.weight"} <= keys:
            kw = dict(w_enc=sd["encoder.weight"], b_enc=sd["encoder.bias"], w_dec=sd["decoder.weight"].t(), b_dec=sd.get("bias"))
        elif {"W_enc", "b_enc", "W_dec"} <= keys:
            kw = dict(w_enc=sd["W_enc"].t(), b_enc=sd["b_enc"], w_dec=sd["W_dec"], b_dec=sd.get("b_dec"))
        else:
            raise ValueError("SparseAutoencoder.from_state_dict: expected the keys encoder.weight / encoder.bias / decoder.weight "
                             f"/ bias or W_enc / b_enc / W_dec / b_dec, found {sorted(keys)}")
        kw.update(overrides)
        return cls(**kw)

    # ---- device state ---------------------------------------------------------------------------------------------------
    @property
    def Ep(self):
        return (self.E + 63) // 64 * 64

    def padded(self):
        """(w_enc [Fp, Ep], b_enc [Fp], threshold [Fp]) on the host: the padding features have zero weights, zero bias and
        threshold +inf; the padding columns are zero."""
        w = torch.zeros((self.Fp, self.Ep), dtype=torch.float32)
        w[:self.F, :self.E] = self.w_enc
        b = torch.zeros((self.Fp,), dtype=torch.float32)
        b[:self.F] = self.b_enc
        t = torch.full((self.Fp,), float("inf"), dtype=torch.float32)
        t[:self.F] = self.threshold
        return w, b, t

    def on(self, device):
        """The SAE's device tensors, built once per device: the fp16 ``hi | lo | hi`` encoder image [Fp, 3 Ep]
        (``esmk_op_split_weight_ex(parts=3)``), b_enc and threshold [Fp], b_dec [E], w_dec [F, E]."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("SparseAutoencoder runs only on an MI355X (ROCm) device; there is no CPU fallback")
        key = (device.type, torch.cuda.current_device() if device.index is None else device.index)
        st = self._dev.get(key)
        if st is None:
            from . import ops

            with torch.cuda.device(key[1]):
                dev = torch.device("cuda", key[1])
                w, b, t = self.padded()
                w3 = torch.zeros((self.Fp, 3 * self.Ep), dtype=torch.float16, device=dev)
                ops.split_weight_ex(w.to(dev), w3, self.Ep, 3)
                st = dict(w3=w3, b_enc=b.to(dev), threshold=t.to(dev),
                          b_dec=None if self.b_dec is None else self.b_dec.to(dev),
                          w_dec=None if self.w_dec is None else self.w_dec.to(dev))
            self._dev[key] = st
        return st

    # ---- decode and directions ------------------------------------------------------------------------------------------
    def decode(self, indices, values):
        """fp32 [n, E]: x^[e] = inv_scale * (b_dec[e] + sum_r values[r] * w_dec[indices[r], e]), the sum taken rank by rank
        from r = 0 with one rounded product and one rounded add per term (numpy float32 reproduces it bit for bit); index -1
        is skipped; inv_scale = float32(1 / input_scale)."""
        from . import ops

        if self.w_dec is None:
            raise ValueError("SparseAutoencoder.decode: this SAE has no decoder (w_dec)")
        st = self.on(indices.device)
        with torch.cuda.device(indices.device):
            return ops.sae_decode(indices.contiguous(), values.contiguous(), st["w_dec"], st["b_dec"], self.inv_scale)

    def direction(self, f):
        """fp32 [E]: inv_scale * w_dec[f], the direction feature ``f`` writes into the representation — ready for
        ``StreamEdit(layer, "add", value=sae.direction(f), gain=g)`` (module docstring: the coordinates at layer L)."""
        if self.w_dec is None:
            raise ValueError("SparseAutoencoder.direction: this SAE has no decoder (w_dec)")
        if not 0 <= int(f) < self.F:
            raise ValueError(f"SparseAutoencoder.direction: feature {f} is outside 0 .. {self.F - 1}")
        return torch.from_numpy(np.float32(self.inv_scale) * self.w_dec[int(f)].numpy())


# ---- the call ---------------------------------------------------------------------------------------------------------------
def plan_chunks(n, F, E, max_bytes, dense_bytes=0):
    """[(first row, rows)] of the chunks of ``n`` scored rows whose scratch — the fp16 operand image [chunk, 3 Ep] plus z fp32
    [chunk, Fp] — fits ``max_bytes`` (less ``dense_bytes`` held for a returned dense matrix).  Chunk sizes are multiples of 256
    rows, except the last; a budget below one such chunk is a ValueError."""
    Fp, Ep = (F + 63) // 64 * 64, (E + 63) // 64 * 64
    per_row = 6 * Ep + 4 * Fp
    budget = int(max_bytes) - int(dense_bytes)
    chunk = budget // per_row // _CHUNK_MULTIPLE * _CHUNK_MULTIPLE
    if chunk < _CHUNK_MULTIPLE:
        raise ValueError(f"sae_features: max_bytes = {max_bytes} does not hold one chunk of {_CHUNK_MULTIPLE} rows "
                         f"({_CHUNK_MULTIPLE * per_row + dense_bytes} bytes are needed)")
    return [(lo, min(chunk, n - lo)) for lo in range(0, n, chunk)]


def _check_call(model, sae, layer, top_k, positions, window):
    from .msa_transformer import MSATransformer

    if isinstance(model, MSATransformer):
        raise NotImplementedError("sae_features is built for ESM-2, ESM-1b / ESM-1v and ESM-1; not for the MSA Transformer")
    if window is not None:
        raise NotImplementedError("sae_features: windows (window=) are not built")
    if not isinstance(sae, SparseAutoencoder):
        raise TypeError(f"sae_features: expected a SparseAutoencoder, got {type(sae).__name__}")
    if sae.E != int(model.embed_dim):
        raise ValueError(f"sae_features: the SAE reads {sae.E} columns, the model's embed_dim is {int(model.embed_dim)}")
    if not 0 <= int(layer) <= int(model.num_layers):
        raise ValueError(f"sae_features: layer {layer} is outside 0 .. {int(model.num_layers)}")
    if positions not in ("residues", "all"):
        raise ValueError("sae_features: positions must be 'residues' or 'all'")
    if top_k is None:
        top_k = sae.k if sae.activation == "topk" else DEFAULT_TOP_K
    top_k = int(top_k)
    if not 1 <= top_k <= MAX_TOP_K:
        raise ValueError(f"sae_features: top_k must be 1 .. {MAX_TOP_K}, got {top_k}")
    if sae.activation == "topk" and top_k > sae.k:
        raise ValueError(f"sae_features: top_k = {top_k} exceeds the {sae.k} features this top-k SAE keeps per row")
    return top_k


def scored_rows(model, tokens, positions):
    """int32 [n, 2] (sequence, token position) of the rows ``positions`` selects, ascending, on the tokens' device: "all"
    leaves out <pad>, "residues" also <cls> and <eos>."""
    keep = tokens.ne(model.padding_idx)
    if positions == "residues":
        for v in (model.cls_idx, model.eos_idx):
            if v is not None:
                keep &= tokens.ne(v)
    return keep.nonzero().to(torch.int32).contiguous()


def sae_features(model, tokens, sae, layer, top_k=None, positions="residues", varlen=False, protein_max=False, return_dense=False,
                 max_bytes=2 << 30, window=None):
    """The SAE features of representation ``layer`` of every scored row of ``tokens`` [B, T] (module docstring): a dict of device
    tensors ``rows``, ``indices``, ``values``, ``n_active`` and, when asked for, ``protein_max`` / ``protein_argmax`` [B, F] and
    ``dense`` fp32 [n, F] (z; a ValueError if it does not fit ``max_bytes``).  ``top_k`` None: ``sae.k`` for a top-k SAE, else 32;
    ``varlen=True`` runs the layer stack through ``forward_varlen``.  Inside ``with model.stream_edits(...)`` the edited stream
    is read.  The scored rows are cut into chunks whose scratch fits ``max_bytes``; per chunk four launches on one stream
    (image, GEMM, top-k, segment maximum) and no host read in between."""
    top_k = _check_call(model, sae, layer, top_k, positions, window)
    assert tokens.ndim == 2
    layer = int(layer)
    if varlen:
        rep = model.forward_varlen(tokens, repr_layers=[layer])["representations"][layer]
    else:
        rep = model.forward(tokens, repr_layers=[layer])["representations"][layer]
    with torch.cuda.device(rep.device):
        rows = scored_rows(model, tokens.to(rep.device), positions)
        return features_of_rows(sae, rep, rows, top_k, protein_max=protein_max, return_dense=return_dense, max_bytes=max_bytes)


def features_of_rows(sae, rep, rows, top_k, protein_max=False, return_dense=False, max_bytes=2 << 30):
    """``sae_features`` behind the forward: ``rep`` [B, T, E] a captured representation on the device, ``rows`` int32 [n, 2] the
    scored (sequence, position) pairs, ascending.  Per chunk: the operand image, the dense GEMM, the top-k, the segment maximum."""
    from . import _native as N
    from . import ops

    B, T, _ = rep.shape
    dev = rep.device
    E, F, Fp, Ep = sae.E, sae.F, sae.Fp, sae.Ep
    x = rep.reshape(B * T, E).to(torch.float32).contiguous()
    st = sae.on(dev)
    n = rows.shape[0]
    dense = None
    if return_dense:
        if n * F * 4 > max_bytes:
            raise ValueError(f"sae_features: return_dense needs {n * F * 4} bytes for [n = {n}, F = {F}] fp32, max_bytes is "
                             f"{max_bytes}")
        dense = torch.empty((n, F), dtype=torch.float32, device=dev)
    chunks = plan_chunks(n, F, E, max_bytes, 0 if dense is None else n * F * 4)
    flat = (rows[:, 0] * T + rows[:, 1]).contiguous()
    indices = torch.empty((n, top_k), dtype=torch.int32, device=dev)
    values = torch.empty((n, top_k), dtype=torch.float32, device=dev)
    n_active = torch.empty((n,), dtype=torch.int32, device=dev)
    out = dict(rows=rows, indices=indices, values=values, n_active=n_active)
    k_sae = sae.k if sae.activation == "topk" else 0
    if protein_max:
        pmax = torch.zeros((B, Fp), dtype=torch.float32, device=dev)
        parg = torch.full((B, Fp), -1, dtype=torch.int32, device=dev)
        counts = torch.bincount(rows[:, 0].long(), minlength=B)
        seg_start = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).to(torch.int32).contiguous()
    cap = max((c for _, c in chunks), default=0)
    image = torch.empty((max(cap, 1), 3 * Ep), dtype=torch.float16, device=dev)
    z = torch.empty((max(cap, 1), Fp), dtype=torch.float32, device=dev)
    for lo, c in chunks:
        ops.sae_rows(x, flat[lo:lo + c], st["b_dec"], sae.input_scale, out=image, n=c)
        ops.linear(image[:c], st["w3"], st["b_enc"], N.EPI_STORE_F32, out=z[:c])
        r = ops.sae_topk(z, top_k, st["threshold"], k_sae=k_sae, n=c, indices=indices[lo:lo + c], values=values[lo:lo + c],
                         n_active=n_active[lo:lo + c], want_cutoff=protein_max and k_sae > 0)
        if protein_max:
            ops.sae_segment_max(z, rows[lo:lo + c], seg_start, pmax, parg, st["threshold"], cutoff=r.get("cutoff"), row0=lo, n=c)
        if dense is not None:
            dense[lo:lo + c] = z[:c, :F]
    if protein_max:
        out["protein_max"] = pmax[:, :F].contiguous()
        out["protein_argmax"] = parg[:, :F].contiguous()
    if dense is not None:
        out["dense"] = dense
    return out


# ---- command line -----------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    import argparse

    p = argparse.ArgumentParser(prog="python -m esm_amd.sae_features",
                                description="Sparse-autoencoder features of a representation: top-k per residue, maxima per protein")
    p.add_argument("--model-location", required=True, help="a model name or a checkpoint file (esm_amd.pretrained)")
    p.add_argument("--sae", required=True, help="the SAE checkpoint (SparseAutoencoder.from_state_dict)")
    p.add_argument("--layer", type=int, required=True, help="the representation the SAE reads (0 .. num_layers)")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--sequence", help="one sequence")
    src.add_argument("--fasta", help="a FASTA file")
    p.add_argument("--output-dir", required=True, help="receives <label>.sae_idx.npy and <label>.sae_val.npy per record")
    p.add_argument("--top-k", type=int, default=None, help="features kept per row (default: the SAE's k, or 32)")
    p.add_argument("--positions", choices=("residues", "all"), default="residues")
    p.add_argument("--protein-max", action="store_true", help="also write protein_max.npy, protein_argmax.npy and labels.txt")
    p.add_argument("--no-varlen", dest="varlen", action="store_false", help="run padded batches instead of token-packed ones")
    p.add_argument("--activation", choices=("relu", "topk"), default=None, help="override the SAE's activation")
    p.add_argument("--sae-k", type=int, default=None, help="k of a top-k SAE (with --activation topk)")
    p.add_argument("--batch-tokens", type=int, default=16384, help="tokens per batch")
    p.add_argument("--max-bytes", type=int, default=2 << 30)
    return p.parse_args(argv)


def main(argv=None):
    import os

    args = parse_args(argv)
    from . import checkpoint as pretrained
    from .fasta import read_fasta

    model, alphabet = pretrained.load_model_and_alphabet(args.model_location)
    model = model.eval().cuda()
    overrides = {}
    if args.activation is not None:
        overrides["activation"] = args.activation
    if args.sae_k is not None:
        overrides["k"] = args.sae_k
    sae = SparseAutoencoder.from_state_dict(args.sae, **overrides)
    records = [("sequence", args.sequence)] if args.sequence else [(label.split()[0], seq) for label, seq in read_fasta(args.fasta)]
    os.makedirs(args.output_dir, exist_ok=True)
    convert = alphabet.get_batch_converter()
    order = sorted(range(len(records)), key=lambda i: len(records[i][1]))  # similar lengths share a batch
    pmax = np.zeros((len(records), sae.F), dtype=np.float32)
    parg = np.full((len(records), sae.F), -1, dtype=np.int32)
    lo = 0
    while lo < len(order):
        hi, longest = lo, 0
        while hi < len(order) and (hi == lo or max(longest, len(records[order[hi]][1]) + 2) * (hi + 1 - lo) <= args.batch_tokens):
            longest = max(longest, len(records[order[hi]][1]) + 2)
            hi += 1
        group = [records[i] for i in order[lo:hi]]
        _, _, tokens = convert(group)
        out = sae_features(model, tokens, sae, args.layer, top_k=args.top_k, positions=args.positions,
                           varlen=args.varlen and getattr(model, "supports_varlen", False), protein_max=args.protein_max,
                           max_bytes=args.max_bytes)
        seq = out["rows"][:, 0].cpu().numpy()
        idx, val = out["indices"].cpu().numpy(), out["values"].cpu().numpy()
        for j, (label, _) in enumerate(group):
            np.save(os.path.join(args.output_dir, f"{label}.sae_idx.npy"), idx[seq == j])
            np.save(os.path.join(args.output_dir, f"{label}.sae_val.npy"), val[seq == j])
        if args.protein_max:
            pmax[order[lo:hi]] = out["protein_max"].cpu().numpy()
            parg[order[lo:hi]] = out["protein_argmax"].cpu().numpy()
        lo = hi
    if args.protein_max:
        np.save(os.path.join(args.output_dir, "protein_max.npy"), pmax)
        np.save(os.path.join(args.output_dir, "protein_argmax.npy"), parg)
        with open(os.path.join(args.output_dir, "labels.txt"), "w") as fh:
            fh.writelines(label + "\n" for label, _ in records)
    return 0
