"""MSA Transformer as a drop-in ``nn.Module`` whose forward pass runs in libesmk.so on the MI355X.

Keeps the public surface of the reference ``esm.model.msa_transformer.MSATransformer`` (reference
esm/model/msa_transformer.py:20-238): ``__init__(args, alphabet)``, attribute and state-dict key names
(``layers.{i}.row_self_attention.layer.q_proj.weight`` ...), ``forward(tokens [B,R,C], repr_layers,
need_head_weights, return_contacts)``, ``predict_contacts``, ``num_layers``, ``max_tokens_per_msa_``.
Sub-modules are parameter containers; the axial layer math (tied row attention, column attention, FFN:
reference esm/axial_attention.py, esm/modules.py:145-221,360-418) runs inside ``esmk_msa_forward``.
There is no CPU path.

``need_head_weights=True`` returns ``row_attentions [B,L,H,C,C]`` and ``col_attentions [B,L,H,C,R,R]`` as the
reference does (the latter is 58 GB in fp32 for a 12-layer 128x513 MSA: it fits the MI355X's 288 GB).  Set
``model.return_col_attentions = False`` to skip it, e.g. for ``predict_contacts`` on deep MSAs.
"""
import re

import torch
import torch.nn as nn

from .engine import MsaEngine, _EngineHost, warn_if_grad_expected
from .esm2 import ContactPredictionHead, RobertaLMHead, _Container

_AXIS = re.compile(r"row|column")


class _AxialAttention(_Container):
    def __init__(self, embed_dim, num_heads, max_tokens_per_msa):
        super().__init__()
        self.num_heads, self.head_dim = num_heads, embed_dim // num_heads
        self.max_tokens_per_msa = max_tokens_per_msa
        self.k_proj = nn.Linear(embed_dim, embed_dim)
        self.v_proj = nn.Linear(embed_dim, embed_dim)
        self.q_proj = nn.Linear(embed_dim, embed_dim)
        self.out_proj = nn.Linear(embed_dim, embed_dim)


class RowSelfAttention(_AxialAttention):
    pass


class ColumnSelfAttention(_AxialAttention):
    pass


class FeedForwardNetwork(_Container):
    def __init__(self, embed_dim, ffn_dim):
        super().__init__()
        self.fc1 = nn.Linear(embed_dim, ffn_dim)
        self.fc2 = nn.Linear(ffn_dim, embed_dim)


class NormalizedResidualBlock(_Container):
    def __init__(self, layer, embed_dim):
        super().__init__()
        self.layer = layer
        self.layer_norm = nn.LayerNorm(embed_dim)


class AxialTransformerLayer(_Container):
    def __init__(self, embed_dim, ffn_dim, heads, max_tokens_per_msa):
        super().__init__()
        self.row_self_attention = NormalizedResidualBlock(RowSelfAttention(embed_dim, heads, max_tokens_per_msa), embed_dim)
        self.column_self_attention = NormalizedResidualBlock(ColumnSelfAttention(embed_dim, heads, max_tokens_per_msa), embed_dim)
        self.feed_forward_layer = NormalizedResidualBlock(FeedForwardNetwork(embed_dim, ffn_dim), embed_dim)


class LearnedPositionalEmbedding(nn.Embedding):
    """Parameter container with the reference's table size (reference esm/modules.py:232-238)."""

    def __init__(self, num_embeddings, embedding_dim, padding_idx):
        super().__init__(num_embeddings + padding_idx + 1, embedding_dim, padding_idx)
        self.max_positions = num_embeddings


class MSATransformer(_EngineHost, nn.Module):
    _engine_class = MsaEngine
    _cpu_refusal = "esm_amd.MSATransformer runs only on an MI355X (ROCm) device; there is no CPU fallback"

    @classmethod
    def add_args(cls, parser):
        # reference esm/model/msa_transformer.py:21-86
        parser.add_argument("--num_layers", default=12, type=int, metavar="N", help="number of layers")
        parser.add_argument("--embed_dim", default=768, type=int, metavar="N", help="embedding dimension")
        parser.add_argument("--logit_bias", action="store_true", help="whether to apply bias to logits")
        parser.add_argument("--ffn_embed_dim", default=3072, type=int, metavar="N", help="embedding dimension for FFN")
        parser.add_argument("--attention_heads", default=12, type=int, metavar="N", help="number of attention heads")
        parser.add_argument("--dropout", default=0.1, type=float, help="Dropout to apply.")
        parser.add_argument("--attention_dropout", default=0.1, type=float, help="Dropout to apply.")
        parser.add_argument("--activation_dropout", default=0.1, type=float, help="Dropout to apply.")
        parser.add_argument("--max_tokens_per_msa", default=2 ** 14, type=int,
                            help="kept for compatibility: the engine never needs to chunk the attention")

    def __init__(self, args, alphabet):
        super().__init__()
        self.args = args
        self.alphabet_size = len(alphabet)
        self.padding_idx = alphabet.padding_idx
        self.mask_idx = alphabet.mask_idx
        self.cls_idx = alphabet.cls_idx
        self.eos_idx = alphabet.eos_idx
        self.prepend_bos = alphabet.prepend_bos
        self.append_eos = alphabet.append_eos
        E = args.embed_dim
        self.embed_tokens = nn.Embedding(self.alphabet_size, E, padding_idx=self.padding_idx)
        if getattr(args, "embed_positions_msa", False):
            emb_dim = getattr(args, "embed_positions_msa_dim", E)
            self.msa_position_embedding = nn.Parameter(0.01 * torch.randn(1, 1024, 1, emb_dim), requires_grad=True)
        else:
            self.register_parameter("msa_position_embedding", None)
        # reference msa_transformer.py:114: a parameter-less child kept for the module surface (named_children order);
        # the engine is forward-only and refuses training mode with non-zero dropout (see forward)
        self.dropout_module = nn.Dropout(getattr(args, "dropout", 0.0))
        mtpm = getattr(args, "max_tokens_per_msa", getattr(args, "max_tokens", 2 ** 14))
        self.layers = nn.ModuleList(
            [AxialTransformerLayer(E, args.ffn_embed_dim, args.attention_heads, mtpm) for _ in range(args.layers)])
        self.contact_head = ContactPredictionHead(args.layers * args.attention_heads, self.prepend_bos, self.append_eos,
                                                  eos_idx=self.eos_idx)
        self.embed_positions = LearnedPositionalEmbedding(args.max_positions, E, self.padding_idx)
        self.emb_layer_norm_before = nn.LayerNorm(E)
        self.emb_layer_norm_after = nn.LayerNorm(E)
        self.lm_head = RobertaLMHead(E, self.alphabet_size, self.embed_tokens.weight)
        self._engine = None
        self.return_col_attentions = True

    @property
    def num_layers(self):
        return self.args.layers

    def max_tokens_per_msa_(self, value: int) -> None:
        """reference msa_transformer.py:229-238 (the engine holds the whole MSA in HBM; kept as a no-op knob)."""
        for module in self.modules():
            if isinstance(module, (RowSelfAttention, ColumnSelfAttention)):
                module.max_tokens_per_msa = value

    def forward(self, tokens, repr_layers=[], need_head_weights=False, return_contacts=False):
        if return_contacts:
            need_head_weights = True
        assert tokens.ndim == 3
        if self.training and (self.args.dropout or self.args.attention_dropout or self.args.activation_dropout):
            raise RuntimeError("esm_amd.MSATransformer is forward-only: call .eval() (dropout is not implemented)")
        w = self._check_devices(tokens)
        warn_if_grad_expected(self)
        from . import _native as N

        dev = tokens.device
        B, R, C = tokens.shape
        if self.msa_position_embedding is not None and R > 1024:
            raise RuntimeError("Using model with MSA position embedding trained on maximum MSA "
                               f"depth of 1024, but received {R} alignments.")
        if C > self.embed_positions.max_positions:
            raise ValueError(f"Sequence length {C} above maximum  sequence length of {self.embed_positions.max_positions}")
        L, E, H, V = self.args.layers, self.args.embed_dim, self.args.attention_heads, self.alphabet_size
        repr_set = self._repr_set(repr_layers)
        with torch.cuda.device(dev):
            eng = self._engine_ready(dev)
            tok = tokens.to(torch.int64).contiguous()
            flags = N.OUT_LOGITS
            f32 = dict(dtype=torch.float32, device=dev)
            logits = torch.empty((B, R, C, V), **f32)
            reps = [torch.empty((B, R, C, E), **f32) for _ in repr_set]
            row_attn = col_attn = contacts = None
            if need_head_weights:
                flags |= N.OUT_ATTN
                row_attn = torch.empty((B, L, H, C, C), **f32)
                if self.return_col_attentions:
                    flags |= N.OUT_COL_ATTN
                    col_attn = torch.empty((B, L, H, C, R, R), **f32)
            if return_contacts:
                flags |= N.OUT_CONTACTS
                S = C - int(self.prepend_bos) - int(self.append_eos)
                contacts = torch.empty((B, S, S), **f32)
            eng.forward(tok, repr_set, reps, flags, logits, row_attn, col_attn, contacts)
        cast = self._cast_to(w.dtype)
        result = {"logits": cast(logits), "representations": {l: cast(r) for l, r in zip(repr_set, reps)}}
        if need_head_weights:
            if col_attn is not None:
                result["col_attentions"] = cast(col_attn)
            result["row_attentions"] = cast(row_attn)
            if return_contacts:
                result["contacts"] = cast(contacts)
        return result

    def predict_contacts(self, tokens):
        return self(tokens, return_contacts=True)["contacts"]

    supports_scoring = False  # esmk_forward_rows takes single-sequence models only; MSAs: the msa_* methods below

    def masked_marginals(self, tokens, positions=None, chunk=None, **kwargs):
        from . import scoring

        scoring._refuse_msa(self)

    wt_marginals = pseudo_log_likelihood = masked_marginals

    def masked_joint(self, *args, **kwargs):
        from . import scoring

        scoring._refuse_msa(self)

    score_variants = masked_joint
    gibbs_sample = inpaint = masked_joint  # esm_amd.sampling draws single sequences only
    categorical_jacobian = jacobian_contacts = masked_joint  # esm_amd.jacobian substitutes in single sequences only
    design = design_energy = masked_joint  # esm_amd.design runs chains of single sequences only
    forward_windows = masked_joint  # esm_amd.windows cuts single sequences into windows only

    def stream_edits(self, *args, **kwargs):
        from . import interventions

        interventions.plan_edits(self, [])  # NotImplementedError: the axial stack has no edit point

    forward_edited = stream_edits

    def embed_layer(self, *args, **kwargs):
        from . import search

        search.check_model(self, None)  # NotImplementedError: the early exit and the pooled index run single sequences

    pool = search = embed_layer

    # Variant scoring of one MSA (esm_amd/msa_scoring.py over esmk_msa_forward_rows): an MSA plus a query row is another
    # argument shape than a batch of sequences, hence names of their own; the single-sequence names above keep refusing
    def msa_forward_rows(self, tokens, sel_rows, return_logits=False):
        from . import msa_scoring

        return msa_scoring.msa_forward_rows(self, tokens, sel_rows, return_logits=return_logits)

    def msa_masked_marginals(self, tokens, positions=None, row=0, chunk=None):
        from . import msa_scoring

        return msa_scoring.msa_masked_marginals(self, tokens, positions=positions, row=row, chunk=chunk)

    def msa_wt_marginals(self, tokens, row=0):
        from . import msa_scoring

        return msa_scoring.msa_wt_marginals(self, tokens, row=row)

    def msa_masked_joint(self, tokens, position_sets, row=0, chunk=None, return_logits=False):
        from . import msa_scoring

        return msa_scoring.msa_masked_joint(self, tokens, position_sets, row=row, chunk=chunk, return_logits=return_logits)

    def msa_score_variants(self, alphabet, msa, variants, strategy="masked-marginals", offset_idx=0, sep=":", chunk=None):
        from . import msa_scoring

        return msa_scoring.msa_score_variants(self, alphabet, msa, variants, strategy=strategy, offset_idx=offset_idx, sep=sep,
                                              chunk=chunk)

    def msa_score_variants_ensemble(self, alphabet, msa, variants, num_seqs, n_subsamples=5, subsample="weighted", theta=0.2,
                                    seed=0, strategy="masked-marginals", offset_idx=0, sep=":", chunk=None):
        from . import msa_scoring

        return msa_scoring.msa_score_variants_ensemble(self, alphabet, msa, variants, num_seqs, n_subsamples=n_subsamples,
                                                       subsample=subsample, theta=theta, seed=seed, strategy=strategy,
                                                       offset_idx=offset_idx, sep=sep, chunk=chunk)


def build_from_checkpoint(model_data):
    """``{"args": Namespace(arch="msa_transformer", ...), "model": state}`` -> (model, alphabet), following
    reference esm/pretrained.py:111-127 (prefix stripping, embed_positions_msa_dim from the tensor)."""
    from .alphabet import Alphabet
    from .checkpoint import strip_arg_prefix, strip_key_prefix

    args = model_data["args"]
    # the released checkpoints name the two axial attentions the other way round from the module attributes
    # (pretrained.py:111-124): "row" <-> "column" in every tensor name, after the usual prefix stripping
    swap_axes = lambda key: _AXIS.sub(lambda m: "column" if m.group(0) == "row" else "row", key)
    model_args = {strip_arg_prefix(k): v for k, v in vars(args).items()}
    state = {strip_key_prefix(swap_axes(k)): v for k, v in model_data["model"].items()}
    if model_args.get("embed_positions_msa", False):
        model_args["embed_positions_msa_dim"] = state["msa_position_embedding"].size(-1)
    import argparse

    alphabet = Alphabet.from_architecture("msa_transformer")
    model = MSATransformer(argparse.Namespace(**model_args), alphabet)
    return model, alphabet, state
