"""ESM-1b / ESM-1v (``ProteinBertModel`` with ``args.arch == "roberta_large"``) on the MI355X engine.

Same public surface as the reference class (reference esm/model/esm1.py:22-200): ``__init__(args, alphabet)``,
state-dict key names, ``forward(tokens, repr_layers, need_head_weights, return_contacts)``,
``predict_contacts``, ``num_layers``.  The layer stack is the ESM-2 one without rotary embeddings
(``TransformerLayer(use_rotary_embeddings=False)``, esm1.py:71-82) plus a learned positional embedding and
``emb_layer_norm_before`` (esm1.py:88-104,133-139); ``forward`` is inherited from ``esm_amd.ESM2`` and runs in
``esmk_forward`` with the ``no_rope / num_positions / ln_before`` fields of ``esmk_config`` set.

The original ESM-1 models (any other arch, in practice ``protein_bert_base``; esm1.py:107-114) differ in the embedding
(x sqrt(E), sinusoidal positions, no embedding LayerNorm, no pad zeroing), the LayerNorm eps (1e-12), the attention (one
learned null key / value pair per layer, ``bias_k`` / ``bias_v``) and the output (no final LayerNorm, untied ``embed_out``):
``esmk_config.no_rope = ESMK_ESM1`` selects all of it.  No LayerNorm fold, no split-operand precision modes and no token-packed batches for
this family: ``forward_varlen`` runs ``forward``.
"""
import math

import torch
import torch.nn as nn

from .esm2 import ESM2, ContactPredictionHead, RobertaLMHead, TransformerLayer, _Container
from .msa_transformer import LearnedPositionalEmbedding


class SinusoidalPositionalEmbedding(_Container):
    """Carries the ``_float_tensor`` buffer of reference esm/modules.py:260-266; the table itself is built by the engine."""

    def __init__(self, embed_dim, padding_idx):
        super().__init__()
        self.embed_dim, self.padding_idx = embed_dim, padding_idx
        self.register_buffer("_float_tensor", torch.FloatTensor(1).zero_())
        self.weights = None


class ProteinBertModel(ESM2):
    @classmethod
    def add_args(cls, parser):
        # reference esm/model/esm1.py:23-46
        parser.add_argument("--num_layers", default=36, type=int, metavar="N", help="number of layers")
        parser.add_argument("--embed_dim", default=1280, type=int, metavar="N", help="embedding dimension")
        parser.add_argument("--logit_bias", action="store_true", help="whether to apply bias to logits")
        parser.add_argument("--ffn_embed_dim", default=5120, type=int, metavar="N", help="embedding dimension for FFN")
        parser.add_argument("--attention_heads", default=20, type=int, metavar="N", help="number of attention heads")

    def __init__(self, args, alphabet):
        nn.Module.__init__(self)
        self.args = args
        esm1 = getattr(args, "arch", None) != "roberta_large"  # as the reference decides (esm1.py:60-65)
        self.model_version = "ESM-1" if esm1 else "ESM-1b"
        self.num_layers_ = args.layers
        self.embed_dim = args.embed_dim
        self.ffn_embed_dim = args.ffn_embed_dim
        self.attention_heads = args.attention_heads
        self.alphabet = alphabet
        self.alphabet_size = len(alphabet)
        self.padding_idx = alphabet.padding_idx
        self.mask_idx = alphabet.mask_idx
        self.cls_idx = alphabet.cls_idx
        self.eos_idx = alphabet.eos_idx
        self.prepend_bos = alphabet.prepend_bos
        self.append_eos = alphabet.append_eos
        self.token_dropout = bool(getattr(args, "token_dropout", False))
        ln_before = bool(getattr(args, "emb_layer_norm_before", False))
        E = self.embed_dim
        self._engine = None
        if esm1:
            self._init_submodules_esm1(args)
            return
        self.embed_scale = 1
        self.embed_tokens = nn.Embedding(self.alphabet_size, E, padding_idx=self.padding_idx)
        self.layers = nn.ModuleList([TransformerLayer(E, self.ffn_embed_dim, self.attention_heads)
                                     for _ in range(args.layers)])
        for layer in self.layers:  # no rotary embedding in ESM-1b: drop the inv_freq buffer from the state dict
            del layer.self_attn.rot_emb
        self.contact_head = ContactPredictionHead(args.layers * self.attention_heads, self.prepend_bos,
                                                  self.append_eos, eos_idx=self.eos_idx)
        self.embed_positions = LearnedPositionalEmbedding(args.max_positions, E, self.padding_idx)
        self.emb_layer_norm_before = nn.LayerNorm(E) if ln_before else None
        self.emb_layer_norm_after = nn.LayerNorm(E)
        self.lm_head = RobertaLMHead(E, self.alphabet_size, self.embed_tokens.weight)
        self._engine = None

    def _init_submodules_esm1(self, args):
        """reference esm1.py:67-89,107-114 with add_bias_kv=True and ESM1LayerNorm (weight / bias, eps 1e-12)."""
        E = self.embed_dim
        if E % self.attention_heads != 0 or E // self.attention_heads != 64:
            raise NotImplementedError(f"ESM-1 models run on the MI355X engine with head_dim 64 only (embed_dim {E}, "
                                      f"{self.attention_heads} heads)")
        self.embed_scale = math.sqrt(E)
        self.embed_tokens = nn.Embedding(self.alphabet_size, E, padding_idx=self.padding_idx)
        self.layers = nn.ModuleList([TransformerLayer(E, self.ffn_embed_dim, self.attention_heads) for _ in range(args.layers)])
        for layer in self.layers:
            del layer.self_attn.rot_emb
            layer.self_attn.bias_k = nn.Parameter(torch.zeros(1, 1, E))
            layer.self_attn.bias_v = nn.Parameter(torch.zeros(1, 1, E))
            layer.self_attn_layer_norm.eps = layer.final_layer_norm.eps = 1e-12
        self.contact_head = ContactPredictionHead(args.layers * self.attention_heads, self.prepend_bos, self.append_eos,
                                                  eos_idx=self.eos_idx)
        self.embed_positions = SinusoidalPositionalEmbedding(E, self.padding_idx)
        self.embed_out = nn.Parameter(torch.zeros((self.alphabet_size, E)))
        self.embed_out_bias = nn.Parameter(torch.zeros(self.alphabet_size)) if args.final_bias else None

    def _engine_config(self):
        """What esm_amd.engine.Esm2Engine sets in esmk_config besides the dimensions: ESM-1 -> no_rope = ESMK_ESM1
        (| ESMK_ESM1_FINAL_BIAS); ESM-1b / ESM-1v -> no_rope, the size of the position table, the embedding LayerNorm."""
        if self.model_version == "ESM-1":
            return dict(esm1=True, final_bias=self.embed_out_bias is not None)
        return dict(no_rope=1, num_positions=self.embed_positions.weight.shape[0],
                    ln_before=self.emb_layer_norm_before is not None)

    def _packs(self):
        return self.model_version != "ESM-1" and super()._packs()

    def _fold_setting(self, gains_known=False):
        # ESM-1 has no LayerNorm fold (eps 1e-12, no final LayerNorm to fold): off whatever ESM_AMD_LN_FOLD says
        return -1 if self.model_version == "ESM-1" else super()._fold_setting(gains_known)

    @property
    def num_layers(self):
        return self.args.layers

    @num_layers.setter
    def num_layers(self, v):  # ESM2.__init__ is bypassed; kept so generic code may assign
        self.args.layers = v

    def forward(self, tokens, repr_layers=[], need_head_weights=False, return_contacts=False, **kw):
        if self.model_version == "ESM-1":  # sinusoidal positions: no maximum length
            return super().forward(tokens, repr_layers, need_head_weights, return_contacts, **kw)
        if tokens.ndim == 2 and tokens.size(1) > self.embed_positions.max_positions:
            raise ValueError(f"Sequence length {tokens.size(1)} above maximum  sequence length of "
                             f"{self.embed_positions.max_positions}")
        return super().forward(tokens, repr_layers, need_head_weights, return_contacts, **kw)


def build_from_checkpoint(model_data):
    """``{"args": Namespace(arch="roberta_large" | "protein_bert_base", ...), "model": state}`` -> (model, alphabet, state),
    following reference esm/pretrained.py:87-110."""
    import argparse

    from .alphabet import Alphabet
    from .checkpoint import strip_arg_prefix, strip_key_prefix

    alphabet = Alphabet.from_architecture(model_data["args"].arch)
    if model_data["args"].arch == "protein_bert_base":
        # ESM-1: hyper-parameters "decoder_<name>", tensors "decoder.<key>"; nothing else is touched
        model_args = {strip_arg_prefix(k, "decoder_"): v for k, v in vars(model_data["args"]).items()}
        state = {strip_key_prefix(k, "decoder."): v for k, v in model_data["model"].items()}
        return ProteinBertModel(argparse.Namespace(**model_args), alphabet), alphabet, state
    # fairseq-era checkpoints: hyper-parameters are "encoder_<name>", tensors "encoder.sentence_encoder.<key>" /
    # "encoder.<key>" 
    model_args = {strip_arg_prefix(k): v for k, v in vars(model_data["args"]).items()}
    state = {strip_key_prefix(k): v for k, v in model_data["model"].items()}
    state["embed_tokens.weight"][alphabet.mask_idx].zero_()  # for token dropout (pretrained.py:97)
    model_args["emb_layer_norm_before"] = any(k.startswith("emb_layer_norm_before") for k in state)
    model = ProteinBertModel(argparse.Namespace(**model_args), alphabet)
    return model, alphabet, state
