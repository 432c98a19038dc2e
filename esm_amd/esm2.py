"""ESM-2 as a drop-in ``nn.Module`` whose forward pass runs in libesmk.so on the MI355X.

The class keeps the public surface of the reference ``esm.model.esm2.ESM2`` (reference
esm/model/esm2.py:15-147): constructor arguments, attribute names, state-dict key names
(``layers.{i}.self_attn.q_proj.weight`` ...), ``forward(tokens, repr_layers, need_head_weights,
return_contacts)`` and ``predict_contacts``.  The sub-modules below are *parameter containers*
with the reference's names; no layer math is done in Python/torch — ``forward`` hands raw device
pointers to ``esmk_forward`` (include/esmk.h).  There is no CPU path: CPU tensors raise.
"""
from typing import Union

import torch
import torch.nn as nn

from .alphabet import Alphabet
# (the environment readers are re-exported under the names tests and tools import from this module)
from .engine import Esm2Engine as _Engine  # noqa: F401
from .engine import (_FOLD_HAZARD_MAX, _dual_stream_wanted, _dual_stream_window, _EngineHost, _ln_fold,  # noqa: F401
                     _native_lowp, _operand_dtype_for, _weight_split, check_finite, ln_fold_hazard, warn_if_grad_expected)


class _Container(nn.Module):
    """Holds parameters under the reference's names; calling it is an error by design."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError(
            f"{type(self).__name__} is a parameter container of the MI355X engine; "
            "the layer math runs inside ESM2.forward (libesmk.so), not per sub-module; what a forward hook would change "
            "between layers is stated as esm_amd.StreamEdit (model.forward_edited, model.stream_edits)"
        )


class RotaryEmbedding(_Container):
    """Carries the ``inv_freq`` buffer of reference esm/rotary_embedding.py:40-41."""

    def __init__(self, dim: int):
        super().__init__()
        inv_freq = 1.0 / (10000 ** (torch.arange(0, dim, 2).float() / dim))
        self.register_buffer("inv_freq", inv_freq)


class MultiheadAttention(_Container):
    def __init__(self, embed_dim, num_heads):
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.head_dim = embed_dim // num_heads
        assert self.head_dim * num_heads == embed_dim, "embed_dim must be divisible by num_heads"
        self.scaling = self.head_dim ** -0.5
        self.k_proj = nn.Linear(embed_dim, embed_dim)
        self.v_proj = nn.Linear(embed_dim, embed_dim)
        self.q_proj = nn.Linear(embed_dim, embed_dim)
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        self.rot_emb = RotaryEmbedding(self.head_dim)


class TransformerLayer(_Container):
    def __init__(self, embed_dim, ffn_embed_dim, attention_heads):
        super().__init__()
        self.embed_dim, self.ffn_embed_dim, self.attention_heads = embed_dim, ffn_embed_dim, attention_heads
        self.self_attn = MultiheadAttention(embed_dim, attention_heads)
        self.self_attn_layer_norm = nn.LayerNorm(embed_dim)
        self.fc1 = nn.Linear(embed_dim, ffn_embed_dim)
        self.fc2 = nn.Linear(ffn_embed_dim, embed_dim)
        self.final_layer_norm = nn.LayerNorm(embed_dim)


class RobertaLMHead(_Container):
    def __init__(self, embed_dim, output_dim, weight):
        super().__init__()
        self.dense = nn.Linear(embed_dim, embed_dim)
        self.layer_norm = nn.LayerNorm(embed_dim)
        self.weight = weight  # tied to embed_tokens.weight
        self.bias = nn.Parameter(torch.zeros(output_dim))


class ContactPredictionHead(_Container):
    def __init__(self, in_features, prepend_bos, append_eos, bias=True, eos_idx=None):
        super().__init__()
        self.in_features, self.prepend_bos, self.append_eos = in_features, prepend_bos, append_eos
        if append_eos and eos_idx is None:
            raise ValueError("Using an alphabet with eos token, but no eos token was passed in.")
        self.eos_idx = eos_idx
        self.regression = nn.Linear(in_features, 1, bias)


def _varlen_kw(varlen, chunk_rows):
    """The keywords the scoring methods add to their ``esm_amd.scoring`` call: none for the default, so that the call is the one
    of before keyword for keyword; ``chunk_rows`` without ``varlen=True`` would be dropped silently, so it is refused."""
    if not varlen:
        if chunk_rows is not None:
            raise ValueError("chunk_rows sizes the packed row spaces of varlen=True; the padded path takes chunk")
        return {}
    return dict(varlen=True, chunk_rows=chunk_rows)


def _window_kw(window, wrap):
    """The keywords of a windowed call (``esm_amd.windows``): none without ``window``, so that the call is the one of before."""
    return {} if window is None else dict(window=window, wrap=wrap)


class ESM2(_EngineHost, nn.Module):
    _engine_class = _Engine
    _cpu_refusal = ("esm_amd.ESM2 runs only on an MI355X (ROCm) device: move the model and tokens to "
                    "'cuda' first; the engine has no CPU fallback")

    def __init__(
        self,
        num_layers: int = 33,
        embed_dim: int = 1280,
        attention_heads: int = 20,
        alphabet: Union[Alphabet, str] = "ESM-1b",
        token_dropout: bool = True,
    ):
        super().__init__()
        self.num_layers = num_layers
        self.embed_dim = embed_dim
        self.attention_heads = attention_heads
        if not isinstance(alphabet, Alphabet):
            alphabet = Alphabet.from_architecture(alphabet)
        self.alphabet = alphabet
        self.alphabet_size = len(alphabet)
        self.padding_idx = alphabet.padding_idx
        self.mask_idx = alphabet.mask_idx
        self.cls_idx = alphabet.cls_idx
        self.eos_idx = alphabet.eos_idx
        self.prepend_bos = alphabet.prepend_bos
        self.append_eos = alphabet.append_eos
        self.token_dropout = token_dropout
        self._engine = None
        self._init_submodules()

    def _init_submodules(self):
        self.embed_scale = 1
        self.embed_tokens = nn.Embedding(self.alphabet_size, self.embed_dim, padding_idx=self.padding_idx)
        self.layers = nn.ModuleList(
            [TransformerLayer(self.embed_dim, 4 * self.embed_dim, self.attention_heads) for _ in range(self.num_layers)]
        )
        self.contact_head = ContactPredictionHead(
            self.num_layers * self.attention_heads, self.prepend_bos, self.append_eos, eos_idx=self.eos_idx
        )
        self.emb_layer_norm_after = nn.LayerNorm(self.embed_dim)
        self.lm_head = RobertaLMHead(self.embed_dim, self.alphabet_size, self.embed_tokens.weight)

    # ------------------------------------------------------------------------------------------
    def _engine_key(self):
        return super()._engine_key() + (self._fold_setting(),)

    def _packs(self):  # False: no token-packed form (f16x3, ESM-1), ``forward_varlen`` and varlen scoring run padded
        return _weight_split() != 4

    def _engine_ready(self, device):
        """The engine for this call, parameters packed.  The fingerprint is taken once: it syncs the weights and, where it is
        still the one the fold decision was last taken under, vouches for the cached hazard (no second key per call)."""
        eng = self._engine
        fp = None if eng is None else eng.fingerprint_of(self)
        known = fp is not None and fp == eng.fingerprint and self.__dict__.get("_fold_fp") is eng.fingerprint
        new = self._get_engine(device, _EngineHost._engine_key(self) + (self._fold_setting(known),))
        new.sync_weights(self, fp if new is eng else None)
        object.__setattr__(self, "_fold_fp", new.fingerprint if _ln_fold() == 0 else None)
        new.set_edits(self.__dict__.get("_stream_edits"))  # (esm_amd/interventions.py; nothing to do unless they changed)
        return new

    def _fold_setting(self, gains_known=False):
        """esmk_config.ln_fold for this model: ESM_AMD_LN_FOLD when set; otherwise 0 (the library's default: on where it is
        supported) unless the LayerNorm gains in front of the q/k/v and fc1 projections make the fold's operand form lossy
        (``ln_fold_hazard``) — then -1.  ``_fold_hazard`` is cached under the (id, address, version) of the CURRENT gain
        tensors: the decision holds with or without an engine, on copies and after ``load_state_dict``, and the gains are read
        only when one changed (``.data`` writes, replaced sub-modules: ``refresh_engine()``).  ``gains_known``: see above."""
        env = _ln_fold()
        if env != 0:
            return env
        state = self.__dict__
        if gains_known:
            return -1 if state["_fold_hazard"] > _FOLD_HAZARD_MAX else 0
        slots = state.get("_fold_slots")
        if slots is None:  # the parameter dicts of the 2L LayerNorms, collected once: no walk of the module tree per call
            slots = [ln._parameters for layer in self.layers for ln in (layer.self_attn_layer_norm, layer.final_layer_norm)]
            object.__setattr__(self, "_fold_slots", slots)
        gains = [slot["weight"] for slot in slots]
        key = tuple((id(t), t.data_ptr(), t._version) for t in gains)
        if key != state.get("_fold_key"):
            h = ln_fold_hazard(torch.stack([t.detach() for t in gains])) if gains else 0.0
            object.__setattr__(self, "_fold_hazard", h)
            object.__setattr__(self, "_fold_key", key)
            object.__setattr__(self, "_fold_fp", None)
        return -1 if state["_fold_hazard"] > _FOLD_HAZARD_MAX else 0

    def refresh_engine(self):
        """Drop the engine state (call after replacing Parameter objects or sub-modules)."""
        super().refresh_engine()
        object.__setattr__(self, "_fold_slots", None)
        object.__setattr__(self, "_fold_key", None)

    def __getstate__(self):
        return dict(super().__getstate__(), _fold_slots=None, _fold_key=None)  # a copy reads its own gains

    def forward(self, tokens, repr_layers=[], need_head_weights=False, return_contacts=False, contacts_only=False):
        """Reference esm/model/esm2.py:77-144.  ``contacts_only=True`` (engine extension, used by ``predict_contacts``
        and the extraction driver) returns ``{"contacts", "representations"}`` only: no logits and no [B,L,H,T,T]
        "attentions" tensor is built — the contact map is accumulated layer by layer (csrc/contacts.hip)."""
        if contacts_only:
            return_contacts, need_head_weights = True, False
        if return_contacts and not contacts_only:
            need_head_weights = True
        assert tokens.ndim == 2
        w = self._check_devices(tokens)
        warn_if_grad_expected(self)
        from . import _native as N

        dev = tokens.device
        B, T = tokens.shape
        L, E, H, V = self.num_layers, self.embed_dim, self.attention_heads, self.alphabet_size
        repr_set = self._repr_set(repr_layers)
        with torch.cuda.device(dev):
            eng = self._engine_ready(dev)
            tok = tokens.to(torch.int64).contiguous()
            # predict_contacts: no logits, no attention tensor (contacts.hip accumulates the map layer by layer)
            flags = 0 if contacts_only else N.OUT_LOGITS
            f32 = dict(dtype=torch.float32, device=dev)
            lowp = _native_lowp(w.dtype, eng.operand_dtype)
            logits = None if contacts_only else torch.empty((B, T, V), **f32)
            if lowp and repr_set:
                flags |= N.OUT_REPR_LOWP
            reps = [torch.empty((B, T, E), dtype=w.dtype if lowp else torch.float32, device=dev) for _ in repr_set]
            attn = contacts = None
            if need_head_weights:
                flags |= N.OUT_ATTN
                if lowp and not return_contacts:  # the contact kernels read fp32 maps
                    flags |= N.OUT_ATTN_LOWP
                    attn = torch.empty((B, L, H, T, T), dtype=w.dtype, device=dev)
                else:
                    attn = torch.empty((B, L, H, T, T), **f32)
            if return_contacts:
                S = max(T - int(self.prepend_bos) - int(self.append_eos), 0)
                contacts = torch.empty((B, S, S), **f32)
                if S > 0:  # empty sequences: the reference returns an empty [B,0,0] map
                    flags |= N.OUT_CONTACTS
            eng.forward(tok, repr_set, reps, flags, logits, attn, contacts)
        cast = self._cast_to(w.dtype)
        if contacts_only:
            result = {"contacts": cast(contacts), "representations": {l: cast(r) for l, r in zip(repr_set, reps)}}
            check_finite(result)
            return result
        result = {"logits": cast(logits), "representations": {l: cast(r) for l, r in zip(repr_set, reps)}}
        if need_head_weights:
            result["attentions"] = cast(attn)
            if return_contacts:
                result["contacts"] = cast(contacts)
        check_finite(result)
        return result

    # ------------------------------------------------------------------------------------------
    # writing into the stream between layers (esm_amd/interventions.py): patching, steering, ablation
    def forward_edited(self, tokens, edits, repr_layers=[], need_head_weights=False, return_contacts=False, contacts_only=False):
        """``esm_amd.interventions.forward_edited``: ``forward``'s dict of one forward with the ``StreamEdit`` list ``edits``
        applied to the residual stream between layers; ``repr_layers`` shows the edited stream."""
        from . import interventions

        return interventions.forward_edited(self, tokens, edits, repr_layers=repr_layers, need_head_weights=need_head_weights,
                                            return_contacts=return_contacts, contacts_only=contacts_only)

    def stream_edits(self, edits):
        """``with model.stream_edits(edits):`` every padded-path engine call inside (``forward``, the scoring, sampling, design
        and Jacobian methods) runs with the token-set ``StreamEdit`` list ``edits`` applied."""
        from . import interventions

        return interventions.stream_edits(self, edits)

    def _refuse_under_edits(self, what=None, varlen=False, window=None):
        """Token-packed batches and windows are not built for edited runs: a ValueError that names the limit."""
        if self.__dict__.get("_stream_edits") is None:
            return
        what = what or ("varlen=True" if varlen else "window=" if window is not None else None)
        if what is not None:
            from .interventions import _NOT_BUILT

            raise ValueError(f"{what} inside model.stream_edits(...): {_NOT_BUILT}")

    # ------------------------------------------------------------------------------------------
    # token-packed batches: no compute on padding (include/esmk.h, esmk_forward_packed)
    supports_varlen = True  # ESM-2 (all sizes) and ESM-1b / ESM-1v; the MSA Transformer has no such path
    supports_contacts_only = True  # forward(contacts_only=True): contact maps without the attention tensor
    supports_varlen_contacts = True  # forward_varlen(contacts_only=True / return_contacts=True): packed contact maps
    supports_varlen_maps = True  # forward_varlen(need_head_weights=True): per-sequence attention maps of a packed batch

    def forward_varlen(self, tokens, repr_layers=[], lengths=None, min_saving=0.08, unpack=True, return_contacts=False,
                       contacts_only=False, need_head_weights=False):
        """Same results as ``forward(tokens, repr_layers)`` on the non-pad positions of a RIGHT-padded batch
        (what ``BatchConverter`` yields, reference esm/data.py:262-297), but the sequences are laid back to back
        in one row space and the engine does no work on padding.  Pad positions of the returned tensors are zero
        (the reference leaves the values the pad rows happened to compute there).

        tokens   [B,T] int64, CPU or device; from a CPU tensor the lengths are read without a device sync
        lengths  optional per-row token counts (incl. <cls>/<eos>); default: up to the last non-pad token
        min_saving  fall back to ``forward`` when packing saves less than this fraction of the rows
                    (None: always pack)
        unpack   False: return the packed tensors ([rows, .]) plus ``segments`` ([B,2] first row, length)
        return_contacts  also return "contacts" (predict_contacts' maps, accumulated per segment without the attention
                    tensor); ``contacts_only`` as in ``forward``: contacts and representations, no logits.  unpack=True:
                    [B, T-2, T-2] like ``forward(contacts_only=True)``, sequence b's map in the top-left [S_b, S_b] block
                    (S_b = its length - 2), zeros elsewhere; unpack=False: a list of per-sequence [S_b, S_b] views.

        need_head_weights  also return "attentions", bit-equal per sequence to ``forward(need_head_weights=True)``.
                    unpack=False: a list of per-sequence [L, H, len_b, len_b] views into ONE flat tensor (len_b includes
                    <cls>/<eos>; no [B, L, H, T, T] tensor is ever allocated — the form to use for mixed lengths);
                    unpack=True: the reference's [B, L, H, T, T] tensor, zero outside each sequence's corner, which is
                    ``forward(tokens, need_head_weights=True)["attentions"]`` as a whole tensor.  Together with
                    return_contacts the contacts stay the per-segment fused maps of ``contacts_only=True``.
                    When the call falls back to ``forward`` (min_saving, f16x3, ESM-1) and asks for maps AND contacts,
                    the model runs twice — once for the maps, once with ``contacts_only=True`` — so that the contacts
                    are the fused ones on both routes and the maps can stay in the model dtype; the fall-back is taken
                    where packing saves little, i.e. the second run costs one contacts-only forward of the same batch.

        The scoring methods follow the same rule (``esm_amd.scoring``): with ``varlen=True`` on an ESM-1 model or in the
        f16x3 mode, which have no token-packed form, the padded path runs."""
        assert tokens.ndim == 2
        self._refuse_under_edits("forward_varlen")
        from . import _native as N
        from .packing import dense_from_views, pack_plan, ragged_views

        w = self.embed_tokens.weight
        if not w.is_cuda:
            raise RuntimeError("esm_amd.ESM2 runs only on an MI355X (ROCm) device; the engine has no CPU fallback")
        warn_if_grad_expected(self)
        dev = w.device
        B, T = tokens.shape
        L, E, H, V = self.num_layers, self.embed_dim, self.attention_heads, self.alphabet_size
        if contacts_only:
            return_contacts = True
        plan = pack_plan(tokens, self.padding_idx, lengths)
        if unpack and ((min_saving is not None and plan.rows > (1.0 - min_saving) * B * T) or not self._packs()):
            # (f16x3 and the ESM-1 models have no token-packed form)
            if need_head_weights:
                full = self.forward(tokens.to(dev), repr_layers=repr_layers, need_head_weights=True)
                if return_contacts:
                    ct = self.forward(tokens.to(dev), repr_layers=repr_layers if contacts_only else [], contacts_only=True)
                    if contacts_only:
                        return dict(ct, attentions=full["attentions"])
                    full = dict(full, contacts=ct["contacts"])
                return full
            if return_contacts:
                out = self.forward(tokens.to(dev), repr_layers=repr_layers, contacts_only=True)
                if not contacts_only:
                    out = dict(self.forward(tokens.to(dev), repr_layers=repr_layers), contacts=out["contacts"])
                return out
            return self.forward(tokens.to(dev), repr_layers=repr_layers)
        repr_set = self._repr_set(repr_layers)
        ends = int(self.prepend_bos) + int(self.append_eos)
        with torch.cuda.device(dev):
            eng = self._engine_ready(dev)
            idx, keep = plan.index(dev)
            flat = plan.pack(tokens, self.padding_idx, idx)
            f32 = dict(dtype=torch.float32, device=dev)
            lowp = _native_lowp(w.dtype, eng.operand_dtype)
            flags = (0 if contacts_only else N.OUT_LOGITS) | (N.OUT_REPR_LOWP if lowp and repr_set else 0)
            logits = None if contacts_only else torch.empty((plan.rows, V), **f32)
            reps = [torch.empty((plan.rows, E), dtype=w.dtype if lowp else torch.float32, device=dev) for _ in repr_set]
            flat_ct = flat_at = None
            if return_contacts:
                # ragged fp32 maps: sequence b's [S_b, S_b] block at sum_{b'<b} S_b'^2 (include/esmk.h)
                flags |= N.OUT_CONTACTS
                sides = [max(n - ends, 0) for n in plan.lengths.tolist()]
                flat_ct = torch.empty((max(1, sum(s * s for s in sides)),), **f32)
            if need_head_weights:
                # ragged maps: sequence b's [L, H, len_b, len_b] block at L H sum_{b'<b} len_b'^2 (include/esmk.h), in the
                # model dtype directly when the engine's operand dtype is that dtype
                flags |= N.OUT_ATTN | (N.OUT_ATTN_LOWP if lowp else 0)
                lens = plan.lengths.tolist()
                flat_at = torch.empty((L * H * sum(n * n for n in lens),), dtype=w.dtype if lowp else torch.float32, device=dev)
            eng.forward_packed(flat, plan.segments, plan.rows, repr_set, reps, flags, logits, flat_at, flat_ct)
        cast = self._cast_to(w.dtype)
        un = (lambda t: plan.unpack(t, idx, keep)) if unpack else (lambda t: t)
        out = {"representations": {l: cast(un(r)) for l, r in zip(repr_set, reps)}}
        if not unpack:
            out["segments"] = plan.segments  # int32 [B,2], CPU, contiguous
        if logits is not None:
            out["logits"] = cast(un(logits))
        if return_contacts:
            flat_ct = cast(flat_ct)
            views = ragged_views(flat_ct, sides)
            out["contacts"] = dense_from_views(views, (), max(T - ends, 0), flat_ct) if unpack else views
        if need_head_weights:
            flat_at = cast(flat_at)
            views = ragged_views(flat_at, lens, (L, H))
            out["attentions"] = dense_from_views(views, (L, H), T, flat_at) if unpack else views
        return out

    # ------------------------------------------------------------------------------------------
    # zero-shot variant scoring (esm_amd/scoring.py; reference examples/variant-prediction/predict.py)
    supports_scoring = True  # esmk_forward_rows: ESM-2, ESM-1b / ESM-1v, ESM-1; not the MSA Transformer

    # varlen=True: the masked copies run token-packed (esmk_forward_packed_rows) — the form for sequences of different lengths;
    # the same bits.  The default call is the one of before, keyword for keyword.
    # window= (an int, or "max" on ESM-1b / ESM-1v): sequences longer than the window are scored inside model-sized windows
    # (esm_amd/windows.py); without it the call is the one of before.
    def masked_marginals(self, tokens, positions=None, chunk=None, varlen=False, chunk_rows=None, window=None, wrap=True):
        """``esm_amd.scoring.masked_marginals``: [B, T, V] fp32 log-probabilities, row (b, i) from the forward with token
        (b, i) alone masked."""
        self._refuse_under_edits(varlen=varlen, window=window)
        from . import scoring

        return scoring.masked_marginals(self, tokens, positions=positions, chunk=chunk, **_varlen_kw(varlen, chunk_rows),
                                        **_window_kw(window, wrap))

    def wt_marginals(self, tokens, varlen=False, chunk_rows=None, window=None, wrap=True):
        """``esm_amd.scoring.wt_marginals``: [B, T, V] fp32 log-probabilities of the unmasked forward, non-pad rows."""
        self._refuse_under_edits(varlen=varlen, window=window)
        from . import scoring

        return scoring.wt_marginals(self, tokens, **_varlen_kw(varlen, chunk_rows), **_window_kw(window, wrap))

    def pseudo_log_likelihood(self, tokens, positions=None, chunk=None, varlen=False, chunk_rows=None, window=None, wrap=True):
        """``esm_amd.scoring.pseudo_log_likelihood``: [B] fp64, sum of the masked-marginal log-probability of the true token."""
        self._refuse_under_edits(varlen=varlen, window=window)
        from . import scoring

        return scoring.pseudo_log_likelihood(self, tokens, positions=positions, chunk=chunk, **_varlen_kw(varlen, chunk_rows),
                                             **_window_kw(window, wrap))

    def masked_joint(self, tokens, position_sets, src=None, chunk=None, return_logits=False, varlen=False, chunk_rows=None,
                     window=None, wrap=True):
        """``esm_amd.scoring.masked_joint``: one forward per position set with ALL its positions masked; (offsets, pos,
        logprobs [n_rows, V]) of the masked rows."""
        self._refuse_under_edits(varlen=varlen, window=window)
        from . import scoring

        return scoring.masked_joint(self, tokens, position_sets, src=src, chunk=chunk, return_logits=return_logits,
                                    **_varlen_kw(varlen, chunk_rows), **_window_kw(window, wrap))

    def score_variants(self, alphabet, sequence, variants, strategy="masked-marginals", offset_idx=0, sep=":", chunk=None,
                       window=None, wrap=True):
        """``esm_amd.scoring.score_variants``: floats, one per variant of one or more substitutions ('A42G:K50R')."""
        self._refuse_under_edits(window=window)
        from . import scoring

        return scoring.score_variants(self, alphabet, sequence, variants, strategy=strategy, offset_idx=offset_idx, sep=sep,
                                      chunk=chunk, **_window_kw(window, wrap))

    def forward_windows(self, tokens, repr_layers=[], window=None, stride=None, wrap=True, stitch="owner", return_contacts=False,
                        chunk=None):
        """``esm_amd.windows.forward_windows``: ``forward``'s dict in source coordinates for sequences longer than the model's
        window — overlapping windows through ``forward``, logits / representations / contact maps stitched on the device."""
        self._refuse_under_edits("forward_windows")
        from . import windows

        return windows.forward_windows(self, tokens, repr_layers=repr_layers, window=window, stride=stride, wrap=wrap,
                                       stitch=stitch, return_contacts=return_contacts, chunk=chunk)

    # drawing sequences (esm_amd/sampling.py): Gibbs sweeps and mask in-painting, every step on the device
    def gibbs_sample(self, tokens, sweeps, per_step=1, positions=None, temperature=1.0, allowed=None, force_new=False, seed=0,
                     chain_ids=None, return_trajectory=False, top_k=0, top_p=1.0, order="random"):
        """``esm_amd.sampling.gibbs_sample``: the final tokens [B, T] of ``sweeps`` Gibbs sweeps over every chain's positions."""
        from . import sampling

        return sampling.gibbs_sample(self, tokens, sweeps, per_step=per_step, positions=positions, temperature=temperature,
                                     allowed=allowed, force_new=force_new, seed=seed, chain_ids=chain_ids,
                                     return_trajectory=return_trajectory, top_k=top_k, top_p=top_p, order=order)

    def inpaint(self, tokens, per_step=1, temperature=1.0, allowed=None, seed=0, chain_ids=None, return_trajectory=False,
                top_k=0, top_p=1.0, order="random"):
        """``esm_amd.sampling.inpaint``: ``tokens`` [B, T] with every <mask> position filled by a draw from the model, in a
        random order or the most confident positions first (``order``), behind an optional top-k / nucleus filter."""
        from . import sampling

        return sampling.inpaint(self, tokens, per_step=per_step, temperature=temperature, allowed=allowed, seed=seed,
                                chain_ids=chain_ids, return_trajectory=return_trajectory, top_k=top_k, top_p=top_p, order=order)

    # design toward a target contact map (esm_amd/design.py): Metropolis-Hastings chains, every step on the device
    def design(self, tokens, target, steps, positions=None, w_contact=1.0, w_lm=1.0, contact_loss="pos", min_sep=6,
               temperature=1.0, proposal="uniform", proposal_temperature=1.0, allowed=None, force_new=None, seed=0, chain_ids=None,
               return_trajectory=False, max_bytes=8 << 30, w_ngram=0.0, ngram=None, replicas=None, swap_every=1):
        """``esm_amd.design.design``: (final tokens [B, T], final energies fp64 [B]) of ``steps`` Metropolis-Hastings steps per
        chain on E = w_contact * E_contact(predicted map, target) + w_lm * E_lm (+ w_ngram * E_ngram); with ``replicas`` the chains
        are temperature ladders that exchange their rungs, and the rungs are returned too."""
        from . import design as D

        return D.design(self, tokens, target, steps, positions=positions, w_contact=w_contact, w_lm=w_lm, contact_loss=contact_loss,
                        min_sep=min_sep, temperature=temperature, proposal=proposal, proposal_temperature=proposal_temperature,
                        allowed=allowed, force_new=force_new, seed=seed, chain_ids=chain_ids,
                        return_trajectory=return_trajectory, max_bytes=max_bytes, w_ngram=w_ngram, ngram=ngram, replicas=replicas,
                        swap_every=swap_every)

    def design_energy(self, tokens, target, w_contact=1.0, w_lm=1.0, contact_loss="pos", min_sep=6, max_bytes=8 << 30, w_ngram=0.0,
                      ngram=None):
        """``esm_amd.design.design_energy``: the energy ``design`` minimises and its terms, fp64 [B] each."""
        from . import design as D

        return D.design_energy(self, tokens, target, w_contact=w_contact, w_lm=w_lm, contact_loss=contact_loss, min_sep=min_sep,
                               max_bytes=max_bytes, w_ngram=w_ngram, ngram=ngram)

    # the categorical Jacobian (esm_amd/jacobian.py): substituted copies in batches that fill the GPU, J kept on the device
    def categorical_jacobian(self, tokens, allowed=None, chunk=None, center=False, max_bytes=8 << 30):
        """``esm_amd.jacobian.categorical_jacobian``: fp32 [L, nA, L, nA], the change of every candidate's logit at every
        residue under every single substitution of ONE sequence."""
        from . import jacobian

        return jacobian.categorical_jacobian(self, tokens, allowed=allowed, chunk=chunk, center=center, max_bytes=max_bytes)

    def jacobian_contacts(self, tokens, allowed=None, chunk=None, return_jacobian=False):
        """``esm_amd.jacobian.jacobian_contacts``: fp32 [L, L], the contact map of the centred categorical Jacobian."""
        from . import jacobian

        return jacobian.jacobian_contacts(self, tokens, allowed=allowed, chunk=chunk, return_jacobian=return_jacobian)

    # linear pairwise heads on the attention maps (esm_amd/pair_head.py): no attention tensor
    def pair_logits(self, tokens, head, max_bytes=8 << 30, varlen=False, window=None):
        """``esm_amd.pair_head.pair_logits``: name -> fp32 [B, S, S, n] logits of the ``PairHead`` ``head`` (lm-design's distogram
        and orientation head, or any linear head on the L*H attention maps)."""
        from . import pair_head

        return pair_head.pair_logits(self, tokens, head, max_bytes=max_bytes, varlen=varlen, window=window)

    # sparse-autoencoder features of the stream (esm_amd/sae.py): device top-k per residue, maxima per protein
    def sae_features(self, tokens, sae, layer, top_k=None, positions="residues", varlen=False, protein_max=False,
                     return_dense=False, max_bytes=2 << 30):
        """``esm_amd.sae.sae_features``: rows, indices, values and n_active of the ``SparseAutoencoder`` ``sae`` on representation
        ``layer`` of every scored row; with ``protein_max`` the per-sequence maximum of every feature and where it was."""
        from . import sae as S

        return S.sae_features(self, tokens, sae, layer, top_k=top_k, positions=positions, varlen=varlen, protein_max=protein_max,
                              return_dense=return_dense, max_bytes=max_bytes)

    # embedding-based alignment (esm_amd/align.py): similarity GEMM and affine-gap DP on the device
    def align(self, tokens_a, tokens_b, layer=None, varlen=False, **kw):
        """``esm_amd.align.align``: every sequence of ``tokens_a`` aligned against every sequence of ``tokens_b`` (or the listed
        ``pairs``) on representation ``layer``: scores, end cells and, with ``paths``, the alignments' columns."""
        from . import align as A

        return A.align(self, tokens_a, tokens_b, layer=layer, varlen=varlen, **kw)

    # protein search on pooled embeddings (esm_amd/search.py): early layer exit, per-protein mean, streaming cosine top-k
    def embed_layer(self, tokens, layer=None, varlen=False, window=None):
        """``esm_amd.search.embed_layer``: fp32 [B, T, E], representation ``layer`` (None: the last) as ``forward`` (with
        ``varlen``: ``forward_varlen``) returns it, bit for bit — from a forward that runs only the layers below it."""
        from . import search

        return search.embed_layer(self, tokens, layer=layer, varlen=varlen, window=window)

    def pool(self, tokens, layer=None, varlen=False, window=None):
        """``esm_amd.search.pool``: fp32 [B, E], the mean of every sequence's residue rows of representation ``layer``."""
        from . import search

        return search.pool(self, tokens, layer=layer, varlen=varlen, window=window)

    def search(self, index, tokens, top_k, varlen=False, **kw):
        """``esm_amd.search.search``: ``pool`` on ``tokens`` at the index's layer, then ``index.search``."""
        from . import search

        return search.search(self, index, tokens, top_k, varlen=varlen, **kw)

    # search hits to a query-anchored MSA (esm_amd/msa_build.py): projection, coverage and redundancy filters on the device
    def build_msas(self, alphabet, queries, index, **kw):
        """``esm_amd.msa_build.build_msas``: one ``BuiltMSA`` per query (label, sequence) from the aligned hits of ``index``."""
        from . import msa_build

        return msa_build.build_msas(self, alphabet, queries, index, **kw)

    def build_msa(self, alphabet, query, index, **kw):
        """``esm_amd.msa_build.build_msa``: ``build_msas`` for one query."""
        from . import msa_build

        return msa_build.build_msa(self, alphabet, query, index, **kw)

    def predict_contacts(self, tokens):
        """Reference esm2.py:146-147 returns ``self(tokens, return_contacts=True)["contacts"]``, which first builds
        the [B,L,H,T,T] attention tensor (2.8 GB per 1024-token sequence at 650M).  Only the map leaves this call, so
        the engine accumulates it layer by layer instead (csrc/contacts.hip) — same formula, no attention tensor."""
        return self(tokens, return_contacts=True, contacts_only=True)["contacts"]
