"""The Python owner of the model-level C ABI calls (include/esmk.h): creating and destroying engine handles, packing the
parameter image, sizing the workspace, every model forward entry, the profiler; the engine's environment switches.  ``Engine``
holds one handle with its image and workspace, ``Esm2Engine`` (ESM-2, ESM-1b / 1v, ESM-1) and ``MsaEngine`` add configuration
and forward entries, ``_EngineHost`` is what the ``nn.Module`` classes mix in.  ``esm_amd.ops`` calls the ``esmk_op_*`` entries.
"""
import ctypes
import os
import warnings

import torch


def _native_lowp(param_dtype, operand_dtype):
    """``.half()`` / ``.bfloat16()`` models return fp16 / bf16 tensors (the reference runs the whole module in that
    dtype; ESMFold's front end does so, esmfold/v1/esmfold.py:61-67).  When the model dtype is the engine's operand
    dtype the engine writes representations / attention maps in it directly (ESMK_OUT_REPR_LOWP / _ATTN_LOWP);
    ``ESM_AMD_NATIVE_LOWP=0`` falls back to fp32 outputs + a cast (same bits, one more pass; used by the tests)."""
    if os.environ.get("ESM_AMD_NATIVE_LOWP", "1") == "0":
        return False
    return param_dtype in (torch.float16, torch.bfloat16) and param_dtype == operand_dtype


def _weight_split():
    """``ESM_AMD_OPERAND=f16x2``: precision mode with split weights (W = W_hi + W_lo, both fp16, two MFMA passes per
    layer GEMM): removes the weight rounding — two thirds of the fp16-operand error of a deep stack — at 2x the GEMM
    time.  ESM-2, ESM-1b and (since round 4) the MSA Transformer engine.
    ``ESM_AMD_OPERAND=f16x2a`` (round 6): the same for the ATTENTION projections only (q, k, v, out: a third of the GEMM
    work) — representations and logits inside 1e-3 in both norms at ~1.3x the plain step instead of 1.6x.
    ``ESM_AMD_OPERAND=f16x2v``: the VALUE path only (v, out: a sixth of the GEMM work, ~1.2x) — most of f16x2a's gain on
    representations and logits; q / k rounding matters for the attention maps / contact logits only.
    ``ESM_AMD_OPERAND=f16x3``: weights AND GEMM inputs split (every layer GEMM a plain launch over K' = 3 K: A_hi W_hi +
    A_hi W_lo + A_lo W_hi) — the mode that holds 1e-3 on EVERY output, contact logits included, at ~2.4x the step;
    head_dim-64 models, padded batches (``forward_varlen`` falls back to ``forward``).
    Returns esmk_config.weight_split: 0 off, 1 f16x2, 2 f16x2a, 3 f16x2v, 4 f16x3."""
    env = os.environ.get("ESM_AMD_OPERAND", "").lower()
    return {"f16x2": 1, "fp16x2": 1, "f16x2a": 2, "fp16x2a": 2, "f16x2v": 3, "fp16x2v": 3, "f16x3": 4, "fp16x3": 4}.get(env, 0)


def _ln_fold():
    """``ESM_AMD_LN_FOLD=1|0``: LayerNorm fold of the engine (esmk_config.ln_fold) on / off; unset = the
    library's default.  ESM-2 / ESM-1b engines with plain fp16 / bf16 operands and head_dim <= 64."""
    v = os.environ.get("ESM_AMD_LN_FOLD", "")
    return 0 if v == "" else (1 if v not in ("0", "off", "false") else -1)


# The LayerNorm fold and small LayerNorm gains (round 6, tools/outlier_stress_study.py, profiles/r6_outlier_stress_study.log).
# The fold's consumers run on gain-folded, row-centred weight images: column j of an image holds gamma_j w_ij - c_i with
# c_i = mean_k(gamma_k w_ik), and its operand rows are the un-normalised fp16(x - mean).  A channel whose gain is far below
# the others (|gamma_j| << median / sqrt(E)) holds almost nothing but -c_i; if the checkpoint uses that small gain to silence
# a large activation (the "massive activation" channels of trained transformers), the fp16 rounding of x_j and of c_i is
# multiplied by that large x_j: the fold's error grows with x_j / (E s) (s: the spread of the ordinary channels) while the
# plain mode — which rounds the normalised value gamma_j (x_j - mean) rstd — does not see the channel at all.  (Same-signed
# outliers add a second term: they shift the row mean, the LayerNorm bias takes the shift back — exactly, as fp32 W . beta, in
# the fold, against a counterpart that went through the rounded image)  Measured on
# the stress weights of esm_amd.synth.add_outlier_channels (650M dims, four channels): gain ratio 133 (outliers 200 x the
# stream) -> fold / plain floor 1.1; 1333 -> 3.3 ... 4.2; 13333 -> 34.  The hazard of one LayerNorm, from its gains alone:
#     h = sum over channels with |gamma_j| < median / 8 of (median / |gamma_j|) / E
# and of a model: the mean over its folded LayerNorms (0.35 / 3.5 / 35 on those three sets; the stream of the first layers
# is small, so their ratios are the largest).  When ESM_AMD_LN_FOLD is unset, a model whose h exceeds 0.5 runs WITHOUT the
# fold (the standalone LayerNorm passes:
# - 1.1 % at B = 64, - 6 % at B = 4); ESM_AMD_LN_FOLD=1 forces it on, =0 off.  Callers of the C ABI choose esmk_config.ln_fold
# themselves.
_FOLD_HAZARD_MAX = 0.5


def ln_fold_hazard(gains):
    """``gains``: [n_layernorms, E] LayerNorm weights whose outputs feed folded GEMMs.  Returns their mean h (see above)."""
    g = gains.detach().float().abs()
    med = g.median(dim=-1, keepdim=True).values
    small = g < med / 8
    h = torch.where(small, med / g.clamp_min(1e-30), torch.zeros_like(g)).sum(-1) / g.shape[-1]
    return float(h.mean().item()) if h.numel() else 0.0


# Small and medium batches as TWO half-batches on two HIP streams (round 6).  Below ~56 k rows the persistent GEMMs end in
# partly filled rounds of tiles over the 256 CUs (B = 8 x 1024 tokens: fc2 has 320 half-height tiles = 1.25 rounds);
# workgroups without a tile exit at once, so the kernels of a second, independent half-batch take the idle CUs.  Measured on
# one box (650M dims, profiles/r6_dual_stream_probe.log), rows -> gain: 4096 + 3.9 %, 6144 - 1.2 %, 8192 + 9.4 %, 12288
# + 2.4 %, 16384 + 7.9 %, 24576 + 2.4 %, 32768 + 2.1 %, 40960 + 6.9 %, 49152 + 2.2 %, 65536 + 0.6 % (whole rounds already);
# the same per row count for other (B, T) shapes.  Sequences are independent and every kernel of the forward is batch-invariant
# bit for bit, so the results are the bits of the one-stream forward (the fused contact map of predict_contacts, whose head
# grouping depends on the batch size, stays on one stream).  ``ESM_AMD_DUAL_STREAM=0`` switches it off,
# ``=lo:hi[,lo:hi...]`` sets the row windows (tokens per forward call).
def _dual_stream_window():
    v = os.environ.get("ESM_AMD_DUAL_STREAM", "")
    if v in ("0", "off", "false"):
        return None
    if ":" in v:
        return [tuple(int(x) for x in w.split(":", 1)) for w in v.split(",")]
    return [(3584, 5120), (7168, 57344)]


def _dual_stream_wanted(rows):
    win = _dual_stream_window()
    return win is not None and any(lo <= rows <= hi for lo, hi in win)


def _operand_dtype_for(param_dtype):
    env = os.environ.get("ESM_AMD_OPERAND", "").lower()
    if env in ("bf16", "bfloat16"):
        return torch.bfloat16
    if env in ("f16", "fp16", "float16", "half", "f16x2", "fp16x2", "f16x2a", "fp16x2a", "f16x2v", "fp16x2v", "f16x3", "fp16x3"):
        return torch.float16
    # fp16 operands keep the 33-layer stack within 1e-3 of the fp32 reference (bf16: ~5e-3)
    return torch.bfloat16 if param_dtype == torch.bfloat16 else torch.float16


def live_tensors(engine, model, skip):
    """[(state-dict key, tensor)] of the model's CURRENT parameters and buffers.  The (owner dict, name) slots are
    collected once per engine; reading them back costs a dict lookup per tensor, so a replaced Parameter object is
    picked up without walking the module tree on every forward."""
    if engine._named is None:
        slots = []
        for prefix, mod in model.named_modules():
            for store in (mod._parameters, mod._buffers):
                for name, t in store.items():
                    key = f"{prefix}.{name}" if prefix else name
                    if t is not None and not skip(key) and name not in getattr(mod, "_non_persistent_buffers_set", ()):
                        slots.append((key, store, name))
        engine._named = slots
    return [(key, store[name]) for key, store, name in engine._named]


def check_finite(result):
    """``ESM_AMD_CHECK_FINITE=1`` (debug aid, synchronises): raise if an output holds inf / NaN.  The engine rounds
    GEMM operands to fp16 (range 65504) also for fp32 models; this has been validated on seeded synthetic weights
    only (no released checkpoint is available offline), so a first run on real weights can be checked this way.
    Pad positions are included: the reference leaves finite garbage there as well."""
    if os.environ.get("ESM_AMD_CHECK_FINITE", "0") != "1":
        return
    def walk(prefix, v):
        if isinstance(v, dict):
            for k, t in v.items():
                walk(f"{prefix}[{k!r}]", t)
        elif torch.is_tensor(v) and v.is_floating_point() and not bool(torch.isfinite(v).all()):
            raise FloatingPointError(f"esm_amd: {prefix} contains inf / NaN (fp16 operand overflow? try ESM_AMD_OPERAND=bf16)")
    walk("out", result)


def warn_if_grad_expected(model):
    """The engine is forward-only: outputs carry no grad_fn.  The reference's own tests call forward without
    ``no_grad`` (tests/test_load_all.py:39-47), so this warns — once per model — instead of raising."""
    if torch.is_grad_enabled() and not getattr(model, "_warned_no_grad", False):
        if any(p.requires_grad for p in model.parameters()):
            warnings.warn(
                "esm_amd: the MI355X engine is forward-only — the tensors returned by forward() have no grad_fn, so "
                "backward() through this model yields no parameter gradients. Wrap inference in torch.no_grad() or "
                "call model.requires_grad_(False) to silence this warning.", RuntimeWarning, stacklevel=3)
            # only once the warning was actually emitted: a later model.requires_grad_(True) must still be told
            object.__setattr__(model, "_warned_no_grad", True)


class Engine:
    """One native model handle + packed parameter image + workspace for one (device, operand dtype).  A subclass builds
    its configuration struct, says which tensors are packed in which order and form, and adds its forward entries."""

    def __init__(self, device, operand_dtype, weight_split):
        from . import _native as N

        self.N = N
        self.device = device
        self.operand_dtype = operand_dtype
        self.weight_split = int(weight_split)  # esmk_config.weight_split: 0 off, 1 f16x2, 2 f16x2a, 3 f16x2v, 4 f16x3
        self.key = (operand_dtype, self.weight_split)  # what _EngineHost._get_engine compares to keep or replace the engine
        self.handle = ctypes.c_void_p()
        self.packed = None
        self.fingerprint = None
        self.workspace = None
        self.profiling = False
        self._named = None

    def _alloc_packed(self):
        # zero-initialised: padded head slots / K columns of the packed image must stay zero
        self.packed = torch.zeros(self._query(self.N.lib.esmk_packed_bytes), dtype=torch.uint8, device=self.device)

    def close(self):
        if self.handle:
            self.N.lib.esmk_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _query(self, fn, *args, offset=False):
        """The size a ``*_bytes`` entry reports for this handle; ``offset``: (size, ``logits_offset``) of a rows entry."""
        need, off = ctypes.c_size_t(), ctypes.c_size_t()
        if offset:
            self.N.check(fn(self.handle, *args, ctypes.byref(need), ctypes.byref(off)))
            return need.value, off.value
        self.N.check(fn(self.handle, *args, ctypes.byref(need)))
        return need.value

    def _grown(self, name, n):
        """Workspace ``name`` with at least ``n`` bytes; the old tensor is released before a larger one is made."""
        if getattr(self, name) is None or getattr(self, name).numel() < n:
            setattr(self, name, None)
            setattr(self, name, torch.empty(n, dtype=torch.uint8, device=self.device))
        return getattr(self, name)

    def workspace_for_bytes(self, n):
        return self._grown("workspace", n)

    # what a subclass may change about the packing: which state-dict keys are left out, the order, the form of a tensor
    @staticmethod
    def _skip(key):
        return key == "lm_head.weight"

    def _pack_order(self, named):
        return named

    def _pack_form(self, key, t):
        return t

    def fingerprint_of(self, model):
        """(object id, storage address, version counter, dtype) of every live tensor of the model that is packed."""
        return tuple((id(t), t.data_ptr(), t._version, t.dtype) for _, t in live_tensors(self, model, self._skip))

    def sync_weights(self, model, fp=None):
        """Re-pack the parameter image when the parameters changed: ``.cuda()`` / ``.half()`` /
        ``load_state_dict`` (also with ``assign=True``), ``module.weight = nn.Parameter(...)``, swapped tensors and
        tracked in-place edits are all seen (live tensors are looked up on every call; fingerprint = object id,
        storage address, version counter, dtype).  NOT seen: writes through ``param.data`` (they bypass the version
        counter) and replaced sub-modules — call ``model.refresh_engine()`` after those.  ``fp``: a just-taken fingerprint."""
        N = self.N
        if fp is None:
            fp = self.fingerprint_of(model)
        if fp == self.fingerprint:
            return
        stream = N.cur_stream()
        for key, t in self._pack_order(live_tensors(self, model, self._skip)):
            t = self._pack_form(key, t.detach())
            if not t.is_contiguous():
                t = t.contiguous()
            shape = (ctypes.c_int64 * t.dim())(*t.shape)
            N.check(N.lib.esmk_pack_weight(self.handle, N.ptr(self.packed), self.packed.numel(),
                                           key.encode(), N.ptr(t), N.dtype_code(t.dtype), shape, t.dim(),
                                           stream))
        self.fingerprint = fp

    @staticmethod
    def _repr_args(repr_set, reps):
        """(layers, n, outs): the representation arguments of a forward entry (arrays of at least one element)."""
        n = len(repr_set)
        return ((ctypes.c_int32 * max(1, n))(*repr_set), n, (ctypes.c_void_p * max(1, n))(*[r.data_ptr() for r in reps]))

    def _rows(self, query, entry, lead, tok, sel_rows, V, return_logits):
        """The row-selected forward ``entry`` (sized by ``query``) on the tokens ``tok``, ``lead`` being the arguments
        between the tokens and the row list: fp32 ``[n, V]`` log-probabilities of ``sel_rows`` and, with ``return_logits``,
        the selected fp32 logits, cloned out of the workspace."""
        N = self.N
        n = sel_rows.numel()
        need, off = self._query(query, *lead, n, offset=True)
        ws = self.workspace_for_bytes(need)
        out = torch.empty((n, V), dtype=torch.float32, device=self.device)
        N.check(entry(self.handle, N.ptr(self.packed), N.ptr(tok), *lead, N.ptr(sel_rows), n, N.ptr(out), N.ptr(ws), ws.numel(),
                      N.cur_stream()))
        if return_logits:
            return out, ws[off: off + n * V * 4].view(torch.float32).view(n, V).clone()
        return out

    def profile_begin(self):
        self.N.check(self.N.lib.esmk_profile_begin(self.handle))
        self.profiling = True  # per-class events live on ONE stream: no dual-stream forward while armed

    def profile_end(self):
        N = self.N
        buf = (N.EsmkProfileEntry * 32)()
        n = ctypes.c_int()
        N.check(N.lib.esmk_profile_end(self.handle, buf, 32, ctypes.byref(n)))
        self.profiling = False
        return [dict(name=buf[i].name.decode(), launches=buf[i].launches, ms=buf[i].ms, flops=buf[i].flops,
                     bytes=buf[i].bytes) for i in range(n.value)]

    def ln_fold_active(self):
        """True / False: the handle runs with / without the LayerNorm fold; None: an engine that has no fold (MSA)."""
        state = self.N.lib.esmk_ln_fold_enabled(self.handle)
        return None if state < 0 else state == 1


class Esm2Engine(Engine):
    """The engine of ``ESM2`` and ``ProteinBertModel`` (ESM-1b / ESM-1v, ESM-1): ``esmk_create`` and the ``esmk_forward*``
    entries."""

    def __init__(self, model, device, operand_dtype, weight_split=0, ln_fold=None):
        # ESM-1b / ESM-1v and ESM-1 (esm_amd.esm1.ProteinBertModel) state these; ESM-2 leaves them at zero
        extra = model._engine_config()
        if extra.get("esm1") and int(weight_split):
            raise RuntimeError(
                f"ESM_AMD_OPERAND={os.environ.get('ESM_AMD_OPERAND', '')}: the split-operand precision modes (f16x2*, f16x3) are not "
                "available for ESM-1 models (bias_kv attention); use f16 or bf16")
        super().__init__(device, operand_dtype, weight_split)
        N = self.N
        # ESM_AMD_LN_FOLD (or the gain check of ESM2._fold_setting) at creation: a changed setting makes a new engine
        self.ln_fold = _ln_fold() if ln_fold is None else int(ln_fold)
        self.key += (self.ln_fold,)
        self.no_rope = int(extra.get("no_rope", 0))
        if extra.get("esm1"):  # esmk_config.no_rope = ESMK_ESM1 (| ESMK_ESM1_FINAL_BIAS)
            self.no_rope = N.ESM1 | (N.ESM1_FINAL_BIAS if extra.get("final_bias") else 0)
        cfg = N.EsmkConfig(
            model.num_layers, model.embed_dim, model.attention_heads, int(getattr(model, "ffn_embed_dim", 4 * model.embed_dim)),
            model.alphabet_size, model.padding_idx, model.mask_idx, model.cls_idx, model.eos_idx,
            int(bool(model.token_dropout)), int(bool(model.prepend_bos)), int(bool(model.append_eos)),
            N.dtype_code(operand_dtype), self.no_rope, int(extra.get("num_positions", 0)), int(extra.get("ln_before", 0)),
            self.weight_split,
            # the fold is asked for only where the library supports it (plain operands, head_dim <= 64); elsewhere "default"
            self.ln_fold if (not self.weight_split and model.embed_dim // model.attention_heads <= 64) or self.ln_fold < 0 else 0,
        )
        with torch.cuda.device(device):
            N.check(N.lib.esmk_create(ctypes.byref(cfg), ctypes.byref(self.handle)))
            if not self.no_rope:
                d = model.embed_dim // model.attention_heads
                inv = (1.0 / (10000 ** (torch.arange(0, d, 2).float() / d))).tolist()
                arr = (ctypes.c_float * len(inv))(*inv)
                N.check(N.lib.esmk_set_rope_inv_freq(self.handle, arr, len(inv)))
            self._alloc_packed()
        self.workspace2 = None   # second half-batch of the dual-stream forward
        self.stream2 = None
        self.max_T = 0           # longest row a finished forward call has seen (its RoPE table exists and is ordered before us)
        self.dual_calls = 0
        self.edits = None        # esm_amd.interventions.DeviceEdits the handle holds (esmk_set_stream_edits), or None

    def set_edits(self, edits):
        """The handle's stream edits become ``edits`` (``esm_amd.interventions.DeviceEdits`` or None); no call when they are."""
        if edits is self.edits:
            return
        N = self.N
        if self.handle:
            N.check(N.lib.esmk_set_stream_edits(self.handle, None if edits is None else edits.array, 0 if edits is None else edits.n))
        self.edits = edits

    def set_layer_limit(self, n):
        """``esmk_set_layer_limit``: the forwards of the handle stop after ``n`` layers; 0 (or L): the whole stack."""
        N = self.N
        N.check(N.lib.esmk_set_layer_limit(self.handle, int(n)))

    def _no_edits(self, what):
        if self.edits is not None:
            from .interventions import _NOT_BUILT

            raise ValueError(f"{what} while stream edits are active: {_NOT_BUILT}")

    @staticmethod
    def _skip(key):
        return key == "lm_head.weight" or key.endswith("inv_freq")

    def _pack_order(self, named):
        # LayerNorm parameters first: with the LayerNorm fold the q/k/v and fc1 weights are folded with them at pack time
        return sorted(named, key=lambda kt: 0 if "layer_norm" in kt[0] else 1)

    def workspace_bytes(self, B, T, flags):
        return self._query(self.N.lib.esmk_workspace_bytes, B, T, flags)

    def workspace_for(self, B, T, flags):
        return self.workspace_for_bytes(self.workspace_bytes(B, T, flags))

    def forward(self, tok, repr_set, reps, flags, logits, attn, contacts):
        """``esmk_forward`` on ``tok`` int64 [B, T] into the given outputs (None: not asked for; no ``logits``: contacts only)."""
        N = self.N
        B, T = tok.shape

        def launch(lo, hi, ws, stream):  # sequences lo : hi of every tensor (the whole batch: no slicing)
            part = (lambda t: t) if hi - lo == B else (lambda t: None if t is None else t[lo:hi])
            N.check(N.lib.esmk_forward(
                self.handle, N.ptr(self.packed), N.ptr(part(tok)), hi - lo, T, *self._repr_args(repr_set, [part(r) for r in reps]),
                flags, N.ptr(part(logits)), N.ptr(part(attn)), N.ptr(part(contacts)), N.ptr(ws), ws.numel(), stream))

        # (an edited call runs on one stream: its row lists count through the whole batch, and the handle's edits are one state)
        if (B >= 2 and logits is not None and self.edits is None and _dual_stream_wanted(B * T) and T <= self.max_T
                and not self.profiling and not torch.cuda.is_current_stream_capturing()):
            # two half-batches, the second on the engine's own stream (see _dual_stream_window): same bits
            cur = torch.cuda.current_stream(self.device)
            if self.stream2 is None:
                self.stream2 = torch.cuda.Stream(self.device)
            h = (B + 1) // 2
            need = self.workspace_bytes(h, T, flags)
            ws = self.workspace_for_bytes(need)
            ws2 = self._grown("workspace2", need)
            ready = torch.cuda.Event()
            ready.record(cur)                      # tokens, weights and the output allocations are ordered before the side stream
            self.stream2.wait_event(ready)
            launch(0, h, ws, ctypes.c_void_p(cur.cuda_stream))
            launch(h, B, ws2, ctypes.c_void_p(self.stream2.cuda_stream))
            done = torch.cuda.Event()
            done.record(self.stream2)
            cur.wait_event(done)                   # the caller's stream sees both halves
            self.dual_calls += 1
        else:
            launch(0, B, self.workspace_for(B, T, flags), N.cur_stream())
            self.max_T = max(self.max_T, T)

    def forward_packed(self, flat, seg, rows, repr_set, reps, flags, logits, flat_at, flat_ct):
        """The token-packed forward of the row space ``flat`` int64 [rows] with the host segment table ``seg`` int32 [n_seg, 2]:
        ``esmk_forward_packed_maps`` when the ragged attention maps ``flat_at`` are asked for, ``esmk_forward_packed_ex`` for
        the ragged contact maps ``flat_ct`` alone, ``esmk_forward_packed`` otherwise."""
        N = self.N
        self._no_edits("a token-packed forward")
        n_seg = seg.shape[0]
        seg_ptr = ctypes.cast(seg.data_ptr(), ctypes.POINTER(ctypes.c_int32))
        head = (self.handle, N.ptr(self.packed), N.ptr(flat), seg_ptr, n_seg, rows) + self._repr_args(repr_set, reps) + (
            flags, N.ptr(logits))
        if flat_at is not None:
            ws = self.workspace_for_bytes(self._query(N.lib.esmk_packed_workspace_bytes_maps, seg_ptr, n_seg, rows, flags))
            N.check(N.lib.esmk_forward_packed_maps(*head, N.ptr(flat_at), flat_at.numel(), N.ptr(flat_ct), N.ptr(ws),
                                                   ws.numel(), N.cur_stream()))
        elif flat_ct is not None:
            ws = self.workspace_for_bytes(self._query(N.lib.esmk_packed_workspace_bytes_ex, seg_ptr, n_seg, rows, flags))
            N.check(N.lib.esmk_forward_packed_ex(*head, N.ptr(flat_ct), N.ptr(ws), ws.numel(), N.cur_stream()))
        else:
            ws = self.workspace_for_bytes(self._query(N.lib.esmk_packed_workspace_bytes, n_seg, rows, flags))
            N.check(N.lib.esmk_forward_packed(*head, N.ptr(ws), ws.numel(), N.cur_stream()))

    def forward_rows(self, tok, sel_rows, V, return_logits=False, seg=None):
        """``esmk_forward_rows`` on padded [B, T] tokens, or (host table ``seg``) ``esmk_forward_packed_rows`` on [rows]."""
        lib = self.N.lib
        if seg is None:
            B, T = tok.shape
            got = self._rows(lib.esmk_rows_workspace_bytes, lib.esmk_forward_rows, (B, T), tok, sel_rows, V, return_logits)
            self.max_T = max(self.max_T, T)  # (not for a packed row space: its length is no row length)
            return got
        self._no_edits("a token-packed forward")
        seg_ptr = ctypes.cast(seg.data_ptr(), ctypes.POINTER(ctypes.c_int32))
        return self._rows(lib.esmk_packed_rows_workspace_bytes, lib.esmk_forward_packed_rows, (seg_ptr, seg.shape[0], tok.numel()),
                          tok, sel_rows, V, return_logits)

    def rows_contacts_bytes(self, B, T, n_sel):
        """The workspace ``esmk_forward_rows_contacts`` takes: the accumulators of the pinned head-group count included."""
        return self._query(self.N.lib.esmk_rows_contacts_workspace_bytes, B, T, n_sel, offset=True)[0]

    def forward_rows_contacts(self, tok, sel_rows, V, S):
        """``esmk_forward_rows_contacts`` on ``tok`` int64 [B, T]: (fp32 [n, V] log-probabilities of ``sel_rows``, or None when
        ``sel_rows`` is None or empty; fp32 [B, S, S] contact maps, each the bits of ``predict_contacts`` on that row alone)."""
        N = self.N
        B, T = tok.shape
        n = 0 if sel_rows is None else sel_rows.numel()
        ws = self.workspace_for_bytes(self.rows_contacts_bytes(B, T, n))
        out = torch.empty((n, V), dtype=torch.float32, device=self.device) if n else None
        contacts = torch.empty((B, S, S), dtype=torch.float32, device=self.device)  # S = T minus the <cls> / <eos> of the alphabet
        N.check(N.lib.esmk_forward_rows_contacts(self.handle, N.ptr(self.packed), N.ptr(tok), B, T, N.ptr(sel_rows if n else None), n,
                                                 N.ptr(out), N.ptr(contacts), N.ptr(ws), ws.numel(), N.cur_stream()))
        self.max_T = max(self.max_T, T)
        return out, contacts

    def set_pair_head(self, head):
        """The handle's pairwise head becomes ``head`` (``esm_amd.pair_head.PairHead`` or None); no call when it is."""
        if head is getattr(self, "pair_head", None):
            return
        N = self.N
        if head is None:
            N.check(N.lib.esmk_set_pair_head(self.handle, None, None, 0, 0))
        else:
            w, b = head.matrix(), head.bias()  # fp32 CPU [C, C_out], [C_out]: the handle copies them
            N.check(N.lib.esmk_set_pair_head(self.handle, N.ptr(w), N.ptr(b), head.n_sym, head.n_asym))
        self.pair_head = head

    def rows_pair_bytes(self, B, T, n_sel):
        """The workspace ``esmk_forward_rows_pair`` takes: the q / k / lse of every layer included."""
        return self._query(self.N.lib.esmk_rows_pair_workspace_bytes, B, T, n_sel, offset=True)[0]

    def forward_rows_pair(self, tok, sel_rows, V, pair_out):
        """``esmk_forward_rows_pair`` on ``tok`` int64 [B, T] with the head of ``set_pair_head``: fp32 [n, V] log-probabilities of
        ``sel_rows`` (None when there are none); ``pair_out`` fp32 [B, S, S, C_out] receives the pair logits."""
        N = self.N
        B, T = tok.shape
        n = 0 if sel_rows is None else sel_rows.numel()
        ws = self.workspace_for_bytes(self.rows_pair_bytes(B, T, n))
        out = torch.empty((n, V), dtype=torch.float32, device=self.device) if n else None
        assert pair_out.dtype == torch.float32 and pair_out.is_contiguous() and pair_out.shape[0] == B
        N.check(N.lib.esmk_forward_rows_pair(self.handle, N.ptr(self.packed), N.ptr(tok), B, T, N.ptr(sel_rows if n else None), n,
                                             N.ptr(out), N.ptr(pair_out), N.ptr(ws), ws.numel(), N.cur_stream()))
        self.max_T = max(self.max_T, T)
        return out


class MsaEngine(Engine):
    """The engine of ``MSATransformer``: ``esmk_msa_create`` and the ``esmk_msa_forward*`` entries."""

    def __init__(self, model, device, operand_dtype, weight_split=0):
        super().__init__(device, operand_dtype, weight_split)  # ESM_AMD_OPERAND=f16x2 / f16x2a: weight_split 1 / 2
        N = self.N
        a = model.args
        self.embed_dim = a.embed_dim
        cfg = N.EsmkMsaConfig(
            a.layers, a.embed_dim, a.attention_heads, a.ffn_embed_dim, model.alphabet_size, model.padding_idx,
            model.mask_idx, model.cls_idx, model.eos_idx if model.eos_idx is not None else -1,
            int(bool(model.prepend_bos)), int(bool(model.append_eos)), model.embed_positions.weight.shape[0],
            int(model.msa_position_embedding is not None), N.dtype_code(operand_dtype), self.weight_split)
        with torch.cuda.device(device):
            N.check(N.lib.esmk_msa_create(ctypes.byref(cfg), ctypes.byref(self.handle)))
            self._alloc_packed()

    def _pack_form(self, key, t):
        if key == "msa_position_embedding":  # [1,1024,1,D] (or [1,1024,1,1] in the first release) -> [1024,D]
            t = t.expand(1, t.shape[1], 1, self.embed_dim).reshape(t.shape[1], self.embed_dim)
        return t

    def forward(self, tok, repr_set, reps, flags, logits, row_attn, col_attn, contacts):
        """``esmk_msa_forward`` on ``tok`` int64 [B, R, C] into the given output tensors (None: not asked for)."""
        N = self.N
        B, R, C = tok.shape
        ws = self.workspace_for_bytes(self._query(N.lib.esmk_msa_workspace_bytes, B, R, C, flags))
        N.check(N.lib.esmk_msa_forward(
            self.handle, N.ptr(self.packed), N.ptr(tok), B, R, C, *self._repr_args(repr_set, reps), flags,
            N.ptr(logits), N.ptr(row_attn), N.ptr(col_attn), N.ptr(contacts), N.ptr(ws), ws.numel(), N.cur_stream()))

    def forward_rows(self, tok, sel_rows, V, return_logits=False):
        lib = self.N.lib
        return self._rows(lib.esmk_msa_rows_workspace_bytes, lib.esmk_msa_forward_rows, tuple(tok.shape), tok, sel_rows, V,
                          return_logits)


class _EngineHost:
    """What an ``nn.Module`` that runs on an ``Engine`` mixes in.  The class names its engine (``_engine_class``), its CPU
    refusal and, beyond its dimensions, ``_engine_config``; the engine lives in ``self._engine``, made on the first call."""

    _engine_class = None
    _cpu_refusal = ""

    def _engine_config(self):
        """Configuration beyond the model's dimensions, as keywords the engine class knows."""
        return {}

    def _engine_key(self):
        """The creation arguments of the engine; a changed key makes a new engine."""
        return _operand_dtype_for(self.embed_tokens.weight.dtype), _weight_split()

    def _get_engine(self, device, key=None):
        if key is None:
            key = self._engine_key()
        eng = self._engine
        if eng is None or eng.device != device or eng.key != key:
            new = self._engine_class(self, device, *key)  # (a refused configuration raises here: the current engine stays)
            if eng is not None:
                eng.close()
            eng = new
            object.__setattr__(self, "_engine", eng)
        return eng

    def _engine_ready(self, device):
        """The engine for this call with the current parameters packed."""
        eng = self._get_engine(device)
        eng.sync_weights(self)
        return eng

    def _check_devices(self, tokens):
        if not tokens.is_cuda:
            raise RuntimeError(self._cpu_refusal)
        w = self.embed_tokens.weight
        if w.device != tokens.device:
            raise RuntimeError(f"model parameters are on {w.device} but tokens on {tokens.device}")
        return w

    def _repr_set(self, repr_layers):
        return sorted({int(i) for i in repr_layers if 0 <= int(i) <= self.num_layers})

    @staticmethod
    def _cast_to(dtype):
        """The cast of an output to the model dtype (a tensor already in it passes through)."""
        return lambda t: t if t.dtype == dtype else t.to(dtype)

    def _selected_rows(self, tok, sel_rows, return_logits, *extra):
        """The tail the row-selected forwards share: an empty selection returns at once, else the engine's ``forward_rows``."""
        dev = sel_rows.device
        V = self.alphabet_size
        if sel_rows.numel() == 0:
            empty = torch.empty((0, V), dtype=torch.float32, device=dev)
            return (empty, empty.clone()) if return_logits else empty
        with torch.cuda.device(dev):
            return self._engine_ready(dev).forward_rows(tok, sel_rows, V, return_logits, *extra)

    def profile_begin(self):
        """Arm per-kernel-class HIP-event timing of the following forward calls (bench.py)."""
        if self._engine is None:
            raise RuntimeError("run one forward before profiling")
        self._engine.profile_begin()

    def profile_end(self):
        """Stop profiling; returns [{name, launches, ms, flops, bytes}] summed over the calls."""
        return self._engine.profile_end()

    def ln_fold_active(self):
        """True / False: the engine runs with / without the LayerNorm fold; None: no engine yet, or no fold."""
        return None if self._engine is None else self._engine.ln_fold_active()

    def refresh_engine(self):
        """Drop the engine state (call after replacing Parameter objects or sub-modules)."""
        if self._engine is not None:
            self._engine.close()
        object.__setattr__(self, "_engine", None)

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_engine"] = None  # the native handle is rebuilt lazily
        state.pop("_stream_edits", None)  # (active edits hold device pointers of this process)
        return state
