"""Writing into the model between layers: activation patching, steering, ablation.

A user of the reference registers a forward hook on ``model.layers[k]``, returns a changed output, and every later layer, the
head and any loop built on ``forward`` see the change.  Here the layer stack is one engine call, so the change is stated as data
— a ``StreamEdit`` — and the engine applies it to its fp32 residual stream between two layers (``esmk_set_stream_edits``,
csrc/interventions.hip):

    steer = StreamEdit(layer=12, op="add", value=direction, gain=4.0, positions="residues")
    out = model.forward_edited(tokens, [steer], repr_layers=[12, 33])        # one edited forward
    with model.stream_edits([steer]):                                        # everything that runs the padded engine path
        new = model.gibbs_sample(tokens, sweeps=4)
        scores = model.score_variants(alphabet, sequence, variants)

``layer`` k = 0 .. L names the stream after k layers (0: the embedded stream; L: the stream in front of the final LayerNorm,
for ESM-1 the stream the output projection reads).  The edit lands BEFORE representation k is captured: ``repr_layers`` shows
the edited stream, as a hook's return value would be what the next layer and the caller see.

ops        add    x' = x + gain * value            set    x' = gain * value (gain 1: the value itself: patching)
           scale  x' = gain * x                    zero   x' = 0
           project  x' = x - gain * <x, value> / <value, value> * value  (gain 1: the direction is projected out)
positions  "all" (every token but <pad>), "residues" (also without <cls>, <eos>, <mask>): token sets, independent of the batch
           shape; a bool mask [B, T] or an index tensor [n, 2] of (b, t) pairs: row lists of ONE batch shape
value      [E] (one vector for every row), [n, E] (row i of a row list), [B, T, E] (the value of every position: run A's
           representation k patched into run B)

Inside ``model.stream_edits`` only token-set edits with an [E] value (or none) are taken: the functions that run there
choose their own batch shapes.  Not built: token-packed batches (``varlen=True``, ``forward_varlen``), windows (``window=``,
``forward_windows``) and the MSA Transformer.
"""
import contextlib

import torch

OPS = ("add", "set", "scale", "zero", "project")
_NEEDS_VALUE = ("add", "set", "project")
_NOT_BUILT = ("stream edits run on padded batches only: token-packed batches (varlen=True, forward_varlen) and windows (window=, "
              "forward_windows) are not built")


def token_set(model, positions):
    """The 64-bit token selector of ``"all"`` / ``"residues"`` for a model's alphabet: bit v set = rows holding token v."""
    V = int(model.alphabet_size)
    if V > 64:
        raise ValueError(f"token-set positions need a vocabulary of at most 64 entries (this one has {V})")
    out = {"all": (model.padding_idx,), "residues": (model.padding_idx, model.cls_idx, model.eos_idx, model.mask_idx)}[positions]
    bits = (1 << V) - 1
    for v in out:
        if v is not None and 0 <= int(v) < V:
            bits &= ~(1 << int(v))
    return bits


class StreamEdit:
    """One edit of the residual stream after ``layer`` layers (module docstring).  Construction checks what needs no batch;
    ``plan(model, B, T)`` normalises the rest for one batch shape, on the host."""

    def __init__(self, layer, op="add", value=None, gain=1.0, positions="all"):
        if op not in OPS:
            raise ValueError(f"StreamEdit: op must be one of {OPS}, got {op!r}")
        if op in _NEEDS_VALUE and value is None:
            raise ValueError(f"StreamEdit: op {op!r} needs a value")
        if op not in _NEEDS_VALUE and value is not None:
            raise ValueError(f"StreamEdit: op {op!r} takes no value (gain alone)")
        if value is not None:
            value = torch.as_tensor(value)
            if value.dim() not in (1, 2, 3) or not value.is_floating_point():
                raise ValueError("StreamEdit: value must be a floating-point tensor of shape [E], [n, E] or [B, T, E]")
        if isinstance(positions, str):
            if positions not in ("all", "residues"):
                raise ValueError("StreamEdit: positions must be 'all', 'residues', a bool mask [B, T] or an index tensor [n, 2]")
        else:
            positions = torch.as_tensor(positions)
            is_mask = positions.dtype == torch.bool and positions.dim() == 2
            is_index = positions.dtype in (torch.int32, torch.int64) and positions.dim() == 2 and positions.shape[1] == 2
            if not (is_mask or is_index):
                raise ValueError("StreamEdit: positions must be 'all', 'residues', a bool mask [B, T] or an index tensor [n, 2]")
        self.layer, self.op, self.value, self.gain, self.positions = int(layer), op, value, float(gain), positions

    @property
    def by_tokens(self):
        """True: the rows are chosen by their tokens (any batch shape); False: a row list of one batch shape."""
        return isinstance(self.positions, str)

    def coefficients(self):
        """(engine op, keep, gain) of ``x' = keep x + gain s`` / the projection."""
        from . import _native as N

        return {"add": (N.EDIT_AXPBY, 1.0, self.gain), "set": (N.EDIT_AXPBY, 0.0, self.gain),
                "scale": (N.EDIT_AXPBY, self.gain, 0.0), "zero": (N.EDIT_AXPBY, 0.0, 0.0),
                "project": (N.EDIT_PROJECT, 1.0, self.gain)}[self.op]

    def rows(self, B, T):
        """int64 host tensor of the flat rows b*T + t of a row-list edit for a [B, T] batch, in list (mask: row-major) order."""
        pos = self.positions.cpu()
        if pos.dtype == torch.bool:
            if tuple(pos.shape) != (B, T):
                raise ValueError(f"StreamEdit: the positions mask is {tuple(pos.shape)}, the batch is {(B, T)}")
            return pos.reshape(-1).nonzero().reshape(-1)
        pos = pos.to(torch.int64)
        if pos.numel() and (pos[:, 0].min() < 0 or pos[:, 0].max() >= B or pos[:, 1].min() < 0 or pos[:, 1].max() >= T):
            raise ValueError(f"StreamEdit: a position index lies outside the batch {(B, T)}")
        rows = pos[:, 0] * T + pos[:, 1]
        if rows.unique().numel() != rows.numel():
            raise ValueError("StreamEdit: a position is listed twice (the order of two edits of one row is not defined)")
        return rows

    def plan(self, model, B=None, T=None):
        """The edit for one batch shape as host data: dict(layer, op, keep, gain, token_set | rows, src, src_index).  ``B`` and
        ``T`` None: any batch shape (inside ``model.stream_edits``) — a row list or a per-position value is a ValueError."""
        L, E = int(model.num_layers), int(model.embed_dim)
        if not 0 <= self.layer <= L:
            raise ValueError(f"StreamEdit: layer {self.layer} is outside 0 .. {L} (the stream after that many layers)")
        op, keep, gain = self.coefficients()
        plan = dict(layer=self.layer, op=op, keep=keep, gain=gain, token_set=0, rows=None, src=None, src_index=None)
        free = B is None
        if self.by_tokens:
            plan["token_set"] = token_set(model, self.positions)
        elif free:
            raise ValueError("model.stream_edits takes token-set edits only (positions 'all' / 'residues'): the functions that run "
                             "inside choose their own batch shapes, which a row list cannot follow; use forward_edited")
        else:
            plan["rows"] = self.rows(B, T).to(torch.int32)
        v = self.value
        if v is None:
            return plan
        if v.shape[-1] != E:
            raise ValueError(f"StreamEdit: value has {v.shape[-1]} columns, the model's embed_dim is {E}")
        if v.dim() == 1:
            plan["src"] = v
        elif v.dim() == 3:
            if free:
                raise ValueError("model.stream_edits takes values of shape [E] only: a [B, T, E] value belongs to one batch shape")
            if tuple(v.shape[:2]) != (B, T):
                raise ValueError(f"StreamEdit: value is {tuple(v.shape)}, the batch is {(B, T)}")
            plan["src"] = v.reshape(B * T, E)
            plan["src_index"] = plan["rows"]  # row r of the batch reads row r of the value (token set: the kernel's default)
        else:
            if self.by_tokens:
                raise ValueError("StreamEdit: a value of shape [n, E] goes with a row list (mask or index positions)")
            if v.shape[0] != plan["rows"].numel():
                raise ValueError(f"StreamEdit: value has {v.shape[0]} rows, positions select {plan['rows'].numel()}")
            plan["src"] = v
        return plan


class DeviceEdits:
    """A planned list of edits on one device: the ``esmk_stream_edit`` array and the tensors its pointers borrow."""

    def __init__(self, plans, device):
        from . import _native as N
        from . import ops

        self.device = device
        self.keep = []  # the device tensors, alive as long as the handle may read them

        def dev(t, dtype):
            if t is None:
                return None
            t = t.detach().to(device=device, dtype=dtype).contiguous()
            self.keep.append(t)
            return t

        descs = []
        for p in plans:
            n_rows = None if p["rows"] is None else p["rows"].numel()
            rows = dev(torch.zeros(1) if n_rows == 0 else p["rows"], torch.int32)  # (an empty list keeps a non-null address)
            index = rows if p["src_index"] is p["rows"] else dev(p["src_index"], torch.int32)
            if n_rows == 0:
                index = None
            descs.append(ops.stream_edit_desc(p["layer"], p["op"], p["keep"], p["gain"], rows, p["token_set"],
                                              dev(p["src"], torch.float32), None, index, n_rows))
        self.array = (N.EsmkStreamEdit * max(1, len(descs)))(*descs)
        self.n = len(descs)


def plan_edits(model, edits, B=None, T=None):
    """[plan] of ``edits`` (a StreamEdit or a sequence of them) for a [B, T] batch, or for any batch shape (B None)."""
    from .msa_transformer import MSATransformer

    if isinstance(model, MSATransformer):
        raise NotImplementedError("stream edits are built for ESM-2, ESM-1b / ESM-1v and ESM-1; the MSA Transformer's axial stack "
                                  "has no edit point yet")
    if isinstance(edits, StreamEdit):
        edits = [edits]
    edits = list(edits)
    for e in edits:
        if not isinstance(e, StreamEdit):
            raise TypeError(f"expected StreamEdit objects, got {type(e).__name__}")
    if len(edits) > 64:  # ESMK_MAX_STREAM_EDITS
        raise ValueError(f"at most 64 stream edits at a time, got {len(edits)}")
    return [e.plan(model, B, T) for e in edits]


@contextlib.contextmanager
def _active(model, plans):
    """``plans`` as the model's active edits for the calls inside; an empty list changes nothing at all."""
    if not plans:
        yield
        return
    device = model.embed_tokens.weight.device
    if device.type != "cuda":
        raise RuntimeError(model._cpu_refusal)
    with torch.cuda.device(device):
        dev = DeviceEdits(plans, device)
    prev = model.__dict__.get("_stream_edits")
    object.__setattr__(model, "_stream_edits", dev)
    try:
        yield
    finally:
        object.__setattr__(model, "_stream_edits", prev)
        if model._engine is not None:  # the handle drops its borrowed pointers before the tensors go
            model._engine.set_edits(prev)


def stream_edits(model, edits):
    """``with model.stream_edits(edits):`` — every padded-path engine call of the model inside runs edited."""
    return _active(model, plan_edits(model, edits))


def forward_edited(model, tokens, edits, repr_layers=[], need_head_weights=False, return_contacts=False, contacts_only=False):
    """``forward``'s dict of one forward under ``edits``; row lists and per-position values refer to this batch."""
    assert tokens.ndim == 2
    plans = plan_edits(model, edits, *tokens.shape)
    with _active(model, plans):
        return model.forward(tokens, repr_layers=repr_layers, need_head_weights=need_head_weights,
                             return_contacts=return_contacts, contacts_only=contacts_only)


def mean_difference(model, tokens_a, tokens_b, layer, positions="residues"):
    """fp32 [E]: the mean of representation ``layer`` over the ``positions`` rows of the sequences ``tokens_a`` minus the same
    over ``tokens_b`` — the usual steering direction.  Right-padded batches; "residues": the rows between <cls> and <eos>,
    "all": every row up to the last non-pad token.  Per-sequence means by ``esmk_op_masked_row_mean``, combined with the
    sequences' row counts as weights."""
    from . import ops

    if positions not in ("all", "residues"):
        raise ValueError("mean_difference: positions must be 'all' or 'residues'")
    ends = (int(model.prepend_bos), int(model.append_eos)) if positions == "residues" else (0, 0)

    def mean_of(tokens):
        rep = model.forward(tokens, repr_layers=[layer])["representations"][layer]
        n = (tokens.to(rep.device).ne(model.padding_idx).sum(1) - sum(ends)).clamp(min=0).to(torch.int32)
        per_seq = ops.masked_row_mean(rep.contiguous(), n.contiguous(), first_row=ends[0])  # [B, E] fp32; NaN where n = 0
        w = n.to(torch.float32)
        if not bool((w > 0).any()):
            raise ValueError("mean_difference: no row selected")
        return (torch.nan_to_num(per_seq) * w[:, None]).sum(0) / w.sum()

    return mean_of(tokens_a) - mean_of(tokens_b)
