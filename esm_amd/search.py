"""Protein search: an index of pooled embeddings, a cosine top-k on the device, the aligner on the survivors.

    index = esm_amd.EmbeddingIndex.build(model, alphabet, records, layer=20)      # one fp32 [E] vector per protein
    index.save("db.npz"); index = esm_amd.EmbeddingIndex.load("db.npz").to("cuda")
    hits = model.search(index, tokens, top_k=100)                                  # scores fp32 [Q, k], ids int32 [Q, k]
    out = esm_amd.search_and_align(model, alphabet, queries, index, top_k=100, align_top=10, mode="local")

    python -m esm_amd.search index --model-location M --fasta DB.fasta [--layer K] [--no-sequences] [--center] --output db.npz
    python -m esm_amd.search query --model-location M --index db.npz --query Q.fasta --top N [--align ...] --output hits.tsv

Definition (tests/_search_ref.py restates it in numpy, and the kernels reproduce that bit for bit).
A protein's vector: ``model.pool`` — representation ``layer`` of its residues (<cls>, <eos> and <pad> are no rows), summed per
column in fp64 in residue order, divided by the residue count, rounded once to fp32 (``esmk_op_pool_rows``).  The engine's rows
carry the same bits alone, in a padded batch and token-packed, so a vector does not depend on how its protein was batched.
The similarity of a query and a database vector is the cosine of ``align``: both scaled to unit length by ``esmk_op_align_rows``
and multiplied on the 16-bit matrix rate in the f16x3 form (hi hi + hi lo + lo hi, fp32 accumulation): near-fp32.
The top-k of a query row: value descending in the total order of the IEEE bits, ties to the lower database id; NaN is no
candidate; the database is walked in blocks of ``Nb`` vectors, one GEMM into an fp32 [Q, Nb] scratch and one
``esmk_op_topk_merge`` per block, so no [Q, N] matrix exists; a list shorter than k ends in (-inf, -1).
``model.embed_layer`` runs only the layers below the representation (``esmk_set_layer_limit``): building an index of a
mid-stack layer costs that share of the forward.

A centred index (``index.centered()``, ``index --center``) holds ``center`` fp32 [E], the database mean — per column the fp64 sum
of the vectors in ascending id, divided by N, rounded once — and vectors with it subtracted (one fp32 subtraction); ``search``
and ``range_search`` subtract it from fp32 queries before the unit scaling.  Raw mean vectors of a language model share a large
common component, so their cosines are high between unrelated proteins; thresholds (``range_search``, ``cluster``:
esm_amd/cluster.py) only mean something on a centred index.

Not built: a whitened index, a 16-bit-only image at a third of the memory, a host-streamed or multi-GPU sharded index,
IVF / quantised search, the MSA Transformer, windows (``window=``).
"""
import json

import numpy as np
import torch

MAX_K = 1024
MAX_BLOCK = 1 << 22  # the columns one esmk_op_topk_merge launch takes
BLOCK_ALIGN = 256
SIM_LIMIT = 1 << 24  # return_similarity: the largest [Q, N] matrix handed back


def _up(n, m):
    return (n + m - 1) // m * m


# ---- the model side: early exit and pooling ---------------------------------------------------------------------------------
def check_model(model, layer, window=None, what="embed_layer"):
    from .msa_transformer import MSATransformer

    if isinstance(model, MSATransformer):
        raise NotImplementedError(f"{what} is built for ESM-2, ESM-1b / ESM-1v and ESM-1; not for the MSA Transformer")
    if window is not None:
        raise NotImplementedError(f"{what}: windows (window=) are not built")
    layer = int(model.num_layers) if layer is None else int(layer)
    if not 0 <= layer <= int(model.num_layers):
        raise ValueError(f"{what}: layer {layer} is outside 0 .. {int(model.num_layers)}")
    return layer


def embed_layer(model, tokens, layer=None, varlen=False, window=None):
    """fp32 [B, T, E]: ``model(tokens, repr_layers=[layer])["representations"][layer]`` bit for bit (``varlen=True``:
    ``forward_varlen``'s, zeros at <pad>), from a forward that ends after ``layer`` layers: no head, and for ``layer`` below the
    model's L none of the layers above.  ``layer`` None or L is the whole stack (ESM-2's final LayerNorm is part of that
    representation), and so is layer 0, which the engine's limit cannot express.  The handle's limit is set around the call and
    cleared whatever happens.  Inside ``model.stream_edits`` the edits at layers <= ``layer`` apply; a later one is a
    ValueError (nothing it changes is computed)."""
    from . import _native as N
    from .engine import _native_lowp, warn_if_grad_expected
    from .packing import pack_plan

    layer = check_model(model, layer, window)
    assert tokens.ndim == 2
    held = model.__dict__.get("_stream_edits")
    if held is not None:
        model._refuse_under_edits(varlen=varlen)
        for i in range(held.n):
            if int(held.array[i].layer) > layer:
                raise ValueError(f"embed_layer(layer={layer}) inside model.stream_edits(...): the edit at layer "
                                 f"{int(held.array[i].layer)} lies above the last layer that runs")
    w = model.embed_tokens.weight
    if not w.is_cuda:
        raise RuntimeError(model._cpu_refusal)
    warn_if_grad_expected(model)
    dev = w.device
    B, T = tokens.shape
    E, L = model.embed_dim, int(model.num_layers)
    packed = bool(varlen) and model._packs()  # (f16x3 and ESM-1 have no token-packed form: the padded path, the same bits)
    with torch.cuda.device(dev):
        eng = model._engine_ready(dev)
        lowp = _native_lowp(w.dtype, eng.operand_dtype)
        flags = N.OUT_REPR_LOWP if lowp else 0
        rdt = w.dtype if lowp else torch.float32
        eng.set_layer_limit(layer if 0 < layer < L else 0)
        try:
            if packed:
                plan = pack_plan(tokens, model.padding_idx)
                idx, keep = plan.index(dev)
                flat = plan.pack(tokens, model.padding_idx, idx)
                rep = torch.empty((plan.rows, E), dtype=rdt, device=dev)
                eng.forward_packed(flat, plan.segments, plan.rows, [layer], [rep], flags, None, None, None)
                rep = plan.unpack(rep, idx, keep)
            else:
                tok = tokens.to(dev).to(torch.int64).contiguous()
                rep = torch.empty((B, T, E), dtype=rdt, device=dev)
                eng.forward(tok, [layer], [rep], flags, None, None, None)
                if varlen:  # forward_varlen's convention on the padded route too
                    rep = rep.masked_fill_(tok.eq(model.padding_idx).unsqueeze(-1), 0)
        finally:
            eng.set_layer_limit(0)
    return rep.to(w.dtype).to(torch.float32)


def pool(model, tokens, layer=None, varlen=False, window=None):
    """fp32 [B, E]: per sequence the mean of its residue rows of representation ``layer`` (module docstring); a sequence
    without residues gives a zero vector."""
    from . import ops
    from .align import residue_rows

    check_model(model, layer, window, "pool")
    rep = embed_layer(model, tokens, layer=layer, varlen=varlen)
    B, T, E = rep.shape
    with torch.cuda.device(rep.device):
        rows, lengths = residue_rows(model, tokens.to(rep.device))
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)).to(rep.device)
        return ops.pool_rows(rep.reshape(B * T, E), rows, off)


def search(model, index, tokens, top_k, varlen=False, **kw):
    """``model.search``: ``pool`` of ``tokens`` at the index's layer, then ``index.search``."""
    index.check_model(model)
    return index.search(pool(model, tokens, layer=index.meta["layer"], varlen=varlen), top_k, **kw)


def _batches(records, batch_tokens):
    """Index lists into ``records`` [(label, sequence)], sorted by length: a batch's padded token grid holds at most
    ``batch_tokens`` tokens (one sequence always fits)."""
    order = sorted(range(len(records)), key=lambda i: (len(records[i][1]), i))
    out, lo = [], 0
    while lo < len(order):
        hi, longest = lo, 0
        while hi < len(order) and (hi == lo or max(longest, len(records[order[hi]][1]) + 2) * (hi + 1 - lo) <= batch_tokens):
            longest = max(longest, len(records[order[hi]][1]) + 2)
            hi += 1
        out.append(order[lo:hi])
        lo = hi
    return out


def pool_records(model, alphabet, records, layer=None, batch_tokens=65536, varlen=True):
    """fp32 [len(records), E] on the model's device: ``model.pool`` per batch of similar lengths, results in record order."""
    layer = check_model(model, layer, None, "pool")
    convert = alphabet.get_batch_converter()
    dev = model.embed_tokens.weight.device
    out = torch.zeros((len(records), model.embed_dim), dtype=torch.float32, device=dev)
    for batch in _batches(records, batch_tokens):
        _, _, tokens = convert([records[i] for i in batch])
        out[torch.tensor(batch, device=dev)] = pool(model, tokens.to(dev), layer=layer, varlen=varlen)
    return out


# ---- blocks -----------------------------------------------------------------------------------------------------------------
def plan_search(n_db, n_q, max_bytes):
    """(queries per chunk, database vectors per block) of a search: the fp32 [Qc, Nb] scratch of one GEMM fits ``max_bytes``,
    Nb is a multiple of 256, at most 2^22 (one top-k launch) and no more than the database rounded up to 256.  Pure."""
    n_db, n_q, max_bytes = int(n_db), int(n_q), int(max_bytes)
    if n_db < 1 or n_q < 1:
        raise ValueError(f"search: need at least one query and one database vector, got {n_q} and {n_db}")
    if max_bytes < 4 * BLOCK_ALIGN:
        raise ValueError(f"search: max_bytes = {max_bytes} does not hold one query row of {BLOCK_ALIGN} similarities")
    qc = min(n_q, max_bytes // (4 * BLOCK_ALIGN))
    nb = min(_up(n_db, BLOCK_ALIGN), MAX_BLOCK, max_bytes // (4 * qc) // BLOCK_ALIGN * BLOCK_ALIGN)
    return qc, nb


# ---- the index --------------------------------------------------------------------------------------------------------------
class EmbeddingIndex:
    """One pooled vector per protein: ``vectors`` fp32 [N, E] on the host, ``labels`` and ``lengths`` (residues) per protein,
    optionally the ``sequences`` (``search_and_align`` embeds the hits again), and ``meta``: layer, pooling ("mean"), the
    model's num_layers / embed_dim and a free-form model name.  ``.to(device)`` builds what a search reads."""

    META_KEYS = ("layer", "pooling", "num_layers", "embed_dim", "model")

    def __init__(self, vectors, labels, lengths, sequences=None, meta=None, center=None):
        if isinstance(center, torch.Tensor):
            center = center.detach().to("cpu", torch.float32).numpy()
        self.center = None if center is None else np.ascontiguousarray(center, dtype=np.float32).reshape(-1)  # already subtracted
        if isinstance(vectors, torch.Tensor):
            vectors = vectors.detach().to("cpu", torch.float32).numpy()
        self.vectors = np.ascontiguousarray(vectors, dtype=np.float32)
        if self.vectors.ndim != 2 or self.vectors.shape[0] < 1:
            raise ValueError("EmbeddingIndex: vectors must be a non-empty [N, E] array")
        if self.vectors.shape[1] % 4 != 0:
            raise ValueError(f"EmbeddingIndex: E = {self.vectors.shape[1]} must be a multiple of 4")
        n = self.vectors.shape[0]
        if self.center is not None and self.center.shape[0] != self.vectors.shape[1]:
            raise ValueError(f"EmbeddingIndex: center has {self.center.shape[0]} entries, the vectors have E = {self.vectors.shape[1]}")
        self.labels = [str(s) for s in labels]
        self.lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        self.sequences = None if sequences is None else [str(s) for s in sequences]
        if len(self.labels) != n or len(self.lengths) != n or (self.sequences is not None and len(self.sequences) != n):
            raise ValueError(f"EmbeddingIndex: {n} vectors, {len(self.labels)} labels, {len(self.lengths)} lengths"
                             + ("" if self.sequences is None else f", {len(self.sequences)} sequences"))
        self.meta = dict(layer=None, pooling="mean", num_layers=None, embed_dim=int(self.vectors.shape[1]), model="")
        self.meta.update(meta or {})
        if self.meta["pooling"] != "mean":
            raise ValueError(f"EmbeddingIndex: pooling {self.meta['pooling']!r} is not built (only 'mean')")
        self.image = None  # fp16 [N rounded up to 256, 3 Ep] on the device: the b-side f16x3 image of the unit vectors

    def __len__(self):
        return int(self.vectors.shape[0])

    @property
    def device(self):
        return None if self.image is None else self.image.device

    # -- files
    def save(self, path):
        """An .npz of plain arrays (no pickle): vectors, labels, lengths, meta as JSON and, if held, the sequences and the
        center."""
        arrays = dict(vectors=self.vectors, labels=np.array(self.labels, dtype=np.str_), lengths=self.lengths,
                      meta=np.array(json.dumps(self.meta), dtype=np.str_))
        if self.sequences is not None:
            arrays["sequences"] = np.array(self.sequences, dtype=np.str_)
        if self.center is not None:
            arrays["center"] = self.center
        with open(path, "wb") as fh:
            np.savez(fh, **arrays)

    @classmethod
    def load(cls, path):
        """Reads what ``save`` wrote, with ``allow_pickle=False``: a file with pickled (object) arrays is a ValueError."""
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in ("vectors", "labels", "lengths", "meta") if k not in z.files]
            if missing:
                raise ValueError(f"EmbeddingIndex.load: {path} has no array {missing[0]!r}")
            seqs = z["sequences"].tolist() if "sequences" in z.files else None
            center = z["center"] if "center" in z.files else None
            return cls(z["vectors"], z["labels"].tolist(), z["lengths"], seqs, json.loads(str(z["meta"])), center)

    def centered(self):
        """A new index on the host with the database mean subtracted (module docstring): ``center[e]`` is the fp64 sum of
        ``vectors[i][e]`` in ascending i, divided by N and rounded once to fp32; every vector loses it in one fp32
        subtraction.  Labels, lengths, sequences and meta are carried over.  An index that is centred already is a ValueError."""
        if self.center is not None:
            raise ValueError("EmbeddingIndex.centered: the index is centred already")
        acc = np.zeros((self.vectors.shape[1],), dtype=np.float64)
        for row in self.vectors:  # one addition per vector: ascending order (np.sum would add pairwise)
            acc += row
        center = (acc / np.float64(len(self))).astype(np.float32)
        return EmbeddingIndex(self.vectors - center, self.labels, self.lengths, self.sequences, self.meta, center)

    # -- building
    @classmethod
    def build(cls, model, alphabet, records, layer=None, batch_tokens=65536, varlen=True, keep_sequences=True, model_name=""):
        """The index of ``records`` [(label, sequence)]: sorted by length, ``model.pool`` per batch of at most ``batch_tokens``
        tokens, vectors in record order — the same bits whatever ``batch_tokens`` and ``varlen`` are.  ``varlen`` runs
        token-packed where the model has that form."""
        layer = check_model(model, layer, None, "EmbeddingIndex.build")
        records = [(str(a), str(b)) for a, b in records]
        vec = pool_records(model, alphabet, records, layer, batch_tokens, varlen)
        meta = dict(layer=layer, pooling="mean", num_layers=int(model.num_layers), embed_dim=int(model.embed_dim), model=str(model_name))
        return cls(vec.cpu(), [r[0] for r in records], [len(r[1]) for r in records], [r[1] for r in records] if keep_sequences else None,
                   meta)

    def check_model(self, model):
        """A ValueError unless the index was built on this model's dimensions (layer, embed_dim, num_layers)."""
        want = dict(embed_dim=int(model.embed_dim), num_layers=int(model.num_layers))
        for k, v in want.items():
            if self.meta.get(k) != v:
                raise ValueError(f"search: the index was built with {k} = {self.meta.get(k)}, the model has {k} = {v}")
        layer = self.meta.get("layer")
        if layer is None or not 0 <= int(layer) <= want["num_layers"]:
            raise ValueError(f"search: the index names layer {layer}, the model has layers 0 .. {want['num_layers']}")

    # -- the device side
    def image_bytes(self):
        Ep = _up(int(self.vectors.shape[1]), 64)
        return _up(len(self), BLOCK_ALIGN) * 3 * Ep * 2

    def to(self, device, rows_per_upload=1 << 16):
        """Builds and holds the device image: fp16 [N rounded up to 256, 3 Ep], the b-side f16x3 form of the cosine unit
        vectors (``esmk_op_align_rows``), uploaded and converted in row blocks; rows behind N are zero.  Nothing else stays on
        the device.  An image that does not fit is a ValueError."""
        from . import ops

        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("EmbeddingIndex.to: search runs only on an MI355X (ROCm) device; there is no CPU fallback")
        need = self.image_bytes()
        with torch.cuda.device(device):
            free = torch.cuda.mem_get_info()[0]
            if need > free:
                raise ValueError(f"EmbeddingIndex.to: the image of {len(self)} vectors takes {need} bytes, {free} are free on {device}; "
                                 "shard the index (several EmbeddingIndex objects searched in turn, their top-k lists merged)")
            n, E = self.vectors.shape
            Ep = _up(E, 64)
            image = torch.zeros((_up(n, BLOCK_ALIGN), 3 * Ep), dtype=torch.float16, device=device)
            for lo in range(0, n, rows_per_upload):
                x = torch.from_numpy(self.vectors[lo:lo + rows_per_upload]).to(device)
                ops.align_rows(x, None, cosine=True, b_side=True, out=image[lo:lo + x.shape[0]])
        self.image = image
        return self

    def _query_vectors(self, queries, what):
        """(queries as an [Q, E] tensor, whether the center still has to be subtracted).  Another index brings vectors that
        are centred already: it must hold this index's center, or none while this one holds none."""
        subtract = self.center is not None
        if isinstance(queries, EmbeddingIndex):
            if (queries.center is None) != (self.center is None) or (subtract and not np.array_equal(queries.center, self.center)):
                raise ValueError(f"{what}: the query index and the database index do not hold the same center "
                                 f"(query: {'none' if queries.center is None else 'one'}, database: "
                                 f"{'none' if self.center is None else 'one'}); center both on one vector, or neither")
            queries, subtract = torch.from_numpy(queries.vectors), False
        if not isinstance(queries, torch.Tensor) or queries.dim() != 2:
            raise ValueError(f"{what}: queries must be an fp32 [Q, E] tensor or an EmbeddingIndex")
        E = self.vectors.shape[1]
        if queries.shape[1] != E:
            raise ValueError(f"{what}: queries have E = {queries.shape[1]}, the index has E = {E}")
        return queries, subtract

    def _query_rows(self, queries, subtract, dev):
        """fp32 [Q, E] on the device, the center subtracted (one fp32 subtraction) where the index holds one."""
        q = queries.detach().to(dev, torch.float32).contiguous()
        return q - torch.from_numpy(self.center).to(dev) if subtract else q

    def _similarity_blocks(self, img_q, Q, max_bytes):
        """Yields (q0, q1, n0, cols, S) over the blocks of ``plan_search``: S fp32 [q1 - q0, cols rounded up to 256] is the
        GEMM of the queries' image and database rows n0 .. n0 + cols - 1, in a scratch that the next block overwrites."""
        from . import _native as N
        from . import ops

        n = len(self)
        qc, nb = plan_search(n, Q, max_bytes)
        scratch = torch.empty((qc * nb,), dtype=torch.float32, device=img_q.device)
        for q0 in range(0, Q, qc):
            q1 = min(q0 + qc, Q)
            for n0 in range(0, n, nb):
                cols = min(nb, n - n0)
                width = _up(cols, BLOCK_ALIGN)  # (the image has these rows: zeros behind N)
                S = scratch[:(q1 - q0) * width].view(q1 - q0, width)
                ops.linear(img_q[q0:q1], self.image[n0:n0 + width], None, N.EPI_STORE_F32, out=S)
                yield q0, q1, n0, cols, S

    def range_search(self, queries, threshold, exclude_self=False, max_edges=1 << 28, max_bytes=2 << 30):
        """Every database vector whose cosine to a query is at least ``threshold``: a CSR of device tensors, ``offsets`` int64
        [Q + 1], ``ids`` int32 [nnz] and ``scores`` fp32 [nnz]; row q lists, in ascending id, every j with ``S[q][j] >=
        threshold`` (a float comparison: NaN never passes, a tie does), S the matrix ``search(return_similarity=True)``
        returns.  ``exclude_self`` leaves id q out of row q.  Two passes over the blocks of ``plan_search``, the [Q, N]
        matrix never exists: the GEMM and a count launch (``esmk_op_range_rows``) per block, one read of the total by the
        host — more than ``max_edges`` is a ValueError — a cumulative sum, then the same GEMMs and a fill launch per block."""
        from . import ops

        queries, subtract = self._query_vectors(queries, "range_search")
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("range_search: the threshold is NaN")
        if int(max_edges) < 0:
            raise ValueError(f"range_search: max_edges = {max_edges} is negative")
        Q = int(queries.shape[0])
        plan_search(len(self), max(Q, 1), max_bytes)
        if self.image is None:
            raise RuntimeError("EmbeddingIndex.range_search: call .to(device) first (the device image has not been built)")
        dev = self.image.device
        with torch.cuda.device(dev):
            counts = torch.zeros((Q,), dtype=torch.int64, device=dev)
            offsets = torch.zeros((Q + 1,), dtype=torch.int64, device=dev)
            empty = dict(offsets=offsets, ids=torch.empty((0,), dtype=torch.int32, device=dev),
                         scores=torch.empty((0,), dtype=torch.float32, device=dev))
            if Q == 0:
                return empty
            img_q = ops.align_rows(self._query_rows(queries, subtract, dev), None, cosine=True, b_side=False)
            exclude = torch.arange(Q, dtype=torch.int32, device=dev) if exclude_self else None
            for q0, q1, n0, cols, S in self._similarity_blocks(img_q, Q, max_bytes):
                ops.range_rows(S, threshold, counts=counts[q0:q1], n_cols=cols, id_base=n0,
                               exclude=None if exclude is None else exclude[q0:q1])
            total = int(counts.sum())  # the one read
            if total > int(max_edges):
                raise ValueError(f"range_search: threshold {threshold:g} passes {total} pairs, more than max_edges = {int(max_edges)}; "
                                 "raise the threshold, or center the index first (EmbeddingIndex.centered()): raw mean vectors "
                                 "share a large common component and their cosines are high everywhere")
            torch.cumsum(counts, 0, out=offsets[1:])
            if total == 0:
                return empty
            cursor = offsets[:-1].clone()
            ids = torch.empty((total,), dtype=torch.int32, device=dev)
            scores = torch.empty((total,), dtype=torch.float32, device=dev)
            for q0, q1, n0, cols, S in self._similarity_blocks(img_q, Q, max_bytes):
                ops.range_rows(S, threshold, offsets=offsets[q0:q1 + 1], cursor=cursor[q0:q1], ids=ids, scores=scores, n_cols=cols,
                               id_base=n0, exclude=None if exclude is None else exclude[q0:q1])
        return dict(offsets=offsets, ids=ids, scores=scores)

    def cluster(self, threshold, priority="length", assign="first", max_edges=1 << 28, max_bytes=2 << 30):
        """``esm_amd.cluster.cluster_embeddings`` on this index: greedy incremental clustering at cosine ``threshold``."""
        from .cluster import cluster_embeddings

        return cluster_embeddings(self, threshold, priority=priority, assign=assign, max_edges=max_edges, max_bytes=max_bytes)

    def search(self, queries, top_k, exclude_self=False, return_similarity=False, max_bytes=2 << 30):
        """The ``top_k`` nearest database vectors of every query by cosine (module docstring): a dict of device tensors
        ``scores`` fp32 [Q, k] and ``ids`` int32 [Q, k] (-inf / -1 behind the last hit).  ``queries``: fp32 [Q, E] or another
        ``EmbeddingIndex``.  ``exclude_self``: query q skips database id q (an index searched against itself).
        ``return_similarity`` also returns ``similarity`` fp32 [Q, N] as the GEMM wrote it (tests; at most 2^24 elements).  Per
        block of the database one GEMM and one merge launch on the current stream; the host reads nothing in between."""
        from . import ops

        queries, subtract = self._query_vectors(queries, "search")
        n = len(self)
        top_k = int(top_k)
        if not 1 <= top_k <= MAX_K:
            raise ValueError(f"search: top_k must be 1 .. {MAX_K}, got {top_k}")
        Q = int(queries.shape[0])
        if return_similarity and Q * n > SIM_LIMIT:
            raise ValueError(f"search: return_similarity would hold {Q} x {n} values, at most 2^24 are handed back")
        plan_search(n, max(Q, 1), max_bytes)  # (its refusals, before anything touches the device)
        if self.image is None:
            raise RuntimeError("EmbeddingIndex.search: call .to(device) first (the device image has not been built)")
        dev = self.image.device
        with torch.cuda.device(dev):
            q = self._query_rows(queries, subtract, dev)
            scores = torch.full((Q, top_k), float("-inf"), dtype=torch.float32, device=dev)
            ids = torch.full((Q, top_k), -1, dtype=torch.int32, device=dev)
            sim = torch.empty((Q, n), dtype=torch.float32, device=dev) if return_similarity else None
            if Q == 0:
                return dict(scores=scores, ids=ids, **({"similarity": sim} if return_similarity else {}))
            img_q = ops.align_rows(q, None, cosine=True, b_side=False)
            exclude = torch.arange(Q, dtype=torch.int32, device=dev) if exclude_self else None
            for q0, q1, n0, cols, S in self._similarity_blocks(img_q, Q, max_bytes):
                ops.topk_merge(S, top_k, scores[q0:q1], ids[q0:q1], n_cols=cols, id_base=n0,
                               exclude=None if exclude is None else exclude[q0:q1], first=n0 == 0)
                if return_similarity:
                    sim[q0:q1, n0:n0 + cols] = S[:, :cols]
        out = dict(scores=scores, ids=ids)
        if return_similarity:
            out["similarity"] = sim
        return out


# ---- prefilter + aligner ----------------------------------------------------------------------------------------------------
def _embed_records(model, alphabet, records, layer, batch_tokens, varlen):
    """``align.embed`` through ``embed_layer``: (x fp32 [N, E], rows int32 [sum L], lengths) in record order."""
    from .align import residue_rows

    convert = alphabet.get_batch_converter()
    dev = model.embed_tokens.weight.device
    xs, rows, lengths, base = [], [None] * len(records), [0] * len(records), 0
    for batch in _batches(records, batch_tokens):
        _, _, tokens = convert([records[i] for i in batch])
        tokens = tokens.to(dev)
        rep = embed_layer(model, tokens, layer=layer, varlen=varlen)
        B, T, E = rep.shape
        with torch.cuda.device(dev):
            r, ln = residue_rows(model, tokens)
        xs.append(rep.reshape(B * T, E))
        first = 0
        for k, i in enumerate(batch):
            rows[i] = r[first:first + ln[k]] + base
            lengths[i] = ln[k]
            first += ln[k]
        base += B * T
    return torch.cat(xs, 0), torch.cat(rows).to(torch.int32).contiguous(), lengths


def plan_groups(query_tokens, hit_ids, target_tokens, batch_tokens):
    """Consecutive groups [q0, q1) of queries: the tokens of a group's queries plus those of the union of their hit targets
    stay within ``batch_tokens`` (a single query always forms a group).  ``hit_ids``: per query the database ids.  Pure."""
    groups, q0, union, used = [], 0, set(), 0
    for q, ids in enumerate(hit_ids):
        new = [t for t in dict.fromkeys(ids) if t not in union]
        add = int(query_tokens[q]) + sum(int(target_tokens[t]) for t in new)
        if q > q0 and used + add > batch_tokens:
            groups.append((q0, q))
            q0, union, used = q, set(), 0
            new = list(dict.fromkeys(ids))
            add = int(query_tokens[q]) + sum(int(target_tokens[t]) for t in new)
        union.update(new)
        used += add
    if q0 < len(hit_ids):
        groups.append((q0, len(hit_ids)))
    return groups


def search_and_align(model, alphabet, queries, index, top_k, align_top=None, batch_tokens=65536, varlen=True, search_bytes=2 << 30,
                     **align_kw):
    """The prefilter, then the aligner on the survivors.  ``queries``: records [(label, sequence)]; ``index`` holds its
    sequences and is on the device.  Every query's ``align_top`` (None: all ``top_k``) best hits are aligned by
    ``align.align_listed_rows`` (``align_kw``: mode, gap_open, gap_extend, enhance, paths, max_bytes, free_ends, hits_per_pair,
    min_hit_score — with K hits per pair every pair stands K times, with ``hit`` and ``valid``) on representation
    ``index.meta["layer"]``, queries in groups whose hit union fits ``batch_tokens``.  Returns the prefilter's ``scores`` /
    ``ids`` and ``alignment``: align's dict with ``pairs`` int32 [P, 2] = (query, database id), in query order, each query's
    hits by rank."""
    from . import align as A

    check_model(model, None, None, "search_and_align")
    index.check_model(model)
    if index.sequences is None:
        raise ValueError("search_and_align: the index holds no sequences (it was built with keep_sequences=False / --no-sequences)")
    if "pairs" in align_kw or "return_similarity" in align_kw or "similarity" in align_kw:
        raise ValueError("search_and_align: pairs, similarity and return_similarity are not arguments of this call")
    A.check_args(align_kw.get("mode", "global"), align_kw.get("gap_open", 1.0), align_kw.get("gap_extend", 0.1))
    _, n_hits, _ = A.check_hits(align_kw.get("mode", "global"), align_kw.get("free_ends"), align_kw.get("hits_per_pair", 1),
                                align_kw.get("min_hit_score", 0.0), align_kw.get("paths", True))
    queries = [(str(a), str(b)) for a, b in queries]
    layer = int(index.meta["layer"])
    qvec = pool_records(model, alphabet, queries, layer, batch_tokens, varlen)
    pre = index.search(qvec, top_k, max_bytes=search_bytes)
    keep = int(top_k) if align_top is None else min(int(align_top), int(top_k))
    if keep < 1:
        raise ValueError(f"search_and_align: align_top must be at least 1, got {align_top}")
    ids_host = pre["ids"][:, :keep].cpu().numpy()
    hit_ids = [[int(t) for t in row if t >= 0] for row in ids_host]
    groups = plan_groups([len(s) + 2 for _, s in queries], hit_ids, index.lengths + 2, batch_tokens)
    paths = align_kw.get("paths", True)
    parts = []
    for q0, q1 in groups:
        union = sorted({t for ids in hit_ids[q0:q1] for t in ids})
        if not union:
            continue
        slot = {t: i for i, t in enumerate(union)}
        xa, ra, la = _embed_records(model, alphabet, queries[q0:q1], layer, batch_tokens, varlen)
        xb, rb, lb = _embed_records(model, alphabet, [(index.labels[t], index.sequences[t]) for t in union], layer, batch_tokens, varlen)
        local = [(q - q0, slot[t]) for q in range(q0, q1) for t in hit_ids[q]]
        with torch.cuda.device(xa.device):
            out = A.align_listed_rows(xa, ra, la, xb, rb, lb, pairs=local, **align_kw)
        dev = out["pairs"].device
        out["pairs"] = torch.stack([out["pairs"][:, 0] + q0, torch.tensor(union, dtype=torch.int32, device=dev)[out["pairs"][:, 1].long()]], 1)
        parts.append(out)
    dev = pre["ids"].device
    if not parts:
        alignment = dict(pairs=torch.zeros((0, 2), dtype=torch.int32, device=dev), score=torch.zeros((0,), dtype=torch.float32, device=dev),
                         end=torch.zeros((0, 2), dtype=torch.int32, device=dev))
        if n_hits > 1:
            alignment.update(hit=torch.zeros((0,), dtype=torch.int32, device=dev), valid=torch.zeros((0,), dtype=torch.bool, device=dev))
    else:
        alignment = {k: torch.cat([p[k] for p in parts], 0) for k in ("pairs", "score", "end")}
        if paths:
            for k in ("start", "n_cols", "n_match", "cols"):
                alignment[k] = torch.cat([p[k] for p in parts], 0)
            nc = alignment["n_cols"].long()
            alignment["col_offsets"] = torch.cat([nc.new_zeros(1), nc.cumsum(0)])
        if n_hits > 1:
            for k in ("hit", "valid"):
                alignment[k] = torch.cat([p[k] for p in parts], 0)
    return dict(scores=pre["scores"], ids=pre["ids"], alignment=alignment)


# ---- text -------------------------------------------------------------------------------------------------------------------
TSV_HEADER = ("query", "target", "rank", "cosine")


def write_tsv(fh, hits, aligned=False, hit_column=False):
    """One line per hit: query, target, rank (1-based), cosine; with ``aligned`` the columns of ``align.write_tsv`` follow
    (score, score_per_residue, n_match, query_range, target_range and, with ``hit_column``, hit).  ``hits``: dicts with query, target, rank, cosine and, when
    aligned, what ``align.write_tsv`` reads."""
    import io

    from . import align as A

    tail = []
    if aligned:
        buf = io.StringIO()
        A.write_tsv(buf, hits, hit_column=hit_column)
        tail = [line.split("\t")[2:] for line in buf.getvalue().splitlines()]
    fh.write("\t".join(TSV_HEADER + (tuple(tail[0]) if aligned else ())) + "\n")
    for i, h in enumerate(hits):
        fh.write("\t".join([h["query"], h["target"], str(h["rank"]), f"{h['cosine']:.6f}"] + (tail[i + 1] if aligned else [])) + "\n")


# ---- command line -----------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    import argparse

    p = argparse.ArgumentParser(prog="python -m esm_amd.search", description="Protein search on pooled embeddings")
    sub = p.add_subparsers(dest="command", required=True)
    a = sub.add_parser("index", help="pool every protein of a FASTA file into an index")
    a.add_argument("--model-location", required=True, help="a model name or a checkpoint file (esm_amd.pretrained)")
    a.add_argument("--fasta", required=True, help="FASTA file of the database")
    a.add_argument("--layer", type=int, default=None, help="the representation to pool (default: the last)")
    a.add_argument("--no-sequences", action="store_true", help="do not keep the sequences (no --align on this index)")
    a.add_argument("--center", action="store_true", help="subtract the database mean (EmbeddingIndex.centered): for thresholds and clustering")
    a.add_argument("--output", required=True, help="the .npz of the index")
    a.add_argument("--batch-tokens", type=int, default=65536, help="tokens per forward batch")
    b = sub.add_parser("query", help="rank the database for every query; optionally align the best hits")
    b.add_argument("--model-location", required=True)
    b.add_argument("--index", required=True, help="the .npz written by the index command")
    b.add_argument("--query", required=True, help="FASTA file of the queries")
    b.add_argument("--top", type=int, required=True, help="hits per query (1 .. 1024)")
    b.add_argument("--align", action="store_true", help="align the hits (needs an index with sequences)")
    b.add_argument("--align-top", type=int, default=None, help="align only the M best hits of every query")
    b.add_argument("--mode", choices=("global", "local"), default=None, help="default: global")
    from .align import add_hit_options, resolve_hit_options
    add_hit_options(b, "target")
    b.add_argument("--gap-open", type=float, default=1.0)
    b.add_argument("--gap-extend", type=float, default=0.1)
    b.add_argument("--enhance", action="store_true", help="sharpen S by row and column z-scores")
    b.add_argument("--output", required=True, help="the TSV of hits")
    b.add_argument("--alignments", default=None, help="with --align: also write the gapped strings of every aligned hit")
    b.add_argument("--batch-tokens", type=int, default=65536)
    b.add_argument("--max-bytes", type=int, default=2 << 30, help="scratch of one similarity block")
    args = p.parse_args(argv)
    if args.command == "query":
        if not 1 <= args.top <= MAX_K:
            p.error(f"--top must be 1 .. {MAX_K}")
        if not args.align and (args.align_top is not None or args.alignments or args.enhance or args.free_ends is not None
                               or args.hits_per_target != 1):
            p.error("--align-top, --alignments, --enhance, --free-ends and --hits-per-target need --align")
        resolve_hit_options(p, args, "global")
        if args.align_top is not None and args.align_top < 1:
            p.error("--align-top must be at least 1")
    return args


def _records(path):
    from .fasta import read_fasta

    return [(label.split()[0], seq) for label, seq in read_fasta(path)]


def main(argv=None):
    args = parse_args(argv)
    from . import align as A
    from . import checkpoint as pretrained

    if args.command == "query":
        A.check_args(args.mode, args.gap_open, args.gap_extend)
        A.check_hits(args.mode, args.free_ends, args.hits_per_target)
        index = EmbeddingIndex.load(args.index)
        if args.align and index.sequences is None:
            raise ValueError("search: --align needs an index with sequences (it was written with --no-sequences)")
    model, alphabet = pretrained.load_model_and_alphabet(args.model_location)
    model = model.eval().cuda()
    if args.command == "index":
        layer = check_model(model, args.layer, None, "search")
        index = EmbeddingIndex.build(model, alphabet, _records(args.fasta), layer=layer, batch_tokens=args.batch_tokens,
                                     keep_sequences=not args.no_sequences, model_name=str(args.model_location))
        (index.centered() if args.center else index).save(args.output)
        return 0
    index.check_model(model)
    index.to(model.embed_tokens.weight.device)
    queries = _records(args.query)
    if args.align:
        out = search_and_align(model, alphabet, queries, index, args.top, align_top=args.align_top, batch_tokens=args.batch_tokens,
                               search_bytes=args.max_bytes, mode=args.mode, gap_open=args.gap_open, gap_extend=args.gap_extend,
                               enhance=args.enhance, free_ends=args.free_ends, hits_per_pair=args.hits_per_target)
    else:
        qvec = pool_records(model, alphabet, queries, int(index.meta["layer"]), args.batch_tokens)
        out = index.search(qvec, args.top, max_bytes=args.max_bytes)
    scores, ids = out["scores"].cpu().numpy(), out["ids"].cpu().numpy()
    al = {k: v.cpu().numpy() for k, v in out["alignment"].items()} if args.align else None
    K = args.hits_per_target if args.align else 1
    by_pair = {} if al is None else {(int(q), int(t)): p for p, (q, t) in list(enumerate(al["pairs"]))[::K]}  # a pair's first entry
    hits = []
    for q in range(len(queries)):
        for r in range(ids.shape[1]):
            t = int(ids[q, r])
            if t < 0:
                break
            h = dict(query=queries[q][0], target=index.labels[t], rank=r + 1, cosine=float(scores[q, r]))
            p = by_pair.get((q, t))
            if args.align:
                if p is None:  # beyond --align-top: ranked, not aligned
                    continue
                for k in range(K):  # of several hits per target the best is always listed, the others when they are valid
                    if k and not al["valid"][p + k]:
                        break
                    hk = dict(h)
                    hk.update(score=float(al["score"][p + k]), la=len(queries[q][1]), lb=int(index.lengths[t]),
                              n_match=int(al["n_match"][p + k]), start=al["start"][p + k].tolist(), end=al["end"][p + k].tolist(),
                              pair=p + k, q=q, t=t, hit=k)
                    hits.append(hk)
                continue
            hits.append(h)
    with open(args.output, "w") as fh:
        write_tsv(fh, hits, aligned=args.align, hit_column=K > 1)
    if args.alignments:
        with open(args.alignments, "w") as fh:
            for h in hits:
                p = h["pair"]
                cols = al["cols"][al["col_offsets"][p]:al["col_offsets"][p + 1]]
                top_s, bottom_s = A.alignment_strings(queries[h["q"]][1], index.sequences[h["t"]], cols)
                fh.write(f">{h['query']} {h['target']} score={h['score']:.4f}\n{top_s}\n{bottom_s}\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
