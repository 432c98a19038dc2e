"""The one loop behind masked, packed, windowed and MSA scoring: a list of copies of the input, per copy the rows to read
back, run in chunks that fill the GPU.  The callers (``esm_amd.scoring``, ``esm_amd.windows``, ``esm_amd.msa_scoring``) upload
their lists once and describe their copies as a ``Layout``; ``run_copies`` walks the chunks and collects the rows.  Nothing
here touches the engine or a model, so the loop runs on any device with any three callables."""
import torch

CHUNK_TOKENS = 65536  # tokens per forward call that fill the GPU (the batch budget of esm_amd.extract)


def copies_per_call(chunk, tokens_per_copy):
    """``chunk`` as given, or what fills the GPU where it is None."""
    if chunk is None:
        return max(1, CHUNK_TOKENS // tokens_per_copy)
    if chunk <= 0:
        raise ValueError("chunk must be positive")
    return chunk


def set_offsets(sets):
    """(offsets [n + 1], pos [total]) of a list of position lists: int64 on the host; set s owns
    ``pos[offsets[s] : offsets[s + 1]]``."""
    offsets = torch.zeros((len(sets) + 1,), dtype=torch.int64)
    offsets[1:] = torch.tensor([len(ps) for ps in sets], dtype=torch.int64).cumsum(0)
    return offsets, torch.tensor([p for ps in sets for p in ps], dtype=torch.int64)


def even_chunks(n_copies, chunk):
    """``Layout.chunks`` of copies that all have one width: ``chunk`` copies per call."""
    return lambda: ((lo, min(lo + chunk, n_copies)) for lo in range(0, n_copies, chunk))


def local_rows(sel_off, chunk, width, col, dev):
    """int32 on ``dev``: the flat row ``(i - lo) * width + col`` of every selected row inside the chunk ``lo : hi`` of its copy i,
    for ``even_chunks`` (lo = i - i % chunk).  ``sel_off`` [n + 1], ``col`` [total]: int64 on the host."""
    i = torch.repeat_interleave(torch.arange(sel_off.numel() - 1, dtype=torch.int64), sel_off[1:] - sel_off[:-1])
    return (i % chunk * width + col).to(torch.int32).to(dev)


class Layout:
    """How a list of copies runs: ``chunks()`` gives the ``(lo, hi)`` ranges of copies, one per call, ascending;
    ``build(lo, hi)`` the copies ``lo : hi``; ``forward(copies, sel, return_logits)`` the fp32 ``[n, V]`` log-probabilities of
    their rows ``sel`` (chunk-local flat indices), as a pair with the logits where ``return_logits``."""

    def __init__(self, chunks, build, forward):
        self.chunks, self.build, self.forward = chunks, build, forward


def run_copies(layout, n_copies, sel_off, sel_local, V, dev, return_logits=False):
    """The log-probabilities fp32 ``[total, V]`` of the selected rows of all copies, in the order of ``sel_local`` (and the
    logits).  Copy i owns ``sel_local[sel_off[i] : sel_off[i + 1]]``: ``sel_off`` int64 [n_copies + 1] on the host,
    ``sel_local`` int32 chunk-local flat rows on ``dev``.  A chunk that owns no row is not run."""
    if n_copies == 0 or sel_local.numel() == 0:
        empty = torch.empty((0, V), dtype=torch.float32, device=dev)
        return (empty, empty.clone()) if return_logits else empty
    lps, logits = [], []
    for lo, hi in layout.chunks():
        r0, r1 = int(sel_off[lo]), int(sel_off[hi])
        if r1 == r0:
            continue
        got = layout.forward(layout.build(lo, hi), sel_local[r0:r1], return_logits)
        lps.append(got[0] if return_logits else got)
        if return_logits:
            logits.append(got[1])
    lp = lps[0] if len(lps) == 1 else torch.cat(lps)
    return (lp, logits[0] if len(logits) == 1 else torch.cat(logits)) if return_logits else lp
