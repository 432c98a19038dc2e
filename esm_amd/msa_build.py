"""Query-anchored MSAs from search hits: the step between ``search_and_align`` and the MSA Transformer, on the device.

    index = esm_amd.EmbeddingIndex.load("db.npz").to("cuda")
    built = model.build_msa(alphabet, ("query", sequence), index, top_k=1024, depth=256)     # a BuiltMSA
    built.msa, built.labels, built.hit_ids, built.scores, built.stats                          # uint8 [R, Lq] on the device, ...
    built.write_a3m("query.a3m"); msa_model.msa_score_variants(msa_alphabet, built.records(), ["A42G"])

    python -m esm_amd.build_msa --model-location M --index db.npz --query Q.fasta --output-dir DIR [--summary OUT.tsv] ...

``search_and_align(..., paths=True)`` returns, per hit, the alignment columns (i, j) against the query — everything a row of an
a3m file is made of.  What hhblits and hhfilter do after their search is done here (tests/_msa_build_ref.py restates every step
in numpy and plain loops, and the device path reproduces that exactly):
1. One ``search_and_align`` call for all queries.  ``align_kw`` defaults to ``mode="local", enhance=True``: raw cosines of
   unrelated residues are all positive, so a local alignment on them spans everything.  These defaults and the gap penalties
   (``align``'s o = 1.0, e = 0.1) are this project's choice; they are not tuned on any benchmark.  ``free_ends="b"`` (with
   ``mode="global"``) aligns the whole query inside each hit instead.  ``hits_per_pair=K`` > 1: every VALID hit of a target
   (``align``'s ``valid``) is a candidate row of its own, with the target's ``hit_id`` and, from the second on, the label
   ``<label>|hit=<k>`` — a repeat protein gives one row per copy of the query it holds.
2. Per query, its hits' sequences go to the device as one blob and ``esmk_op_msa_project`` writes one row of Lq bytes per hit:
   '-' everywhere, the hit's letter in every matched query column; and per hit six integers (``STATS``).  The unaligned ends of
   a hit and its insertions are not in the row (an a3m's match states).
3. The row filter, on the int32 stats on the device: a hit stays when ``n_match >= 1``, ``n_match >= min_coverage * Lq`` and
   ``n_ident >= min_query_identity * n_match`` — each product in fp64, the integers converted exactly.
4. The redundancy filter at ``max_identity`` (hhfilter's -id; None skips it).  The rows are ranked: the query, then the hits by
   alignment score descending, ties to the prefilter's rank, then to the lower hit number k.  The gap-aware identity of two rows is same / both
   (``esmk_op_msa_pair_identity``: ``both`` the columns in which neither has a gap, ``same`` those in which they agree; 0 when
   ``both < min_overlap``).  Walk the rows by rank: a row that no earlier kept row has covered is kept and covers every later
   row whose identity to it is at least ``max_identity`` — the greedy cover of esm_amd/cluster.py on the thresholded identity
   matrix (``esmk_op_range_rows``, ``cluster.greedy_rounds``).  A hit identical to the query is covered by the query and drops
   out: this is the only handling of self hits.  Rows that failed step 3 rank behind all others, where they cover nothing that
   counts, and are dropped afterwards; so the walk needs no compaction in between.
5. More than ``depth`` rows left: ``subsample_indices(rows, depth, subsample, theta, seed)``, which keeps the query; "first"
   keeps the best ranked.
Between 2 and 5 the host reads the number of kept rows and the undecided counts of ``greedy_rounds``, nothing else.

Not built: one command that loads both models and chains into ``predict_msa``; iterative (profile) search rounds; a projection
launch that serves several queries.
"""
import numpy as np
import torch

STATS = ("n_match", "n_ident", "n_ins", "n_del", "first", "last")
GAP = ord("-")
A3M_DELETED = "abcdefghijklmnopqrstuvwxyz.*"  # what read_msa deletes from a row
MAX_ROWS = 1024       # msa_scoring._check_msa: the MSA position embedding
MAX_POSITIONS = 1024  # and the learned positions, <cls> included


# ---- arguments ------------------------------------------------------------------------------------------------------------
def _unit(name, v):
    v = float(v)
    if not 0.0 <= v <= 1.0:  # (false for NaN)
        raise ValueError(f"build_msas: {name} must be in [0, 1], got {v}")
    return v


def check_args(index, depth=None, min_coverage=0.5, max_identity=0.9, min_query_identity=0.0, min_overlap=8, subsample="first",
               align_kw=None):
    """The ValueErrors that need no device.  Returns (depth, min_coverage, max_identity, min_query_identity, min_overlap, the
    aligner's keywords with this module's defaults)."""
    from .msa_select import STRATEGIES

    if getattr(index, "sequences", None) is None:
        raise ValueError("build_msas: the index holds no sequences (it was built with keep_sequences=False / --no-sequences)")
    if depth is not None:
        if int(depth) != depth or int(depth) < 1:
            raise ValueError(f"build_msas: depth must be a positive integer or None, got {depth!r}")
        depth = int(depth)
    min_coverage = _unit("min_coverage", min_coverage)
    min_query_identity = _unit("min_query_identity", min_query_identity)
    if max_identity is not None:
        max_identity = _unit("max_identity", max_identity)
    if int(min_overlap) != min_overlap or int(min_overlap) < 1:
        raise ValueError(f"build_msas: min_overlap must be an integer >= 1, got {min_overlap!r}")
    if subsample not in STRATEGIES:
        raise ValueError(f"build_msas: unknown subsampling strategy {subsample!r} (one of {', '.join(STRATEGIES)})")
    align_kw = dict(align_kw or {})
    for k in ("paths", "pairs", "similarity", "return_similarity"):
        if k in align_kw:
            raise ValueError(f"build_msas: {k} is not an argument of this call")
    kw = dict(mode="local", enhance=True)
    kw.update(align_kw)
    if "free_ends" in kw or "hits_per_pair" in kw or "min_hit_score" in kw:
        from .align import check_hits

        check_hits(kw["mode"], kw.get("free_ends"), kw.get("hits_per_pair", 1), kw.get("min_hit_score", 0.0))
    return depth, min_coverage, max_identity, min_query_identity, int(min_overlap), kw


def rank_order(scores, passed):
    """int64 [N] on the device of ``scores``: the rows in rank order.  Row 0 (the query) first; then the hits that ``passed``
    (bool [N]) by ``scores`` (fp32 [N], row 0 unused) descending, ties to the lower row (the prefilter's rank); then the others,
    ordered likewise.  Two stable sorts."""
    by_score = torch.sort(scores[1:], descending=True, stable=True).indices
    failed = (~passed[1:])[by_score].to(torch.int8)
    hits = by_score[torch.sort(failed, stable=True).indices] + 1
    return torch.cat([hits.new_zeros(1), hits])


def identity_blocks(n, max_bytes):
    """The row blocks [(i0, nb)] of the identity matrix of n rows: fp32 [nb, n rounded up to 4] within ``max_bytes``, whole
    tiles of 64 rows where more than one fits.  Pure."""
    per_row = 4 * ((n + 3) // 4 * 4)
    nb = max(1, min(n, int(max_bytes) // per_row))
    if nb < n and nb >= 64:
        nb -= nb % 64
    return [(i0, min(nb, n - i0)) for i0 in range(0, n, nb)]


# ---- the text -------------------------------------------------------------------------------------------------------------
def a3m_row(row, seq, cols, insertions=True):
    """One a3m row of a hit: ``row`` its match states (Lq characters, '-' for a deletion), ``seq`` its residues, ``cols`` its
    path [(i, j)].  Between the first and the last match the path is followed — a match gives the row's letter, (i, -1) a '-',
    (-1, j) the residue j in lower case (``insertions``) — and '-' stands for the query columns on either side: unaligned
    ends are not written.  A path whose query columns do not ascend one by one is a ValueError."""
    Lq = len(row)
    cols = [(int(i), int(j)) for i, j in cols]
    at = [c for c, (i, j) in enumerate(cols) if 0 <= i < Lq and 0 <= j < len(seq)]
    if not at:
        return "-" * Lq
    first, last = cols[at[0]][0], cols[at[-1]][0]
    out, states = ["-" * first], first
    for i, j in cols[at[0]:at[-1] + 1]:
        if 0 <= i < Lq and (j == -1 or 0 <= j < len(seq)):
            if i != states:
                raise ValueError(f"a3m: the path names query column {i} where column {states} is due")
            out.append(row[i] if j >= 0 else "-")
            states += 1
        elif i == -1 and 0 <= j < len(seq) and insertions:
            out.append(seq[j].lower())
    if states != last + 1:
        raise ValueError("a3m: the path does not end in its last match")
    out.append("-" * (Lq - states))
    return "".join(out)


def token_table(alphabet):
    """int64 [256]: the token of every byte value, ``alphabet.get_idx(chr(b))`` (<unk> for what the alphabet does not hold)."""
    return torch.tensor([alphabet.get_idx(chr(b)) for b in range(256)], dtype=torch.int64)


class BuiltMSA:
    """One query's alignment.  ``msa`` uint8 [R, Lq] on the device, the query first, then the kept hits in rank order — a valid
    input to ``encode_msa`` / ``msa_neff`` / ``subsample_msa`` as it stands; ``labels`` [R]; ``hit_ids`` int32 [R] (database ids,
    -1 for the query), ``scores`` fp32 [R] (alignment scores, +inf for the query) and ``stats`` int32 [R, 6] (``STATS``; the
    query's row is the query against itself) on the device.  ``counts``: hits found, rows after the row filter (coverage and
    query identity), after the redundancy filter, and kept, the query included from the second on."""

    def __init__(self, msa, labels, hit_ids, scores, stats, counts=None, paths=None):
        self.msa, self.labels, self.hit_ids, self.scores, self.stats = msa, list(labels), hit_ids, scores, stats
        self.counts = dict(counts or {})
        self._paths = paths  # (cols on the device, the kept hits' (lo, hi) into it, their sequences)
        self._rows = None

    def __len__(self):
        return int(self.msa.shape[0])

    def _row_strings(self):
        if self._rows is None:
            host = self.msa.cpu().numpy()
            self._rows = [bytes(r).decode("latin-1") for r in host]
        return self._rows

    def records(self):
        """``[(label, row string)]``, what ``msa_score_variants`` takes and ``read_msa`` returns."""
        return list(zip(self.labels, self._row_strings()))

    def tokens(self, msa_alphabet, max_rows=MAX_ROWS, max_positions=MAX_POSITIONS):
        """int64 [1, R, Lq + 1] on the device: the rows through a 256-entry table of ``msa_alphabet.get_idx``, <cls> in front.
        More rows or columns than the MSA Transformer takes (``msa_scoring._check_msa``) is a ValueError."""
        R, Lq = self.msa.shape
        if R > max_rows:
            raise ValueError(f"BuiltMSA.tokens: {R} rows, the MSA Transformer takes at most {max_rows}; build with depth={max_rows}")
        if Lq + 1 > max_positions:
            raise ValueError(f"BuiltMSA.tokens: {Lq + 1} columns with <cls>, the MSA Transformer takes at most {max_positions}")
        dev = self.msa.device
        body = token_table(msa_alphabet).to(dev)[self.msa.long()]
        cls = torch.full((R, 1), int(msa_alphabet.cls_idx), dtype=torch.int64, device=dev)
        return torch.cat([cls, body], 1).unsqueeze(0)

    def a3m_lines(self, insertions=True):
        rows = self._row_strings()
        for k, row in enumerate(rows):
            bad = sorted(set(row) & set(A3M_DELETED))
            if bad:
                raise ValueError(f"a3m: row {k} ({self.labels[k]}) holds {bad[0]!r}, which an a3m reader takes for an insertion")
        lines = [f">{self.labels[0]}", rows[0]]
        if len(rows) > 1:
            if self._paths is None:
                raise ValueError("a3m: this BuiltMSA does not hold its alignment paths")
            cols, ranges, seqs = self._paths
            lo, hi = min(r[0] for r in ranges), max(r[1] for r in ranges)
            host = cols[lo:hi].cpu().numpy()  # one copy: the kept rows' columns
            for k in range(1, len(rows)):
                a, b = ranges[k - 1]
                lines += [f">{self.labels[k]}", a3m_row(rows[k], seqs[k - 1], host[a - lo:b - lo], insertions)]
        return lines

    def write_a3m(self, path, insertions=True):
        """The alignment as an a3m file: the query row first; per hit its match letters as stored and '-' for deletions; with
        ``insertions`` the hit's inserted residues inside the aligned span in lower case.  ``read_msa(path)`` gives
        ``records()`` back."""
        text = "\n".join(self.a3m_lines(insertions)) + "\n"
        with open(path, "w") as fh:
            fh.write(text)


# ---- the pipeline ---------------------------------------------------------------------------------------------------------
def _bytes_to(text, dev):
    try:
        blob = text.encode("ascii")
    except UnicodeEncodeError as e:
        raise ValueError(f"build_msas: not an ASCII sequence ({e})") from None
    if not blob:
        return torch.empty((0,), dtype=torch.uint8, device=dev)
    return torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)


def redundancy_keep(M, Lq, order, max_identity, min_overlap, max_bytes):
    """bool [N] on the device: the rows of ``M`` uint8 [N, ld] the greedy cover keeps when the rows are walked in ``order``
    (module docstring, 4).  No host read but ``greedy_rounds``' counters."""
    from . import ops
    from .cluster import COVERED, ROUNDS_PER_READ, greedy_rounds

    n = M.shape[0]
    dev = M.device
    rank = torch.empty((n,), dtype=torch.int64, device=dev)
    rank[order] = torch.arange(n, device=dev)
    rank = rank.to(torch.int32)
    if n == 1:
        return torch.ones((1,), dtype=torch.bool, device=dev)
    blocks = identity_blocks(n, max_bytes)
    ldS = (n + 3) // 4 * 4
    scratch = torch.empty((blocks[0][1], ldS), dtype=torch.float32, device=dev)
    exclude = torch.arange(n, dtype=torch.int32, device=dev)
    counts = torch.zeros((n,), dtype=torch.int64, device=dev)
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    for i0, nb in blocks:
        S = ops.msa_pair_identity(M, L=Lq, gap=GAP, min_overlap=min_overlap, i0=i0, nb=nb, out=scratch)
        ops.range_rows(S, max_identity, counts=counts[i0:i0 + nb], n_cols=n, exclude=exclude[i0:i0 + nb], n_rows=nb)
    torch.cumsum(counts, 0, out=offsets[1:])
    cap = n * (n - 1)  # every pair: no read of the total (n <= 1025 behind a search)
    ids = torch.empty((cap,), dtype=torch.int32, device=dev)
    scores = torch.empty((cap,), dtype=torch.float32, device=dev)
    cursor = offsets[:-1].clone()
    for i0, nb in blocks:
        if len(blocks) > 1:  # (a single block still stands in the scratch)
            S = ops.msa_pair_identity(M, L=Lq, gap=GAP, min_overlap=min_overlap, i0=i0, nb=nb, out=scratch)
        ops.range_rows(S, max_identity, offsets=offsets[i0:i0 + nb + 1], cursor=cursor[i0:i0 + nb], ids=ids, scores=scores, n_cols=n,
                       exclude=exclude[i0:i0 + nb], n_rows=nb)
    state, _ = greedy_rounds(offsets, ids, rank, lanes=16, max_rounds=n + ROUNDS_PER_READ)
    return state != COVERED


def msa_from_hits(query, index, hit_ids, scores, cols, col_offsets, depth=None, min_coverage=0.5, max_identity=0.9,
                  min_query_identity=0.0, min_overlap=8, subsample="first", theta=0.2, seed=0, max_bytes=2 << 30, hit_numbers=None):
    """Steps 2 to 5 for one query: ``query`` (label, sequence); ``hit_ids`` the database ids of its P hits in the prefilter's
    order (host ints), ``scores`` fp32 [P] their alignment scores, ``cols`` / ``col_offsets`` (int64 [P + 1], indexing ``cols``)
    their paths, on the device.  ``hit_numbers`` (several hits per target): per hit its number k among its target's hits, a
    target's hits standing one after the other; k >= 1 is labelled ``<label>|hit=<k>``.  Returns a ``BuiltMSA``."""
    from . import ops
    from .msa_select import subsample_indices

    label, qseq = str(query[0]), str(query[1])
    dev = col_offsets.device
    P, Lq = len(hit_ids), len(qseq)
    if Lq < 1:
        raise ValueError(f"build_msas: query {label!r} is empty")
    with torch.cuda.device(dev):
        # 2. the projection
        seqs = [index.sequences[t] for t in hit_ids]
        lens = np.array([len(s) for s in seqs], dtype=np.int64)
        ld = (Lq + 3) // 4 * 4
        M = torch.zeros((P + 1, ld), dtype=torch.uint8, device=dev)
        M[0, :Lq] = _bytes_to(qseq, dev)
        stats = torch.zeros((P + 1, 6), dtype=torch.int32, device=dev)
        stats[0] = torch.tensor([Lq, Lq, 0, 0, 0, Lq - 1], dtype=torch.int32).to(dev)
        if P:
            seq_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)).to(dev)
            seq_len = torch.from_numpy(lens.astype(np.int32)).to(dev)
            ops.msa_project(cols, col_offsets.contiguous(), _bytes_to("".join(seqs), dev), seq_off, seq_len, M[0, :Lq].contiguous(), ld=ld,
                            msa=M[1:], stats=stats[1:])
        # 3. the row filter
        nm, ni = stats[:, 0].double(), stats[:, 1].double()
        covered = (stats[:, 0] >= 1) & (nm >= min_coverage * float(Lq))
        passed = covered & (ni >= min_query_identity * nm)
        all_scores = torch.cat([torch.full((1,), float("inf"), dtype=torch.float32, device=dev), scores.to(torch.float32)])
        order = rank_order(all_scores, passed)
        # 4. the redundancy filter
        kept = passed
        if max_identity is not None and P:
            kept = passed & redundancy_keep(M, Lq, order, max_identity, min_overlap, max_bytes)
        sel = order[kept[order]]  # the kept rows in rank order; its length is the one read
        n_nonredundant = int(sel.numel())
        # 5. the depth
        if depth is not None and n_nonredundant > depth:
            pick = subsample_indices(M[sel][:, :Lq].contiguous(), depth, strategy=subsample, theta=theta, seed=seed)
            sel = sel[torch.tensor(pick, dtype=torch.int64).to(dev)]
        ids_dev = torch.cat([torch.full((1,), -1, dtype=torch.int32), torch.tensor(list(hit_ids), dtype=torch.int32)]).to(dev)
        sel_host = sel.cpu().tolist()
        offs = col_offsets.cpu().tolist() if P else [0]
        kept_hits = [r - 1 for r in sel_host[1:]]
        counts = dict(hits=P, after_row_filter=passed.sum(), after_redundancy_filter=n_nonredundant, kept=len(sel_host))
        names = [index.labels[t] for t in hit_ids]
        if hit_numbers is not None:
            names = [f"{name}|hit={int(k)}" if k else name for name, k in zip(names, hit_numbers)]
        return BuiltMSA(M[sel][:, :Lq].contiguous(), [label] + [names[h] for h in kept_hits], ids_dev[sel], all_scores[sel],
                        stats[sel], counts=counts, paths=(cols, [(offs[h], offs[h + 1]) for h in kept_hits], [seqs[h] for h in kept_hits]))


def msas_from_alignment(queries, index, alignment, **kw):
    """Steps 2 to 5 for every query on the ``alignment`` dict of one ``search_and_align(..., paths=True)`` call.  An alignment
    with several hits per pair (``hit``, ``valid``) is cut down to its valid entries first: one read of their number."""
    queries = [(str(a), str(b)) for a, b in queries]
    hit_numbers = None
    if "valid" in alignment:
        keep = alignment["valid"].nonzero().flatten()
        nc = alignment["n_cols"].long()
        nk = nc[keep]
        offsets = torch.cat([nk.new_zeros(1), nk.cumsum(0)])
        total = int(offsets[-1])
        pos = torch.repeat_interleave((nc.cumsum(0) - nc)[keep] - offsets[:-1], nk, output_size=total) + torch.arange(total, device=nk.device)
        hit_numbers = alignment["hit"][keep].cpu().tolist()
        alignment = dict(pairs=alignment["pairs"][keep], score=alignment["score"][keep], cols=alignment["cols"][pos], col_offsets=offsets)
    pairs = alignment["pairs"].cpu().numpy()
    bounds = np.searchsorted(pairs[:, 0], np.arange(len(queries) + 1))  # (pairs are in query order)
    dev = alignment["pairs"].device
    out = []
    for q, query in enumerate(queries):
        p0, p1 = int(bounds[q]), int(bounds[q + 1])
        if p1 > p0:
            cols, col_offsets = alignment["cols"], alignment["col_offsets"][p0:p1 + 1]
        else:
            cols, col_offsets = torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int64, device=dev)
        out.append(msa_from_hits(query, index, [int(t) for t in pairs[p0:p1, 1]], alignment["score"][p0:p1], cols, col_offsets,
                                 hit_numbers=None if hit_numbers is None else hit_numbers[p0:p1], **kw))
    return out


def build_msas(model, alphabet, queries, index, top_k=1024, depth=None, min_coverage=0.5, max_identity=0.9, min_query_identity=0.0,
               min_overlap=8, subsample="first", theta=0.2, seed=0, batch_tokens=65536, max_bytes=2 << 30, **align_kw):
    """One ``BuiltMSA`` per query (module docstring).  ``queries``: records [(label, sequence)]; ``index`` holds its sequences
    and is on the device; ``top_k`` hits per query go to the aligner.  ``align_kw`` (mode, gap_open, gap_extend, enhance,
    max_bytes, free_ends, hits_per_pair, min_hit_score) defaults to ``mode="local", enhance=True``: these and the gap penalties are this project's choice and are not
    tuned on any benchmark.  ``max_bytes`` bounds one block of the identity matrix."""
    from .search import check_model, search_and_align

    check_model(model, None, None, "build_msas")
    depth, min_coverage, max_identity, min_query_identity, min_overlap, kw = check_args(
        index, depth, min_coverage, max_identity, min_query_identity, min_overlap, subsample, align_kw)
    queries = [(str(a), str(b)) for a, b in queries]
    out = search_and_align(model, alphabet, queries, index, top_k, batch_tokens=batch_tokens, paths=True, **kw)
    return msas_from_alignment(queries, index, out["alignment"], depth=depth, min_coverage=min_coverage, max_identity=max_identity,
                               min_query_identity=min_query_identity, min_overlap=min_overlap, subsample=subsample, theta=theta,
                               seed=seed, max_bytes=max_bytes)


def build_msa(model, alphabet, query, index, **kw):
    """``build_msas`` for one query (label, sequence): its ``BuiltMSA``."""
    return build_msas(model, alphabet, [query], index, **kw)[0]


# ---- command line ---------------------------------------------------------------------------------------------------------
SUMMARY_HEADER = ("query", "hits", "after_coverage", "after_identity", "written", "neff")


def parse_args(argv=None):
    import argparse

    from .msa_select import STRATEGIES

    p = argparse.ArgumentParser(prog="python -m esm_amd.build_msa",
                                description="Query-anchored a3m alignments from the hits of an embedding search")
    p.add_argument("--model-location", required=True, help="a model name or a checkpoint file (esm_amd.pretrained)")
    p.add_argument("--index", required=True, help="the .npz written by python -m esm_amd.search index (with sequences)")
    p.add_argument("--query", required=True, help="FASTA file of the queries")
    p.add_argument("--output-dir", required=True, help="receives <label>.a3m per query")
    p.add_argument("--top", type=int, default=1024, help="hits per query that are aligned (1 .. 1024)")
    p.add_argument("--depth", type=int, default=None, help="at most this many rows, the query included")
    p.add_argument("--min-coverage", type=float, default=0.5, help="matched share of the query's columns a hit needs")
    p.add_argument("--max-identity", type=float, default=0.9, help="pairwise identity at which a better ranked row covers another")
    p.add_argument("--min-query-identity", type=float, default=0.0, help="identical share of a hit's matches it needs")
    p.add_argument("--subsample", choices=[s for s in STRATEGIES if s != "greedy-min"], default="first")
    p.add_argument("--mode", choices=("local", "global"), default=None, help="default: local")
    from .align import add_hit_options, resolve_hit_options
    add_hit_options(p, "target")
    p.add_argument("--gap-open", type=float, default=1.0)
    p.add_argument("--gap-extend", type=float, default=0.1)
    p.add_argument("--no-enhance", action="store_true", help="align on raw cosines (default: row and column z-scores)")
    p.add_argument("--no-insertions", action="store_true", help="do not write inserted residues (lower case)")
    p.add_argument("--summary", default=None, help="a TSV: per query the hits found, the rows after the coverage (row) filter, after "
                                                   "the identity (redundancy) filter, the rows written, and Neff")
    p.add_argument("--batch-tokens", type=int, default=65536)
    args = p.parse_args(argv)
    resolve_hit_options(p, args, "local")
    if not 1 <= args.top <= 1024:
        p.error("--top must be 1 .. 1024")
    if args.depth is not None and args.depth < 1:
        p.error("--depth must be at least 1")
    for name in ("min_coverage", "max_identity", "min_query_identity"):
        v = getattr(args, name)
        if not 0.0 <= v <= 1.0:
            p.error(f"--{name.replace('_', '-')} must be in [0, 1]")
    return args


def file_name(label):
    """The file name of a query's a3m: its label with every character that is not a letter, a digit, '.', '_' or '-' replaced."""
    safe = "".join(ch if ch.isalnum() or ch in "._-" else "_" for ch in label)
    return (safe.lstrip(".") or "query") + ".a3m"


def main(argv=None):
    args = parse_args(argv)
    import os

    from . import align as A
    from . import checkpoint as pretrained
    from .msa_select import msa_neff
    from .search import EmbeddingIndex, _records

    A.check_args(args.mode, args.gap_open, args.gap_extend)
    index = EmbeddingIndex.load(args.index)
    check_args(index)
    model, alphabet = pretrained.load_model_and_alphabet(args.model_location)
    model = model.eval().cuda()
    index.check_model(model)
    index.to(model.embed_tokens.weight.device)
    queries = _records(args.query)
    names = [file_name(label) for label, _ in queries]
    if len(set(names)) != len(names):
        raise ValueError("build_msa: two queries would be written to the same file")
    built = build_msas(model, alphabet, queries, index, top_k=args.top, depth=args.depth, min_coverage=args.min_coverage,
                       max_identity=args.max_identity, min_query_identity=args.min_query_identity, subsample=args.subsample,
                       batch_tokens=args.batch_tokens, mode=args.mode, gap_open=args.gap_open, gap_extend=args.gap_extend,
                       enhance=not args.no_enhance, free_ends=args.free_ends, hits_per_pair=args.hits_per_target)
    os.makedirs(args.output_dir, exist_ok=True)
    for name, b in zip(names, built):
        b.write_a3m(os.path.join(args.output_dir, name), insertions=not args.no_insertions)
    if args.summary:
        with open(args.summary, "w") as fh:
            fh.write("\t".join(SUMMARY_HEADER) + "\n")
            for (label, _), b in zip(queries, built):
                c = b.counts
                fh.write("\t".join([label, str(int(c["hits"])), str(int(c["after_row_filter"])), str(int(c["after_redundancy_filter"])),
                                    str(int(c["kept"])), f"{msa_neff(b.msa):.3f}"]) + "\n")
    return 0
