"""Embedding-based alignment of proteins: residue-by-residue similarity of two sets of per-residue representations, optionally
sharpened by row and column z-scores, then Needleman-Wunsch or Smith-Waterman with affine gaps — all on the device.

    out = model.align(tokens_a, tokens_b, layer=33, mode="local")          # every a against every b
    out = esm_amd.align_embeddings(reps_a, reps_b, pairs=[(0, 3), (1, 2)])  # on representations the caller holds
    out["pairs"]   int32 [P, 2]    (index in a, index in b)
    out["score"]   fp32  [P]
    out["end"]     int32 [P, 2]    the cell (i, j) the alignment ends in: it covers residues < i of a and < j of b
    with paths:    out["start"] int32 [P, 2], out["n_cols"], out["n_match"] int32 [P], out["col_offsets"] int64 [P + 1],
                   out["cols"] int32 [sum n_cols, 2]: per alignment column (i, j) a match, (i, -1) residue i of a against a gap,
                   (-1, j) residue j of b against a gap, ascending; pair p owns cols[col_offsets[p] : col_offsets[p + 1]]
    with return_similarity:  out["similarity"], a list of P views fp32 [La, Lb]
    with hits_per_pair = K > 1: every per-pair entry above has P K rows, pair p's hits k = 0 .. K - 1 one after the other
                   (``pairs`` repeats each pair K times), plus out["hit"] int32 [P K] (k) and out["valid"] bool [P K]

Definition (tests/_align_ref.py restates it in numpy, and the kernels reproduce that bit for bit given S).
Operand rows: ``similarity="cosine"``: u = x * r, r = float32(1 / sqrt(sum x^2)), the sum in fp64 in the order of
``esmk_op_align_rows`` (columns 4 t .. 4 t + 3, 4 t + 1024 .. ascending per thread t of 256, the 256 partial sums folded as
p[k] += p[k + s] for s = 128 .. 1); a zero row gives r = 0; ``"dot"``: u = x — rows with |x| >= 65504 overflow fp16, the split
below cannot hold them.  S[i][j] = <u_a[i], u_b[j]> runs on the 16-bit matrix rate with both operands split hi = fp16(u),
lo = fp16(u - hi) (the f16x3 form of the dense GEMM: hi hi + hi lo + lo hi, fp32 accumulation; the lo lo term is dropped).
``enhance=True``: per pair, S' = 0.5 ((S - mu_r[i]) / sigma_r[i] + (S - mu_c[j]) / sigma_c[j]) with the row's and the column's
mean and population deviation inside the pair's block (fp64 sums in ascending order, rounded once; 1 / sigma = 0 where sigma = 0).
Alignment: gap open o >= gap extend e >= 0; over (i, j) in 0 .. La x 0 .. Lb, H[0][0] = 0, E[i][0] = F[0][j] = -inf:
    E[i][j] = max(H[i][j-1] - o, E[i][j-1] - e)     F[i][j] = max(H[i-1][j] - o, F[i-1][j] - e)     D = S[i-1][j-1] + H[i-1][j-1]
    H[i][j] = the first of maximal value among [stop = 0 (local only), D, F[i][j], E[i][j]]
A gap of k residues costs o + (k - 1) e.  ``mode="global"``: the score is H[La][Lb]; ``mode="local"``: the largest H, ending in
the first such cell in row-major order, the walk back ending at the first stop; nothing above 0: score 0, an empty alignment.
The defaults o = 1.0, e = 0.1 are this project's choice for cosine similarities in [-1, 1]; they are not tuned on any benchmark.

Free end gaps (``free_ends=``, global mode only; tests/_align_free_ref.py restates them).  A mask of four bits: 1 ``a_start``,
2 ``a_end``, 4 ``b_start``, 8 ``b_end`` — leading / trailing residues of that side cost nothing.  ``"b"`` = b_start | b_end aligns
a end to end inside b (a domain in a long target), ``"a"`` the converse, ``"both"`` all four (overlap / dovetail); an iterable of
the four names or an int 0 .. 15 is taken as it stands.  Only the stop candidate on the borders and the end cell change:
a_start: H[i][0] = 0; b_start: H[0][j] = 0 (choice "stop"; E and F on the borders are unchanged); the end cell is the largest H
among (La, Lb), the cells (i, Lb), i >= 1, with a_end and the cells (La, j), j >= 1, with b_end — ties go to the lower row, then
the lower column; the walk back stops on row 0 with b_start and on column 0 with a_start and emits the gaps otherwise.

Several hits per pair (``hits_per_pair=K``, 1 .. 16; Waterman-Eggert in its plainest form): after hit k is traced, S[i][j] of
every MATCH column (i, j) of its path is set to -inf in the pair's block of S, and the DP and the walk run again.  Only match
cells are excluded: a later path may cross an earlier one through a gap.  A pair's scores are non-increasing in k and the match
cells of its hits are disjoint; ``valid`` = ``score > min_hit_score`` and ``n_match >= 1``, so a pair's valid hits form a prefix.
All rounds of a block run on one stream and reuse one traceback buffer; S is overwritten, so ``return_similarity`` is refused.

Not built: the MSA Transformer, windows (``window=``).  The prefilter on pooled embeddings is esm_amd/search.py.
"""
import numpy as np
import torch

MAX_LEN = 8192
MODES = {"global": 0, "local": 1}
FREE_END_BITS = {"a_start": 1, "a_end": 2, "b_start": 4, "b_end": 8}
FREE_END_NAMES = {"a": 3, "b": 12, "both": 15}
MAX_HITS = 16


# ---- arguments ------------------------------------------------------------------------------------------------------------
def check_args(mode="global", gap_open=1.0, gap_extend=0.1, similarity="cosine", len_a=(), len_b=()):
    """Raises on what the kernels would refuse, before any GPU call; returns (mode code, o, e)."""
    if mode not in MODES:
        raise ValueError(f"align: mode must be 'global' or 'local', got {mode!r} (free end gaps: mode='global' with free_ends=)")
    if similarity not in ("cosine", "dot"):
        raise ValueError(f"align: similarity must be 'cosine' or 'dot', got {similarity!r}")
    o, e = float(np.float32(gap_open)), float(np.float32(gap_extend))
    if not (np.isfinite(o) and np.isfinite(e)) or e < 0 or o < 0:
        raise ValueError(f"align: gap penalties must be finite and >= 0, got gap_open = {gap_open}, gap_extend = {gap_extend}")
    if e > o:
        raise ValueError(f"align: gap_extend = {gap_extend} exceeds gap_open = {gap_open}")
    for side, lens in (("a", len_a), ("b", len_b)):
        for k, n in enumerate(lens):
            if not 1 <= int(n) <= MAX_LEN:
                raise ValueError(f"align: sequence {k} of side {side} has {int(n)} residues, 1 .. {MAX_LEN} are supported")
    return MODES[mode], o, e


def parse_free_ends(free_ends):
    """The four-bit mask of ``free_ends``: None -> 0; "a" / "b" / "both"; an iterable of a_start, a_end, b_start, b_end; an int."""
    if free_ends is None:
        return 0
    if isinstance(free_ends, (bool, float)):
        raise ValueError(f"align: free_ends must be None, 'a', 'b', 'both', names of {sorted(FREE_END_BITS)} or 0 .. 15, got {free_ends!r}")
    if isinstance(free_ends, (int, np.integer)):
        if not 0 <= int(free_ends) <= 15:
            raise ValueError(f"align: free_ends = {int(free_ends)} is outside 0 .. 15")
        return int(free_ends)
    if isinstance(free_ends, str):
        if free_ends in FREE_END_NAMES:
            return FREE_END_NAMES[free_ends]
        free_ends = (free_ends,)
    mask = 0
    try:
        names = list(free_ends)
    except TypeError:
        names = [free_ends]
    for name in names:
        if not isinstance(name, str) or name not in FREE_END_BITS:
            raise ValueError(f"align: free_ends must be None, 'a', 'b', 'both', names of {sorted(FREE_END_BITS)} or 0 .. 15, got {name!r}")
        mask |= FREE_END_BITS[name]
    return mask


def check_hits(mode="global", free_ends=None, hits_per_pair=1, min_hit_score=0.0, paths=True, return_similarity=False):
    """Raises on the combinations that are refused, before any GPU call; returns (mask, K, min_hit_score)."""
    mask = parse_free_ends(free_ends)
    if mask and mode == "local":
        raise ValueError("align: free_ends applies to mode='global' only; local mode has all four ends free already")
    if isinstance(hits_per_pair, bool) or not isinstance(hits_per_pair, (int, np.integer)) or not 1 <= int(hits_per_pair) <= MAX_HITS:
        raise ValueError(f"align: hits_per_pair must be an int 1 .. {MAX_HITS}, got {hits_per_pair!r}")
    K = int(hits_per_pair)
    m = float(min_hit_score)
    if np.isnan(m):
        raise ValueError("align: min_hit_score is NaN")
    if K > 1 and not paths:
        raise ValueError("align: hits_per_pair > 1 needs paths=True (the next hit is found by masking the path of the last)")
    if K > 1 and return_similarity:
        raise ValueError("align: hits_per_pair > 1 overwrites S, return_similarity=True is refused")
    return mask, K, m


def check_pairs(pairs, n_a, n_b):
    """int64 [P, 2] on the host: every (a, b) when ``pairs`` is None; listed pairs must be in range and distinct."""
    if pairs is None:
        ia, ib = np.meshgrid(np.arange(n_a, dtype=np.int64), np.arange(n_b, dtype=np.int64), indexing="ij")
        return np.stack([ia.ravel(), ib.ravel()], 1)
    if isinstance(pairs, torch.Tensor):
        pairs = pairs.detach().cpu().numpy()
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pairs) and (pairs.min() < 0 or pairs[:, 0].max() >= n_a or pairs[:, 1].max() >= n_b):
        raise ValueError(f"align: pairs must index 0 .. {n_a - 1} on side a and 0 .. {n_b - 1} on side b")
    if len(np.unique(pairs[:, 0] * max(n_b, 1) + pairs[:, 1])) != len(pairs):
        raise ValueError("align: a pair is listed twice")
    return pairs


# ---- blocks ---------------------------------------------------------------------------------------------------------------
def _up(n, m):
    return (n + m - 1) // m * m


def block_bytes(len_a, len_b, pairs, E, paths=True, enhance=False, panel=512):
    """The scratch one (a-chunk x b-chunk) block needs: S fp32 [Ma, Nb], the two fp16 images [Ma + Nb, 3 Ep], the traceback
    bytes of the listed pairs (La x Lb rounded up to 16) and the kernels' workspaces.  Ma = the a side's residues; Nb = the b
    side's, every sequence rounded up to 8 and the sum to 64.  ``pairs`` [P, 2] index into ``len_a`` / ``len_b``."""
    len_a, len_b = np.asarray(len_a, dtype=np.int64), np.asarray(len_b, dtype=np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    Ep = _up(int(E), 64)
    Ma = int(len_a.sum())
    Nb = _up(int(((len_b + 7) // 8 * 8).sum()), 64)
    total = 4 * Ma * Nb + 6 * Ep * (Ma + Nb)
    P = len(pairs)
    la, lb = len_a[pairs[:, 0]], len_b[pairs[:, 1]]
    if paths:
        total += int((la * ((lb + 15) // 16 * 16)).sum())
    if P and int(lb.max()) > panel:
        total += min(P, 16384) * 8 * (int(la.max()) + 1)
    if P and enhance:
        total += min(P, 1024) * 8 * int(lb.max())
    return total


def plan_blocks(len_a, len_b, pairs, E, max_bytes, paths=True, enhance=False, panel=512):
    """The blocks of an alignment call: a list of (a0, a1, b0, b1, idx) — sequences a0 .. a1 - 1 of side a against b0 .. b1 - 1 of
    side b, ``idx`` the positions in ``pairs`` of the listed pairs that fall into the block.  Every listed pair is in exactly one
    block; sequences are never cut; every block's ``block_bytes`` is at most ``max_bytes``; a rectangle without a listed pair
    gives no block.  A rectangle over the budget is halved (by sequence count) along the side that holds more residues; a
    single pair over the budget is a ValueError.  Pure: it depends on its arguments alone."""
    len_a, len_b = np.asarray(len_a, dtype=np.int64), np.asarray(len_b, dtype=np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    blocks = []

    def rec(a0, a1, b0, b1, idx):
        if len(idx) == 0:
            return
        local = pairs[idx] - np.array([a0, b0])
        need = block_bytes(len_a[a0:a1], len_b[b0:b1], local, E, paths, enhance, panel)
        if need <= max_bytes:
            blocks.append((a0, a1, b0, b1, idx))
            return
        if a1 - a0 == 1 and b1 - b0 == 1:
            raise ValueError(f"align: max_bytes = {max_bytes} does not hold the pair ({a0}, {b0}) of {int(len_a[a0])} x "
                             f"{int(len_b[b0])} residues ({need} bytes are needed)")
        split_a = a1 - a0 > 1 and (b1 - b0 == 1 or len_a[a0:a1].sum() >= len_b[b0:b1].sum())
        if split_a:
            m = (a0 + a1) // 2
            rec(a0, m, b0, b1, idx[pairs[idx, 0] < m])
            rec(m, a1, b0, b1, idx[pairs[idx, 0] >= m])
        else:
            m = (b0 + b1) // 2
            rec(a0, a1, b0, m, idx[pairs[idx, 1] < m])
            rec(a0, a1, m, b1, idx[pairs[idx, 1] >= m])

    rec(0, len(len_a), 0, len(len_b), np.arange(len(pairs), dtype=np.int64))
    return blocks


def pair_table(a_off, la, b_off, lb):
    """int64 [P, 5] on the host, the table the kernels read: (first row of a in S, La, first column of b in S, Lb, offset of the
    pair's traceback bytes), and the bytes all pairs need.  A pair's bytes are La rows of Lb rounded up to 16."""
    la, lb = np.asarray(la, dtype=np.int64), np.asarray(lb, dtype=np.int64)
    size = la * ((lb + 15) // 16 * 16)
    off = np.concatenate([[0], np.cumsum(size)])
    table = np.stack([np.asarray(a_off, dtype=np.int64), la, np.asarray(b_off, dtype=np.int64), lb, off[:-1]], 1)
    return np.ascontiguousarray(table), int(off[-1])


# ---- the call -------------------------------------------------------------------------------------------------------------
def _flat(reps, what):
    """(flat fp32 [sum L, E] on the device, lengths on the host) of a list of [L_i, E] tensors or a pair (flat, lengths)."""
    if isinstance(reps, tuple) and len(reps) == 2 and isinstance(reps[0], torch.Tensor) and reps[0].dim() == 2 \
            and not (isinstance(reps[1], torch.Tensor) and reps[1].dim() == 2):
        flat, lengths = reps
        lengths = [int(n) for n in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        if sum(lengths) != flat.shape[0]:
            raise ValueError(f"align: the lengths of side {what} sum to {sum(lengths)}, the flat tensor has {flat.shape[0]} rows")
    else:
        reps = list(reps)
        if not reps or any(not isinstance(r, torch.Tensor) or r.dim() != 2 for r in reps):
            raise ValueError(f"align: side {what} must be a non-empty list of [L, E] tensors or a pair (flat [sum L, E], lengths)")
        lengths = [int(r.shape[0]) for r in reps]
        if len({int(r.shape[1]) for r in reps}) != 1:
            raise ValueError(f"align: the tensors of side {what} differ in E")
        flat = torch.cat([r.to(torch.float32) for r in reps], 0)
    return flat, lengths


def align_embeddings(reps_a, reps_b, pairs=None, mode="global", gap_open=1.0, gap_extend=0.1, similarity="cosine", enhance=False,
                     paths=True, return_similarity=False, max_bytes=4 << 30, free_ends=None, hits_per_pair=1, min_hit_score=0.0):
    """Aligns per-residue representations (module docstring).  ``reps_a`` / ``reps_b``: a list of fp32 [L_i, E] device tensors, or
    a pair (flat [sum L, E], lengths); <cls>, <eos> and <pad> must not be rows.  ``pairs``: [P, 2] (index in a, index in b),
    None: every pair.  Returns the dict of device tensors the module docstring lists; ``paths=False`` scores only (no traceback
    byte is allocated or written, and ``start``, ``n_cols``, ``n_match``, ``cols`` are absent).  The work is cut into blocks of
    whole sequences whose scratch fits ``max_bytes`` (``plan_blocks``); the column slots of the paths (8 (La + Lb) bytes per
    pair and hit) and, with ``return_similarity``, the kept S blocks are outputs and stand outside that budget.  ``free_ends``,
    ``hits_per_pair``, ``min_hit_score``: the module docstring."""
    flat_a, len_a = _flat(reps_a, "a")
    flat_b, len_b = _flat(reps_b, "b")
    check_args(mode, gap_open, gap_extend, similarity, len_a, len_b)
    check_hits(mode, free_ends, hits_per_pair, min_hit_score, paths, return_similarity)
    if flat_a.shape[1] != flat_b.shape[1]:
        raise ValueError(f"align: side a has E = {flat_a.shape[1]}, side b has E = {flat_b.shape[1]}")
    if not flat_a.is_cuda or not flat_b.is_cuda:
        raise RuntimeError("align runs only on an MI355X (ROCm) device; there is no CPU fallback")
    with torch.cuda.device(flat_a.device):
        return align_listed_rows(flat_a, None, len_a, flat_b, None, len_b, pairs=pairs, mode=mode, gap_open=gap_open, gap_extend=gap_extend,
                          similarity=similarity, enhance=enhance, paths=paths, return_similarity=return_similarity,
                          max_bytes=max_bytes, free_ends=free_ends, hits_per_pair=hits_per_pair, min_hit_score=min_hit_score)


def align_listed_rows(x_a, rows_a, len_a, x_b, rows_b, len_b, pairs=None, mode="global", gap_open=1.0, gap_extend=0.1, similarity="cosine",
               enhance=False, paths=True, return_similarity=False, max_bytes=4 << 30, free_ends=None, hits_per_pair=1,
               min_hit_score=0.0):
    """``align_embeddings`` on rows picked out of larger matrices: x_* fp32 [N, E] on the device, rows_* int32 [sum L] the residue
    rows of the side's sequences one after the other (None: rows 0 .. sum L - 1), len_* the lengths on the host."""
    from . import _native as N
    from . import ops

    mode_code, o, e = check_args(mode, gap_open, gap_extend, similarity, len_a, len_b)
    mask, K, min_hit_score = check_hits(mode, free_ends, hits_per_pair, min_hit_score, paths, return_similarity)
    E = int(x_a.shape[1])
    if E % 4 != 0:
        raise ValueError(f"align: E = {E} must be a multiple of 4")
    pairs = check_pairs(pairs, len(len_a), len(len_b))
    len_a, len_b = np.asarray(len_a, dtype=np.int64), np.asarray(len_b, dtype=np.int64)
    panel = ops.align_panel()
    blocks = plan_blocks(len_a, len_b, pairs, E, max_bytes, paths=paths, enhance=enhance, panel=panel)
    dev = x_a.device
    x_a, x_b = x_a.to(torch.float32).contiguous(), x_b.to(torch.float32).contiguous()
    if rows_a is None:
        rows_a = torch.arange(int(len_a.sum()), dtype=torch.int32, device=dev)
    if rows_b is None:
        rows_b = torch.arange(int(len_b.sum()), dtype=torch.int32, device=dev)
    off_a = np.concatenate([[0], np.cumsum(len_a)])
    off_b = np.concatenate([[0], np.cumsum(len_b)])
    P = len(pairs) * K  # entry p K + k: hit k of pair p
    la_all, lb_all = len_a[pairs[:, 0]], len_b[pairs[:, 1]]
    score = torch.zeros((P,), dtype=torch.float32, device=dev)
    end = torch.zeros((P, 2), dtype=torch.int32, device=dev)
    out = dict(pairs=torch.from_numpy(np.repeat(pairs, K, axis=0).astype(np.int32)).to(dev), score=score, end=end)
    if paths:
        cap = np.repeat(la_all + lb_all, K)
        slot_np = np.concatenate([[0], np.cumsum(cap)])
        slot = torch.from_numpy(slot_np[:-1].copy()).to(dev)
        slots = torch.empty((max(int(slot_np[-1]), 1), 2), dtype=torch.int32, device=dev)
        start = torch.zeros((P, 2), dtype=torch.int32, device=dev)
        n_cols = torch.zeros((P,), dtype=torch.int32, device=dev)
        n_match = torch.zeros((P,), dtype=torch.int32, device=dev)
    sims = [None] * len(pairs)
    cosine = similarity == "cosine"
    for a0, a1, b0, b1, idx in blocks:
        # side a: the chunk's residue rows as they stand; side b: every sequence starts at a multiple of 8 columns of S
        # (zero rows in between), the whole rounded up to 64
        ra = rows_a[int(off_a[a0]):int(off_a[a1])].contiguous()
        lb8 = (len_b[b0:b1] + 7) // 8 * 8
        col_b = np.concatenate([[0], np.cumsum(lb8)])
        Nb = _up(int(col_b[-1]), 64)
        src = np.full((Nb,), -1, dtype=np.int64)
        for k in range(b1 - b0):
            src[col_b[k]:col_b[k] + len_b[b0 + k]] = np.arange(off_b[b0 + k], off_b[b0 + k + 1])
        src = torch.from_numpy(src).to(dev)
        rb = torch.where(src >= 0, rows_b[src.clamp(min=0)], torch.full_like(src, -1, dtype=torch.int32)).to(torch.int32).contiguous()
        img_a = ops.align_rows(x_a, ra, cosine=cosine, b_side=False)
        img_b = ops.align_rows(x_b, rb, cosine=cosine, b_side=True)
        S = ops.linear(img_a, img_b, None, N.EPI_STORE_F32)
        pa, pb = pairs[idx, 0], pairs[idx, 1]
        table_np, tb_bytes = pair_table(off_a[pa] - off_a[a0], len_a[pa], col_b[pb - b0], len_b[pb])
        table = torch.from_numpy(table_np).to(dev)
        max_la, max_lb = int(len_a[pa].max()), int(len_b[pb].max())
        if enhance:
            ops.align_enhance(S, table, max_lb)
        tb = torch.empty((max(tb_bytes, 16),), dtype=torch.uint8, device=dev) if paths else None
        didx = torch.from_numpy(idx).to(dev)
        for k in range(K):
            # round k: the DP on S as the walks of the rounds before left it; every round but the last masks its paths in S
            r = ops.align_dp(S, table, mode_code, o, e, max_la, max_lb, want_traceback=paths, tb=tb, free_ends=mask)
            dk = didx if K == 1 else didx * K + k
            score.index_copy_(0, dk, r["score"])
            end.index_copy_(0, dk, r["end"])
            if paths:
                t = ops.align_traceback(table, mode_code, r["end"], tb, slot[dk].contiguous(), slots, free_ends=mask,
                                        S_mask=S if k + 1 < K else None)
                start.index_copy_(0, dk, t["start"])
                n_cols.index_copy_(0, dk, t["n_cols"])
                n_match.index_copy_(0, dk, t["n_match"])
        if return_similarity:
            for k, p in enumerate(idx):
                ao, bo = int(table_np[k, 0]), int(table_np[k, 2])
                sims[int(p)] = S[ao:ao + int(table_np[k, 1]), bo:bo + int(table_np[k, 3])]
    if paths:
        # the columns stand at the back of each pair's slot: gather them into one ragged tensor
        nc = n_cols.long()
        col_offsets = torch.cat([nc.new_zeros(1), nc.cumsum(0)])
        total = int(col_offsets[-1])
        first = slot + torch.from_numpy(cap).to(dev) - nc
        pos = torch.repeat_interleave(first - col_offsets[:-1], nc, output_size=total) + torch.arange(total, device=dev)
        out.update(start=start, n_cols=n_cols, n_match=n_match, col_offsets=col_offsets, cols=slots[pos])
    if K > 1:
        out["hit"] = torch.arange(K, dtype=torch.int32, device=dev).repeat(len(pairs))
        out["valid"] = (score > min_hit_score) & (n_match >= 1)
    if return_similarity:
        out["similarity"] = sims
    return out


def residue_rows(model, tokens):
    """(rows int32 [sum L] into the [B * T] token grid, lengths on the host) of the residues of ``tokens`` [B, T]: <cls>, <eos>
    and <pad> are no rows."""
    from .sae import scored_rows

    B, T = tokens.shape
    rows = scored_rows(model, tokens, "residues")
    lengths = torch.bincount(rows[:, 0].long(), minlength=B).cpu().tolist()
    return (rows[:, 0] * T + rows[:, 1]).to(torch.int32).contiguous(), lengths


def check_model(model, layer, window=None):
    from .msa_transformer import MSATransformer

    if isinstance(model, MSATransformer):
        raise NotImplementedError("align is built for ESM-2, ESM-1b / ESM-1v and ESM-1; not for the MSA Transformer")
    if window is not None:
        raise NotImplementedError("align: windows (window=) are not built")
    layer = int(model.num_layers) if layer is None else int(layer)
    if not 0 <= layer <= int(model.num_layers):
        raise ValueError(f"align: layer {layer} is outside 0 .. {int(model.num_layers)}")
    return layer


def align(model, tokens_a, tokens_b, layer=None, varlen=False, window=None, **kw):
    """``model.align``: the forward of each side for representation ``layer`` (None: the last), then ``align_embeddings`` on the
    residue rows — sequence k of a side is row k of its token batch.  ``varlen=True`` runs ``forward_varlen``."""
    layer = check_model(model, layer, window)
    check_args(kw.get("mode", "global"), kw.get("gap_open", 1.0), kw.get("gap_extend", 0.1), kw.get("similarity", "cosine"))
    check_hits(kw.get("mode", "global"), kw.get("free_ends"), kw.get("hits_per_pair", 1), kw.get("min_hit_score", 0.0),
               kw.get("paths", True), kw.get("return_similarity", False))
    for tokens in (tokens_a, tokens_b):
        assert tokens.ndim == 2
        if tokens.shape[1] - 2 > MAX_LEN:  # the longest row a batch of this width can hold
            n = int(tokens.ne(model.padding_idx).sum(1).max())
            if n - 2 > MAX_LEN:
                raise ValueError(f"align: a sequence of {n - 2} residues, 1 .. {MAX_LEN} are supported")
    fwd = model.forward_varlen if varlen else model.forward
    sides = []
    for tokens in (tokens_a, tokens_b):
        rep = fwd(tokens, repr_layers=[layer])["representations"][layer]
        B, T, E = rep.shape
        with torch.cuda.device(rep.device):
            rows, lengths = residue_rows(model, tokens.to(rep.device))
        sides.append((rep.reshape(B * T, E), rows, lengths))
    (xa, ra, la), (xb, rb, lb) = sides
    with torch.cuda.device(xa.device):
        return align_listed_rows(xa, ra, la, xb, rb, lb, **kw)


# ---- text -----------------------------------------------------------------------------------------------------------------
def alignment_strings(seq_a, seq_b, cols):
    """The two gapped strings of an alignment: ``cols`` [n, 2] as ``align_embeddings`` returns them (a tensor, an array or a
    list); column (i, j) shows seq_a[i] over seq_b[j], -1 shows '-'."""
    if isinstance(cols, torch.Tensor):
        cols = cols.detach().cpu().numpy()
    cols = np.asarray(cols, dtype=np.int64).reshape(-1, 2)
    top = "".join("-" if i < 0 else seq_a[i] for i in cols[:, 0])
    bottom = "".join("-" if j < 0 else seq_b[j] for j in cols[:, 1])
    return top, bottom


TSV_HEADER = ("query", "target", "score", "score_per_residue", "n_match", "query_range", "target_range")


def write_tsv(fh, hits, hit_column=False):
    """One line per hit: query, target, score, score / min(La, Lb), n_match and the two ranges (1-based, inclusive; '-' for an
    empty alignment or an untraced hit).  ``hits``: dicts with query, target, score, la, lb and, when traced, n_match, start, end.
    ``hit_column`` (several hits per target): a last column ``hit``, the dict's ``hit`` (0: the best path of the pair)."""
    fh.write("\t".join(TSV_HEADER + (("hit",) if hit_column else ())) + "\n")
    for h in hits:
        traced = h.get("start") is not None
        rng = ["-", "-"]
        if traced:
            for k in (0, 1):
                if h["end"][k] > h["start"][k]:
                    rng[k] = f"{h['start'][k] + 1}-{h['end'][k]}"
        fh.write("\t".join([h["query"], h["target"], f"{h['score']:.4f}", f"{h['score'] / min(h['la'], h['lb']):.4f}",
                            str(h["n_match"]) if traced else "-", rng[0], rng[1]] + ([str(h.get("hit", 0))] if hit_column else []))
                 + "\n")


# ---- command line ---------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    import argparse

    p = argparse.ArgumentParser(prog="python -m esm_amd.align",
                                description="Embedding-based alignment of every query against every target")
    p.add_argument("--model-location", required=True, help="a model name or a checkpoint file (esm_amd.pretrained)")
    p.add_argument("--query", required=True, help="FASTA file of the queries")
    p.add_argument("--target", required=True, help="FASTA file of the targets")
    p.add_argument("--layer", type=int, default=None, help="the representation to align (default: the last)")
    p.add_argument("--mode", choices=("global", "local"), default=None, help="default: global")
    add_hit_options(p, "target")
    p.add_argument("--gap-open", type=float, default=1.0)
    p.add_argument("--gap-extend", type=float, default=0.1)
    p.add_argument("--similarity", choices=("cosine", "dot"), default="cosine")
    p.add_argument("--enhance", action="store_true", help="sharpen S by row and column z-scores")
    p.add_argument("--top", type=int, default=None, help="trace only the N best targets of every query")
    p.add_argument("--output", required=True, help="the TSV of hits")
    p.add_argument("--alignments", default=None, help="also write the gapped strings of every traced hit")
    p.add_argument("--batch-tokens", type=int, default=16384, help="tokens per forward batch")
    p.add_argument("--max-bytes", type=int, default=4 << 30)
    args = p.parse_args(argv)
    resolve_hit_options(p, args, "global")
    return args


def add_hit_options(p, what):
    """The two options the command lines share: --free-ends and --hits-per-<what>."""
    p.add_argument("--free-ends", choices=("a", "b", "both"), default=None,
                   help="free end gaps on that side (b: the query end to end inside the target); implies --mode global")
    p.add_argument(f"--hits-per-{what}", type=int, default=1, dest="hits_per_target",
                   help=f"up to K non-overlapping paths per {what} (1 .. {MAX_HITS})")


def resolve_hit_options(p, args, default_mode):
    """--free-ends implies --mode global and refuses --mode local; without it --mode defaults to ``default_mode``."""
    if args.free_ends is not None:
        if args.mode == "local":
            p.error("--free-ends needs --mode global (local mode has every end free)")
        args.mode = "global"
    elif args.mode is None:
        args.mode = default_mode
    if not 1 <= args.hits_per_target <= MAX_HITS:
        p.error(f"--hits-per-target must be 1 .. {MAX_HITS}")


def embed(model, alphabet, records, layer, batch_tokens=16384):
    """(x fp32 [N, E], rows int32 [sum L], lengths) of the residues of ``records`` [(label, sequence)], in record order: batches
    of similar lengths, the representations kept on the device."""
    convert = alphabet.get_batch_converter()
    order = sorted(range(len(records)), key=lambda i: len(records[i][1]))
    xs, rows, lengths, base = [], [None] * len(records), [0] * len(records), 0
    lo = 0
    while lo < len(order):
        hi, longest = lo, 0
        while hi < len(order) and (hi == lo or max(longest, len(records[order[hi]][1]) + 2) * (hi + 1 - lo) <= batch_tokens):
            longest = max(longest, len(records[order[hi]][1]) + 2)
            hi += 1
        _, _, tokens = convert([records[i] for i in order[lo:hi]])
        tokens = tokens.to(next(model.parameters()).device)
        rep = model.forward(tokens, repr_layers=[layer])["representations"][layer]
        B, T, E = rep.shape
        with torch.cuda.device(rep.device):
            r, ln = residue_rows(model, tokens)
        xs.append(rep.reshape(B * T, E).to(torch.float32))
        first = 0
        for k, i in enumerate(order[lo:hi]):
            rows[i] = r[first:first + ln[k]] + base
            lengths[i] = ln[k]
            first += ln[k]
        base += B * T
        lo = hi
    return torch.cat(xs, 0), torch.cat(rows).to(torch.int32).contiguous(), lengths


def main(argv=None):
    args = parse_args(argv)
    check_args(args.mode, args.gap_open, args.gap_extend, args.similarity)
    check_hits(args.mode, args.free_ends, args.hits_per_target)
    from . import checkpoint as pretrained
    from .fasta import read_fasta

    model, alphabet = pretrained.load_model_and_alphabet(args.model_location)
    model = model.eval().cuda()
    layer = check_model(model, args.layer)
    queries = [(label.split()[0], seq) for label, seq in read_fasta(args.query)]
    targets = [(label.split()[0], seq) for label, seq in read_fasta(args.target)]
    xa, ra, la = embed(model, alphabet, queries, layer, args.batch_tokens)
    xb, rb, lb = embed(model, alphabet, targets, layer, args.batch_tokens)
    kw = dict(mode=args.mode, gap_open=args.gap_open, gap_extend=args.gap_extend, similarity=args.similarity, enhance=args.enhance,
              max_bytes=args.max_bytes, free_ends=args.free_ends)
    K = args.hits_per_target
    with torch.cuda.device(xa.device):
        if args.top is None:
            out = align_listed_rows(xa, ra, la, xb, rb, lb, hits_per_pair=K, **kw)
        else:
            # every pair is scored without traceback bytes; only the best targets of each query are traced, in a second pass
            scores = align_listed_rows(xa, ra, la, xb, rb, lb, paths=False, **kw)["score"].reshape(len(queries), len(targets))
            top = scores.topk(min(args.top, len(targets)), dim=1).indices.sort(dim=1).values.cpu().numpy()
            picked = [(q, int(t)) for q in range(len(queries)) for t in top[q]]
            out = align_listed_rows(xa, ra, la, xb, rb, lb, pairs=picked, hits_per_pair=K, **kw)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    # of several hits per target the best is always listed, the others when they are valid
    keep = [p for p in range(len(host["pairs"])) if K == 1 or host["hit"][p] == 0 or host["valid"][p]]
    hits = []
    for p in keep:
        q, t = host["pairs"][p]
        hits.append(dict(query=queries[q][0], target=targets[t][0], score=float(host["score"][p]), la=la[q], lb=lb[t],
                         n_match=int(host["n_match"][p]), start=host["start"][p].tolist(), end=host["end"][p].tolist(),
                         hit=int(host["hit"][p]) if K > 1 else 0))
    with open(args.output, "w") as fh:
        write_tsv(fh, hits, hit_column=K > 1)
    if args.alignments:
        with open(args.alignments, "w") as fh:
            for p in keep:
                q, t = host["pairs"][p]
                cols = host["cols"][host["col_offsets"][p]:host["col_offsets"][p + 1]]
                top_s, bottom_s = alignment_strings(queries[q][1], targets[t][1], cols)
                fh.write(f">{queries[q][0]} {targets[t][0]} score={host['score'][p]:.4f}\n{top_s}\n{bottom_s}\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
