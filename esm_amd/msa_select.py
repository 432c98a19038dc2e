"""Choosing the rows of an MSA on the MI355X: the step between an alignment of 10^4 .. 10^5 records and the at most 1024 rows
the MSA Transformer takes.  Two recipes of the reference's workflow, both on the device (csrc/msa_select.hip):

greedy     the contact notebook's ``greedy_select`` (examples/contact_prediction.ipynb, "Subsampling MSA"): start from the query
           and repeatedly add the row with the largest summed Hamming distance to the rows picked so far ("greedy-min": the
           smallest).  The engine compares INTEGER sums of mismatch counts, ties to the lowest row.  The notebook compares float
           means of count / L: where L is not a power of two its rounding breaks exact ties its own way, so the two can choose
           different rows there; where count / L is exact (L = 64) they choose the same rows.
weighted   the subsamples of the ESM-1v paper (Meier et al. 2021): sequence weights ``w_i = 1 / #{j : d_H(i, j) < theta}``, rows
           drawn without replacement with probability proportional to w.  The draw is an exponential race: row i gets the key
           ``-log(u_i) / w_i`` from a Philox counter addressed by (seed, subsample, i), and the rows of the smallest keys win.
           The same (seed, subsample) gives the same rows in any process and on any device.  "uniform": all weights one.

The neighbour counts behind the weights are the N^2 L part: ``esmk_op_msa_neighbor_counts``.  A row is a neighbour when its
mismatch count is below ``theta * L`` (that product in fp64); a gap is a symbol like any other, as the notebook's
``cdist(..., "hamming")`` on the byte view treats it.  Row 0, the query, is always kept, and the picked rows come back in
ascending file order.  Strategy "first" is ``msa[:num_seqs]`` and touches no GPU.
"""
import math

import torch

STRATEGIES = ("first", "greedy", "greedy-min", "weighted", "uniform")


def max_mismatch(theta, L):
    """The largest integer m with ``float(m) < theta * L``, the product taken in fp64; -1 when there is none.  Row j is a
    neighbour of row i when they differ in at most that many columns."""
    p = float(theta) * float(L)
    if not p > 0.0:
        return -1
    m = min(int(math.ceil(p)) - 1, int(L))
    while m < L and float(m + 1) < p:
        m += 1
    while m >= 0 and not float(m) < p:
        m -= 1
    return m


def _is_records(msa):
    return not torch.is_tensor(msa)


def _n_rows(msa):
    if torch.is_tensor(msa):
        if msa.dim() == 3 and msa.shape[0] == 1:
            return msa.shape[1]
        if msa.dim() != 2:
            raise ValueError(f"msa: [(label, sequence)], a token tensor [R, C] or a byte matrix [N, L], got shape {tuple(msa.shape)}")
        return msa.shape[0]
    return len(msa)


def encode_msa(msa, device="cuda"):
    """The device byte matrix uint8 ``[N, L]`` the kernels compare.

    ``[(label, aligned sequence)]``  the ASCII bytes of the sequences; rows of different lengths raise ValueError
    token tensor ``[R, C]`` / ``[1, R, C]`` of the MSA alphabet (any integer dtype but uint8): the leading <cls> column dropped
    uint8 ``[N, L]``  taken as it is (moved to the device)"""
    if torch.is_tensor(msa):
        if msa.dim() == 3 and msa.shape[0] == 1:
            msa = msa[0]
        if msa.dim() != 2:
            raise ValueError(f"msa: a token tensor [R, C] or a byte matrix [N, L], got shape {tuple(msa.shape)}")
        if msa.dtype == torch.uint8:
            out = msa
        else:
            if msa.shape[1] < 2:
                raise ValueError("msa: a token tensor needs a column behind <cls>")
            out = msa[:, 1:].to(torch.uint8)
        if out.shape[0] < 1 or out.shape[1] < 1:
            raise ValueError("msa is empty")
        return out.to(device).contiguous()
    rows = [seq for _, seq in msa]
    if not rows:
        raise ValueError("msa is empty")
    L = len(rows[0])
    if L == 0:
        raise ValueError("msa: the sequences are empty")
    for i, seq in enumerate(rows):
        if len(seq) != L:
            raise ValueError(f"msa: row {i} has {len(seq)} columns, row 0 has {L}: the rows of an alignment have one length")
    try:
        blob = "".join(rows).encode("ascii")
    except UnicodeEncodeError as e:
        raise ValueError(f"msa: not an ASCII alignment ({e})") from None
    host = torch.frombuffer(bytearray(blob), dtype=torch.uint8).view(len(rows), L)
    return host.to(device).contiguous()


def msa_mismatches(msa, rows):
    """int32 ``[len(rows), N]`` on the device: the number of columns in which row ``rows[q]`` differs from every row."""
    from . import ops

    enc = encode_msa(msa)
    if torch.is_tensor(rows):
        q = rows.to(device=enc.device, dtype=torch.int32).contiguous().view(-1)
    else:
        q = torch.tensor([int(r) for r in rows], dtype=torch.int32).to(enc.device)
    if q.numel() == 0:
        return torch.empty((0, enc.shape[0]), dtype=torch.int32, device=enc.device)
    return ops.msa_mismatch_rows(enc, q)


def msa_neighbor_counts(msa, theta=0.2):
    """int32 ``[N]`` on the device: for every row the number of rows (itself included) whose Hamming distance to it is below
    ``theta``, i.e. that differ from it in fewer than ``theta * L`` columns."""
    from . import ops

    enc = encode_msa(msa)
    return ops.msa_neighbor_counts(enc, max_mismatch(theta, enc.shape[1]))


def msa_sequence_weights(msa, theta=0.2):
    """fp64 ``[N]`` on the device: ``1 / msa_neighbor_counts`` (a row without a neighbour, theta <= 0, weighs +inf)."""
    return 1.0 / msa_neighbor_counts(msa, theta).to(torch.float64)


def msa_neff(msa, theta=0.2):
    """The effective number of sequences: the sum of the sequence weights, a Python float."""
    return float(msa_sequence_weights(msa, theta).sum())


def _check_num(num_seqs):
    if int(num_seqs) != num_seqs or int(num_seqs) < 1:
        raise ValueError(f"num_seqs {num_seqs!r} must be a positive integer")
    return int(num_seqs)


def subsample_indices(msa, num_seqs, strategy="greedy", theta=0.2, seed=0, subsample=0, counts=None):
    """The rows a subsample of ``num_seqs`` rows keeps: a list of ascending row indices that starts with the query, row 0.
    Every row when the MSA has no more than ``num_seqs``.  ``strategy``: see the module.  ``counts``: the result of
    ``msa_neighbor_counts(msa, theta)`` when the caller already has it ("weighted" only)."""
    from . import ops

    if strategy not in STRATEGIES:
        raise ValueError(f"unknown subsampling strategy {strategy!r} (one of {', '.join(STRATEGIES)})")
    num_seqs = _check_num(num_seqs)
    n = _n_rows(msa)
    if n <= num_seqs:
        return list(range(n))
    if strategy == "first":
        return list(range(num_seqs))
    if strategy in ("greedy", "greedy-min"):
        sel = ops.msa_greedy_select(encode_msa(msa), num_seqs, first=0, mode=0 if strategy == "greedy" else 1)
        return sorted(sel.tolist())
    if strategy == "weighted":
        if counts is None:
            counts = msa_neighbor_counts(msa, theta)
        keys = ops.msa_race_keys(n, seed, subsample, counts=counts)
    else:
        keys = ops.msa_race_keys(n, seed, subsample)
    keys[0] = -1.0  # the query: in front of every key of the race (those are positive)
    rank = ops.rank_keys(keys)
    return (rank < num_seqs).nonzero().view(-1).tolist()


def subsample_msa(msa, num_seqs, strategy="greedy", theta=0.2, seed=0, subsample=0, counts=None):
    """``msa`` restricted to the rows of ``subsample_indices``: a list of records for a list, the indexed rows for a tensor
    (of ``[R, C]`` or ``[1, R, C]``)."""
    idx = subsample_indices(msa, num_seqs, strategy, theta, seed, subsample, counts)
    if _is_records(msa):
        return [msa[i] for i in idx]
    at = torch.tensor(idx, dtype=torch.int64, device=msa.device)
    return msa.index_select(msa.dim() - 2, at)
