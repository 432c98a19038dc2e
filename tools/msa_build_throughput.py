#!/usr/bin/env python
"""From aligned hits to an MSA (esm_amd/msa_build.py): (i) the stages behind ``search_and_align`` — projection, row filter,
redundancy filter — on the device (``msa_build.msa_from_hits``) against the loop a user writes today: ``cols`` to the host, a
Python projection, the pairwise identity in numpy in chunks of rows on 16 threads, the sequential filter; both must keep the
same rows, which is asserted; (ii) ``esmk_op_msa_pair_identity`` on a large matrix against ``esmk_op_msa_neighbor_counts`` on
the same matrix in the same process, by device events: the existing kernel of the same tile shape.

  python tools/msa_build_throughput.py [--query-len 512] [--hits 1024] [--rows 16384] [--cols 512] [--rounds 5]
      [--out profiles/msa_build_throughput.log]

The stages behind the aligner read the hits' sequences, scores and alignment columns and nothing of the model, so the input is
made by construction rather than by a forward: one query, families of hits (a family's centre is the query with 35 % of its
residues substituted, a member its centre with 8 % more, deletions, insertions and unaligned ends), each hit's path the true
alignment of that construction, its score the number of identical matches.  One warm-up of every side, then --rounds timed
rounds alternating the sides in one process, each ending in a device synchronise; medians [min .. max]."""
import argparse
import os
import statistics
import sys
import time
import types
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from esm_amd import msa_build as MB  # noqa: E402
from esm_amd import ops  # noqa: E402

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
THREADS = 16


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def fmt(ts):
    return "%9.2f ms [%8.2f .. %8.2f]" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts))


def device_events(fn, rounds):
    ts = []
    for r in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if r:
            ts.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(ts)


def substitute(rng, seq, rate):
    out = seq.copy()
    at = rng.random(len(seq)) < rate
    out[at] = rng.choice(AA, int(at.sum()))
    return out


def planted(rng, Lq, P, family=16):
    """(query, hit sequences, paths, scores): see the module docstring."""
    query = rng.choice(AA, Lq)
    seqs, paths, scores = [], [], []
    centre = None
    for p in range(P):
        if p % family == 0:
            centre = substitute(rng, query, 0.35)
        member = substitute(rng, centre, 0.08)
        i0, i1 = int(rng.integers(0, Lq // 8)), Lq - int(rng.integers(0, Lq // 8))
        head, tail = rng.choice(AA, int(rng.integers(0, 20))), rng.choice(AA, int(rng.integers(0, 20)))
        seq, path, j, ident = list(head), [], len(head), 0
        for i in range(i0, i1):
            u = rng.random()
            if i0 < i < i1 - 1 and u < 0.02:
                path.append((i, -1))
                continue
            if i0 < i < i1 - 1 and u < 0.04:
                for _ in range(int(rng.integers(1, 4))):
                    seq.append(int(rng.choice(AA)))
                    path.append((-1, j))
                    j += 1
            seq.append(int(member[i]))
            path.append((i, j))
            ident += int(member[i] == query[i])
            j += 1
        seqs.append(bytes(seq + list(tail)).decode())
        paths.append(path)
        scores.append(float(ident))
    return bytes(query).decode(), seqs, paths, np.array(scores, dtype=np.float32)


def host_identity(m, gap, min_overlap, pool):
    """same / both of every pair of rows, fp32 [N, N]: numpy in chunks of rows on the pool's threads"""
    n = m.shape[0]
    letter = m != gap
    S = np.zeros((n, n), dtype=np.float32)

    def rows(lo, hi):
        for r in range(lo, hi):
            shared = letter[r][None, :] & letter
            both = shared.sum(1)
            same = (shared & (m[r][None, :] == m)).sum(1)
            ok = both >= min_overlap
            S[r, ok] = same[ok].astype(np.float32) / both[ok].astype(np.float32)

    step = -(-n // (4 * THREADS))
    list(pool.map(lambda lo: rows(lo, min(lo + step, n)), range(0, n, step)))
    return S


def host_loop(query, seqs, scores, cols_dev, offs_dev, min_coverage, max_identity, min_overlap, pool):
    """the loop a user writes today; returns the kept rows of [query; hits] in rank order and their matrix"""
    cols, offs = cols_dev.cpu().numpy(), offs_dev.cpu().numpy()
    Lq, P = len(query), len(seqs)
    m = np.full((P + 1, Lq), ord("-"), dtype=np.uint8)
    m[0] = np.frombuffer(query.encode(), dtype=np.uint8)
    n_match = np.zeros((P + 1,), dtype=np.int64)
    n_match[0] = Lq
    for p in range(P):
        seq = seqs[p]
        for i, j in cols[offs[p]:offs[p + 1]]:
            if i >= 0 and j >= 0:
                m[p + 1, i] = ord(seq[j])
                n_match[p + 1] += 1
    passed = (n_match >= 1) & (n_match.astype(np.float64) >= min_coverage * float(Lq))
    order = [0] + sorted((r for r in range(1, P + 1) if passed[r]), key=lambda r: (-float(scores[r - 1]), r))
    S = host_identity(m, ord("-"), min_overlap, pool)
    thr, kept = np.float32(max_identity), []
    for r in order:
        if not kept or not (S[kept, r] >= thr).any():
            kept.append(r)
    return kept, m[kept]


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--query-len", type=int, default=512)
    p.add_argument("--hits", type=int, default=1024)
    p.add_argument("--rows", type=int, default=16384)
    p.add_argument("--cols", type=int, default=512)
    p.add_argument("--min-coverage", type=float, default=0.5)
    p.add_argument("--max-identity", type=float, default=0.9)
    p.add_argument("--min-overlap", type=int, default=8)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msa_build_throughput: needs the GPU (a timing taken anywhere else says nothing)")
    rng = np.random.default_rng(args.seed)
    lines = ["search hits to an MSA on %s; %d rounds after one warm-up, alternating in one process, medians [min .. max]" % (
        torch.cuda.get_device_name(0), args.rounds)]
    # (i) the stages behind search_and_align
    query, seqs, paths, scores = planted(rng, args.query_len, args.hits)
    P = len(seqs)
    cols = torch.tensor([c for path in paths for c in path], dtype=torch.int32).cuda()
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum([len(path) for path in paths])]).astype(np.int64)).cuda()
    scores_dev = torch.from_numpy(scores).cuda()
    index = types.SimpleNamespace(sequences=seqs, labels=[f"hit{p}" for p in range(P)])
    kw = dict(min_coverage=args.min_coverage, max_identity=args.max_identity, min_overlap=args.min_overlap)
    pool = ThreadPoolExecutor(THREADS)
    sides = {"msa_build.msa_from_hits (device)": lambda: MB.msa_from_hits(("query", query), index, list(range(P)), scores_dev, cols, offs, **kw),
             "host loop (python + numpy, 16 threads)": lambda: host_loop(query, seqs, scores, cols, offs, args.min_coverage, args.max_identity,
                                                                         args.min_overlap, pool)}
    times = {name: [] for name in sides}
    for fn in sides.values():
        fn()
    for _ in range(args.rounds):
        for name, fn in sides.items():
            times[name].append(timed(fn)[0])
    built = sides["msa_build.msa_from_hits (device)"]()
    kept, rows = sides["host loop (python + numpy, 16 threads)"]()
    same = built.hit_ids.cpu().tolist() == [r - 1 for r in kept] and np.array_equal(built.msa.cpu().numpy(), rows)
    assert same, "the device path and the host loop keep different rows"
    lines.append("")
    lines.append("one query of %d residues, %d hits in families of 16 (paths by construction, %d alignment columns): %d hits pass the row "
                 "filter at coverage %.2f, %d rows stay at identity %.2f; both sides keep the same rows: %s" % (
                     args.query_len, P, cols.shape[0], int(built.counts["after_row_filter"]) - 1, args.min_coverage, len(kept),
                     args.max_identity, same))
    med = {k: statistics.median(v) for k, v in times.items()}
    for name in sides:
        lines.append("      %-42s %s" % (name, fmt(times[name])))
    a, b = med["msa_build.msa_from_hits (device)"], med["host loop (python + numpy, 16 threads)"]
    lines.append("      the device path over the host loop: %.2f x" % (b / a))
    # (ii) the identity kernel against the neighbour counts of the same matrix
    N_, L = args.rows, args.cols
    m = torch.from_numpy(rng.choice(AA[:6], (N_, L))).cuda()
    m[torch.rand((N_, L), device="cuda") < 0.25] = ord("-")
    S = torch.empty((N_, (N_ + 3) // 4 * 4), dtype=torch.float32, device="cuda")
    t_id = device_events(lambda: ops.msa_pair_identity(m, L=L, min_overlap=args.min_overlap, out=S), args.rounds)
    t_nc = device_events(lambda: ops.msa_neighbor_counts(m, L // 5), args.rounds)
    rate = lambda t: N_ * N_ * L / t / 1e12
    lines.append("")
    lines.append("msa uint8 [%d, %d], 25 %% gaps, device events: msa_pair_identity %.3f ms (%.2f T byte compares/s, fp32 [N, N] written: "
                 "%.2f GB), msa_neighbor_counts %.3f ms (%.2f T byte compares/s); identity over neighbour counts: %.2f x the rate" % (
                     N_, L, 1e3 * t_id, rate(t_id), 4.0 * N_ * S.shape[1] / 1e9, 1e3 * t_nc, rate(t_nc), t_nc / t_id))
    lines.append("")
    lines.append("    not measured: paths from the aligner on real embeddings, other lengths, depths and thresholds, several identity blocks, "
                 "the depth cut, the command line")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
