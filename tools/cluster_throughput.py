#!/usr/bin/env python
"""Range search and greedy clustering on pooled embeddings (esm_amd/cluster.py): (i) ``EmbeddingIndex.range_search`` of a centred
index against itself — two passes of the dense GEMM per block, the count and the fill launch — against the loop a user writes
today (unit vectors in fp32, ``torch`` matmul in chunks of rows, ``>=``, ``nonzero``); (ii) ``EmbeddingIndex.cluster`` against
that loop plus the sequential greedy walk on the host; (iii) the range kernel alone, by device events, against one read of its
block at the device's copy rate; (iv) the number of rounds.

  python tools/cluster_throughput.py [--vectors 65536 262144] [--embed-dim 1280] [--family 31] [--threshold 0.5] [--rounds 5]
      [--out profiles/cluster_throughput.log]

The data are random family-structured vectors: a common component 3 * randn(E), one centre randn(E) per family of --family
members, members = centre + common + 0.25 * randn(E); centred, so that a member's cosine to its family is about 0.94 and to the
rest about 0: the threshold gives --family - 1 neighbours per node.  One warm-up of every side, then --rounds timed rounds
alternating the sides in one process, each ending in a device synchronise; medians [min .. max].  Both sides' graphs and clusters
are compared (torch's fp32 product is rounded differently from the f16x3 GEMM; at these margins they agree, which is reported)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from esm_amd import _native as N  # noqa: E402
from esm_amd import cluster as C  # noqa: E402
from esm_amd import ops  # noqa: E402
from esm_amd import search as S  # noqa: E402

COPY_RATE = 4.05e12  # bytes / s of a device copy's read side, profiles/stream_edit_throughput.log


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def fmt(ts):
    return "%9.2f ms [%8.2f .. %8.2f]" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts))


def alternate(sides, rounds):
    times = {name: [] for name in sides}
    for fn in sides.values():
        fn()
    for _ in range(rounds):
        for name, fn in sides.items():
            times[name].append(timed(fn)[0])
    return times


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


def torch_range(unit, threshold, chunk_bytes):
    """the loop a user writes: fp32 matmul per chunk of rows against the whole (unit) database, >=, nonzero; the diagonal dropped"""
    n = unit.shape[0]
    rows = max(1, chunk_bytes // (4 * n))
    src, dst, val = [], [], []
    for lo in range(0, n, rows):
        s = unit[lo:lo + rows] @ unit.t()
        s[torch.arange(s.shape[0], device=s.device), torch.arange(lo, lo + s.shape[0], device=s.device)] = -2.0
        hit = (s >= threshold).nonzero()
        src.append(hit[:, 0] + lo)
        dst.append(hit[:, 1])
        val.append(s[hit[:, 0], hit[:, 1]])
    return torch.cat(src), torch.cat(dst), torch.cat(val)


def host_greedy(src, dst, lengths):
    """... and the sequential greedy walk on the host: the longest first, a representative covers its undecided neighbours"""
    n = len(lengths)
    src, dst = src.cpu().numpy(), dst.cpu().numpy()
    offsets = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))])
    walk = np.argsort(-lengths, kind="stable")
    state = np.zeros((n,), dtype=np.int8)
    rep_of = np.arange(n)
    for u in walk:
        if state[u]:
            continue
        state[u] = 1
        out = dst[offsets[u]:offsets[u + 1]]
        out = out[state[out] == 0]
        state[out] = 2
        rep_of[out] = u
    return rep_of


def one_size(args, n, lines):
    E, fam = args.embed_dim, args.family
    g = torch.Generator(device="cuda").manual_seed(args.seed)
    common = 3 * torch.randn((E,), generator=g, device="cuda")
    centres = torch.randn((-(-n // fam), E), generator=g, device="cuda")
    vectors = np.empty((n, E), dtype=np.float32)
    for lo in range(0, n, 1 << 16):
        hi = min(lo + (1 << 16), n)
        x = centres[torch.arange(lo, hi, device="cuda") // fam] + common + 0.25 * torch.randn((hi - lo, E), generator=g, device="cuda")
        vectors[lo:hi] = x.cpu().numpy()
    lengths = np.random.default_rng(args.seed).integers(50, 1000, n)
    t_center, index = timed(lambda: S.EmbeddingIndex(vectors, [""] * n, lengths).centered())
    del vectors
    t_image, _ = timed(lambda: index.to("cuda"))
    unit = torch.empty((n, E), dtype=torch.float32, device="cuda")
    for lo in range(0, n, 1 << 16):
        unit[lo:lo + (1 << 16)] = torch.nn.functional.normalize(torch.from_numpy(index.vectors[lo:lo + (1 << 16)]).cuda(), dim=1)
    thr = args.threshold
    qc, nb = S.plan_search(n, n, args.max_bytes)
    lines.append("")
    lines.append("N = %d family-structured fp32 vectors (families of %d), E = %d, centred on the host in %.2f s, device image %.2f GB built in "
                 "%.2f s; threshold %.2f; blocks of [%d, %d] similarities (%d x %d blocks a pass)" % (
                     n, fam, E, t_center, index.image_bytes() / 1e9, t_image, thr, qc, nb, -(-n // qc), -(-n // nb)))
    sides = {"index.range_search": lambda: index.range_search(index, thr, exclude_self=True, max_bytes=args.max_bytes),
             "torch matmul + >= + nonzero": lambda: torch_range(unit, thr, args.max_bytes),
             "index.cluster": lambda: index.cluster(thr, max_bytes=args.max_bytes),
             "torch loop + host greedy": lambda: host_greedy(*torch_range(unit, thr, args.max_bytes)[:2], lengths)}
    times = alternate(sides, args.rounds)
    G, theirs = sides["index.range_search"](), sides["torch matmul + >= + nonzero"]()
    out, rep_host = sides["index.cluster"](), sides["torch loop + host greedy"]()
    nnz = G["ids"].numel()
    same_graph = nnz == theirs[1].numel() and bool((G["ids"].long() == theirs[1]).all())
    same_clusters = bool((out["rep_of"].cpu().numpy() == rep_host).all())
    med = {k: statistics.median(v) for k, v in times.items()}
    lines.append("    %.1f neighbours per node (%d pairs); %d clusters in %d rounds (one host read per %d rounds); the torch loop's graph equal: %s, "
                 "its clusters equal: %s" % (nnz / n, nnz, out["representatives"].numel(), out["rounds"],
                                             C.ROUNDS_PER_READ, same_graph, same_clusters))
    for name in sides:
        lines.append("      %-30s %s   %8.2f G similarities/s" % (name, fmt(times[name]), n * n / med[name] / 1e9))
    lines.append("      range_search over the torch loop: %.2f x; cluster over the torch loop + host greedy: %.2f x; the rounds and the assignment "
                 "(cluster - range_search): %.2f ms" % (med["torch matmul + >= + nonzero"] / med["index.range_search"],
                                                       med["torch loop + host greedy"] / med["index.cluster"],
                                                       1e3 * (med["index.cluster"] - med["index.range_search"])))
    # the first block's launches by device events
    width = min(nb, S._up(n, S.BLOCK_ALIGN))
    cols = min(nb, n)
    img_q = ops.align_rows(torch.from_numpy(index.vectors[:qc]).cuda(), None, cosine=True, b_side=False)
    blk = torch.empty((qc, width), dtype=torch.float32, device="cuda")
    counts = torch.zeros((qc,), dtype=torch.int64, device="cuda")
    t_gemm = device_events(lambda: ops.linear(img_q, index.image[:width], None, N.EPI_STORE_F32, out=blk), args.rounds)
    t_count = device_events(lambda: ops.range_rows(blk, thr, counts=counts, n_cols=cols), args.rounds)
    counts.zero_()
    ops.range_rows(blk, thr, counts=counts, n_cols=cols)
    offsets = torch.zeros((qc + 1,), dtype=torch.int64, device="cuda")
    offsets[1:] = counts.cumsum(0)
    ids = torch.empty((int(offsets[-1]),), dtype=torch.int32, device="cuda")
    scores = torch.empty((int(offsets[-1]),), dtype=torch.float32, device="cuda")
    cursor = offsets[:-1].clone()

    def fill():
        cursor.copy_(offsets[:-1])
        ops.range_rows(blk, thr, offsets=offsets, cursor=cursor, ids=ids, scores=scores, n_cols=cols)

    t_fill = device_events(fill, args.rounds)
    read = 4.0 * qc * cols
    lines.append("      first block [%d, %d], device events: GEMM %.3f ms (%.1f TFLOP/s of 2 Q N 3 Ep), count launch %.3f ms (%.2f TB/s read; one "
                 "read at the copy rate: %.3f ms, %.2f x that), fill launch (with the copy of the cursors) %.3f ms (%.2f x one read), %d pairs" % (
                     qc, cols, 1e3 * t_gemm, 2.0 * qc * width * index.image.shape[1] / t_gemm / 1e12, 1e3 * t_count, read / t_count / 1e12,
                     1e3 * read / COPY_RATE, t_count / (read / COPY_RATE), 1e3 * t_fill, t_fill / (read / COPY_RATE), ids.numel()))
    del index, unit, blk
    torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--vectors", type=int, nargs="+", default=[1 << 16, 1 << 18])
    p.add_argument("--embed-dim", type=int, default=1280)
    p.add_argument("--family", type=int, default=31)
    p.add_argument("--threshold", type=float, default=0.5)
    p.add_argument("--max-bytes", type=int, default=2 << 30)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cluster_throughput: needs the GPU (a timing taken anywhere else says nothing)")
    lines = ["range search and clustering on %s; %d rounds after one warm-up, alternating in one process, medians [min .. max]" % (
        torch.cuda.get_device_name(0), args.rounds)]
    for n in args.vectors:
        one_size(args, n, lines)
    lines.append("")
    lines.append("    not measured: real embeddings, other thresholds, family sizes and E, assign=\"nearest\", priority=\"degree\", the command line")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
