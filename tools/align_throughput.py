#!/usr/bin/env python
"""Embedding-based alignment of a query set against a target set: ``esm_amd.align_embeddings`` (esm_amd/align.py: operand
images, the dense GEMM, the affine-gap DP and the walk on the device, in blocks that fit ``--max-bytes``) against the loop a user
writes today: cosine similarity in torch on the device, the matrix to the host, and a numpy DP vectorised along anti-diagonals
(scores only), one pair at a time.

  python tools/align_throughput.py [--queries 64] [--targets 256] [--embed-dim 1280] [--mode local] [--baseline-pairs 24]
      [--rounds 5] [--free-ends b] [--hits-per-pair 3] [--baseline-lib OTHER/libesmk.so] [--out profiles/align_throughput.log]

Lengths are drawn from the UniRef-like mix of tools/bench_varlen.py; the representations are random fp32 rows of ``--embed-dim``
columns (1280: the 650M model) — the forward is not part of the measurement, the alignment is.  The host loop is far too slow
for all pairs: it is timed on the first ``--baseline-pairs`` pairs of a fixed shuffle and reported in cells per second, like the
engine (a cell is one (i, j) of a pair).  One warm-up of every side, then --rounds timed rounds alternating the sides in one
process, each ending in a device synchronise; medians [min .. max].  The DP kernel's share is measured on the call's first
block with device events: images + GEMM, DP, walk.  The two sides' scores are compared on the baseline pairs (torch's fp32
similarity is rounded differently from the f16x3 GEMM: the largest difference is reported, not asserted).

``--free-ends`` (a, b, both) and ``--hits-per-pair K`` add sides of the same alternating rounds: global mode with that mask
(scores only, with paths) and ``--mode`` with K hits per pair.  ``--baseline-lib`` names another build of libesmk.so (the parent
commit's): local and global mode, scores only and with paths, are timed under it and under this library as further sides, the
library swapped in around each of its calls; an older build has no ``_ex`` alignment entries, so those calls (always with
free_ends = 0 and without a mask there) go to its plain entries."""
import argparse
import contextlib
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_varlen import uniref_like_lengths  # noqa: E402
from esm_amd import _native as N  # noqa: E402
from esm_amd import align as A  # noqa: E402
from esm_amd import ops  # noqa: E402


class BaselineLibrary:
    """Another build of libesmk.so under the signatures of esm_amd/_native.py.  The two ``_ex`` alignment entries an older
    build lacks are served by its plain entries: the calls made under it carry free_ends = 0 and no mask."""

    def __init__(self, path):
        self._lib = ctypes.CDLL(path)
        for name, (res, argtypes) in N.SIGNATURES.items():
            fn = getattr(self._lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, argtypes

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def esmk_op_align_dp_ex(self, *a):
        assert a[7] == 0
        return self._lib.esmk_op_align_dp(*a[:7], *a[8:])

    def esmk_op_align_traceback_ex(self, *a):
        assert a[3] == 0 and not a[13].value
        return self._lib.esmk_op_align_traceback(*a[:3], *a[4:13], a[17])


@contextlib.contextmanager
def library(lib):
    """Every engine call inside goes to ``lib`` (esm_amd looks ``_native.lib`` up at call time)."""
    mine, N.lib = N.lib, lib
    try:
        yield
    finally:
        N.lib = mine


def numpy_dp_score(S, local, o, e):
    """the score of the affine-gap DP on S [La, Lb], one vectorised step per anti-diagonal"""
    La, Lb = S.shape
    o, e = np.float32(o), np.float32(e)
    neg = np.float32(-np.inf)
    H = np.full((La + 1, Lb + 1), neg, dtype=np.float32)
    E, F = H.copy(), H.copy()
    H[0, 0] = 0
    floor = np.float32(0) if local else neg
    for d in range(1, La + Lb + 1):
        i = np.arange(max(0, d - Lb), min(La, d) + 1)
        j = d - i
        Ev = np.where(j > 0, np.maximum(H[i, j - 1] - o, E[i, j - 1] - e), neg)
        Fv = np.where(i > 0, np.maximum(H[i - 1, j] - o, F[i - 1, j] - e), neg)
        Dv = np.where((i > 0) & (j > 0), S[i - 1, j - 1] + H[i - 1, j - 1], neg)
        H[i, j], E[i, j], F[i, j] = np.maximum(np.maximum(np.maximum(floor, Dv), Fv), Ev), Ev, Fv
    return float(H.max()) if local else float(H[La, Lb])


def host_loop(reps_a, reps_b, pairs, local, o, e):
    scores = []
    for a, b in pairs:
        xa, xb = reps_a[a], reps_b[b]
        S = (torch.nn.functional.normalize(xa, dim=1) @ torch.nn.functional.normalize(xb, dim=1).t()).cpu().numpy()
        scores.append(numpy_dp_score(S, local, o, e))
    return scores


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def fmt(ts, cells):
    m = statistics.median(ts)
    return "%9.2f ms [%8.2f .. %8.2f]   %9.3f G cells/s" % (1e3 * m, 1e3 * min(ts), 1e3 * max(ts), cells / m / 1e9)


def first_block_parts(flat_a, len_a, flat_b, len_b, pairs, mode, o, e, max_bytes, rounds):
    """device-event times of the parts of the call's first block: (images + GEMM, DP with bytes, walk), cells of the block"""
    la, lb = np.asarray(len_a), np.asarray(len_b)
    a0, a1, b0, b1, idx = A.plan_blocks(la, lb, pairs, flat_a.shape[1], max_bytes)[0]
    off_a, off_b = np.concatenate([[0], np.cumsum(la)]), np.concatenate([[0], np.cumsum(lb)])
    ra = torch.arange(int(off_a[a0]), int(off_a[a1]), dtype=torch.int32, device="cuda")
    lb8 = (lb[b0:b1] + 7) // 8 * 8
    col_b = np.concatenate([[0], np.cumsum(lb8)])
    src = np.full(((int(col_b[-1]) + 63) // 64 * 64,), -1, dtype=np.int32)
    for k in range(b1 - b0):
        src[col_b[k]:col_b[k] + lb[b0 + k]] = np.arange(off_b[b0 + k], off_b[b0 + k + 1])
    rb = torch.from_numpy(src).cuda()
    pa, pb = pairs[idx, 0], pairs[idx, 1]
    table_np, tb_bytes = A.pair_table(off_a[pa] - off_a[a0], la[pa], col_b[pb - b0], lb[pb])
    table = torch.from_numpy(table_np).cuda()
    tb = torch.empty((tb_bytes,), dtype=torch.uint8, device="cuda")
    cap = la[pa] + lb[pb]
    slot = torch.from_numpy(np.concatenate([[0], np.cumsum(cap)])[:-1].copy()).cuda()
    cols = torch.empty((int(cap.sum()), 2), dtype=torch.int32, device="cuda")
    times = [[], [], []]
    for r in range(rounds + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        S = ops.linear(ops.align_rows(flat_a, ra), ops.align_rows(flat_b, rb, b_side=True), None, N.EPI_STORE_F32)
        ev[1].record()
        res = ops.align_dp(S, table, A.MODES[mode], o, e, int(la[pa].max()), int(lb[pb].max()), want_traceback=True, tb=tb)
        ev[2].record()
        ops.align_traceback(table, A.MODES[mode], res["end"], tb, slot, cols)
        ev[3].record()
        torch.cuda.synchronize()
        if r:  # the first round warms up
            for k in range(3):
                times[k].append(ev[k].elapsed_time(ev[k + 1]) * 1e-3)
    return [statistics.median(t) for t in times], int((la[pa] * lb[pb]).sum()), len(idx)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--queries", type=int, default=64)
    p.add_argument("--targets", type=int, default=256)
    p.add_argument("--embed-dim", type=int, default=1280)
    p.add_argument("--mode", choices=("global", "local"), default="local")
    p.add_argument("--gap-open", type=float, default=1.0)
    p.add_argument("--gap-extend", type=float, default=0.1)
    p.add_argument("--baseline-pairs", type=int, default=24)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--max-bytes", type=int, default=4 << 30)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--free-ends", choices=("a", "b", "both"), default=None, help="a further side: global mode with this free-end mask")
    p.add_argument("--hits-per-pair", type=int, default=1, help="a further side: --mode with K hits per pair")
    p.add_argument("--baseline-lib", default=None, help="another build of libesmk.so: local and global mode under it are further sides")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("align_throughput: needs the GPU (a timing taken anywhere else says nothing)")
    g = torch.Generator().manual_seed(args.seed)
    len_a, len_b = uniref_like_lengths(args.queries, g), uniref_like_lengths(args.targets, g)
    E = args.embed_dim
    flat_a = torch.randn((sum(len_a), E), generator=g).cuda()
    flat_b = torch.randn((sum(len_b), E), generator=g).cuda()
    reps_a, reps_b = list(flat_a.split(len_a)), list(flat_b.split(len_b))
    pairs = A.check_pairs(None, len(len_a), len(len_b))
    cells = int(sum(len_a)) * int(sum(len_b))
    sample = pairs[np.random.default_rng(args.seed).permutation(len(pairs))[:args.baseline_pairs]]
    sample_cells = int(sum(len_a[a] * len_b[b] for a, b in sample))
    kw = dict(mode=args.mode, gap_open=args.gap_open, gap_extend=args.gap_extend, max_bytes=args.max_bytes)
    local = args.mode == "local"
    sides = {
        "engine, scores only": (lambda: A.align_embeddings((flat_a, len_a), (flat_b, len_b), paths=False, **kw), cells),
        "engine, with paths": (lambda: A.align_embeddings((flat_a, len_a), (flat_b, len_b), **kw), cells),
        "host loop (sample)": (lambda: host_loop(reps_a, reps_b, sample, local, args.gap_open, args.gap_extend), sample_cells),
        "engine on the sample": (lambda: A.align_embeddings((flat_a, len_a), (flat_b, len_b), pairs=sample, paths=False, **kw), sample_cells),
    }
    both = ((flat_a, len_a), (flat_b, len_b))
    pen = dict(gap_open=args.gap_open, gap_extend=args.gap_extend, max_bytes=args.max_bytes)
    if args.free_ends:
        sides["free_ends=%s, scores only" % args.free_ends] = (lambda: A.align_embeddings(*both, mode="global", free_ends=args.free_ends, paths=False, **pen), cells)
        sides["free_ends=%s, with paths" % args.free_ends] = (lambda: A.align_embeddings(*both, mode="global", free_ends=args.free_ends, **pen), cells)
    if args.hits_per_pair > 1:
        sides["%s, %d hits per pair" % (args.mode, args.hits_per_pair)] = (lambda: A.align_embeddings(*both, hits_per_pair=args.hits_per_pair, **kw), cells)
    base = None
    if args.baseline_lib:
        base = BaselineLibrary(args.baseline_lib)

        def under(lib, mode, paths):
            def call():
                with library(lib):
                    return A.align_embeddings(*both, mode=mode, paths=paths, **pen)
            return call

        for mode in ("local", "global"):
            for paths in (False, True):
                what = "%s, %s" % (mode, "with paths" if paths else "scores only")
                sides["parent library, " + what] = (under(base, mode, paths), cells)
                sides["this library,   " + what] = (under(N.lib, mode, paths), cells)
    times = {name: [] for name in sides}
    for fn, _ in sides.values():
        fn()
    for _ in range(args.rounds):
        for name, (fn, _) in sides.items():
            times[name].append(timed(fn)[0])
    blocks = len(A.plan_blocks(len_a, len_b, pairs, E, args.max_bytes))
    lines = ["%d x %d pairs, lengths of the UniRef-like mix (mean %.0f / %.0f residues), E = %d random fp32 rows, on %s; mode %s, o = %g, "
             "e = %g, cosine; %.3f G cells, %d block%s at max_bytes = %d; %d rounds after one warm-up, alternating, medians [min .. max]"
             % (len(len_a), len(len_b), np.mean(len_a), np.mean(len_b), E, torch.cuda.get_device_name(0), args.mode, args.gap_open,
                args.gap_extend, cells / 1e9, blocks, "" if blocks == 1 else "s", args.max_bytes, args.rounds), ""]
    for name, (_, c) in sides.items():
        lines.append("    %-42s %s   (%d pairs)" % (name, fmt(times[name], c), len(sample) if "sample" in name else len(pairs)))
    ratio = (cells / statistics.median(times["engine, scores only"])) / (sample_cells / statistics.median(times["host loop (sample)"]))
    lines.append("    cells per second, engine (scores only, all pairs) over host loop (sample): %.0f x" % ratio)
    if base is not None:
        lines.append("    parent library: %s; this library: %s" % (base.esmk_version().decode(), N.lib.esmk_version().decode()))
        for mode in ("local", "global"):
            for what in ("scores only", "with paths"):
                old, new = times["parent library, %s, %s" % (mode, what)], times["this library,   %s, %s" % (mode, what)]
                m_old, m_new, spread = statistics.median(old), statistics.median(new), max(old) - min(old)
                ok = min(old) <= m_new <= max(old) or m_new <= m_old + spread
                lines.append("    %s, %s: this library's median %.2f ms against the parent's %.2f ms [%.2f .. %.2f]: %s" % (
                    mode, what, 1e3 * m_new, 1e3 * m_old, 1e3 * min(old), 1e3 * max(old),
                    "within the parent's rounds" if ok else "SLOWER than the parent's rounds"))
            outs = [sides["%s %s, with paths" % (lib, mode)][0]() for lib in ("parent library,", "this library,  ")]
            same = all(torch.equal(outs[0][k], outs[1][k]) for k in ("score", "end", "cols"))
            lines.append("    %s: score, end and cols of the two libraries: %s" % (mode, "the same bits" if same else "DIFFERENT"))
    if args.hits_per_pair > 1:
        one = statistics.median(times["engine, with paths"])
        k_hits = statistics.median(times["%s, %d hits per pair" % (args.mode, args.hits_per_pair)])
        lines.append("    %d hits per pair cost %.2f x the call with one hit (both with paths; images and GEMM run once)" % (args.hits_per_pair, k_hits / one))
    ours = sides["engine on the sample"][0]()["score"].cpu().numpy()
    theirs = np.array(sides["host loop (sample)"][0](), dtype=np.float64)
    lines.append("    scores on the sample: largest difference %.3e (largest score %.3f)" % (np.abs(ours - theirs).max(), np.abs(theirs).max()))
    parts, bc, bp = first_block_parts(flat_a, len_a, flat_b, len_b, pairs, args.mode, args.gap_open, args.gap_extend, args.max_bytes,
                                      args.rounds)
    total = sum(parts)
    lines.append("    first block (%d pairs, %.3f G cells), device events: images + GEMM %.2f ms, DP with traceback bytes %.2f ms (%.0f %%, "
                 "%.1f G cells/s), walk %.2f ms" % (bp, bc / 1e9, 1e3 * parts[0], 1e3 * parts[1], 100 * parts[1] / total,
                                                    bc / parts[1] / 1e9, 1e3 * parts[2]))
    lines.append("    not measured: the forward that produces the representations, enhance=True, the command line")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
