#!/usr/bin/env python
"""Neighbour counts and the greedy pick of a deep MSA: the device entries (esm_amd/msa_select.py over csrc/msa_select.hip)
against what a user does without them, numpy on the host.

  python tools/msa_select_throughput.py [--rows 16384 65536] [--cols 512] [--rounds 5] [--threads 16] [--host-rows 2048]
      [--full-check-up-to 16384] [--greedy 128] [--out profiles/msa_select_throughput.log]

``neighbour counts``: ``esmk_op_msa_neighbor_counts`` (one call ending in a device synchronise; the byte matrix is already on
the device) against a chunked numpy count — per row ``count_nonzero(msa != msa[i], axis=1) <= m`` — spread over --threads
threads of this process.  The counts of both sides are compared first — on every row up to --full-check-up-to rows, on the
first --host-rows rows beyond — and nothing is timed unless they are equal; the time of that host pass is reported as one run.
Then --rounds rounds alternating the sides, medians and the spread; to keep the device from idling for minutes a timed host
round counts the first --host-rows rows against all N and its time is scaled by N / host-rows (the work per row is the same
for every row), and the log says so.  ``greedy``: ``esmk_op_msa_greedy_select`` for --greedy rows against the notebook's rule
in numpy (per step the Hamming distances of the last pick to every row, kept as a growing matrix whose column means are taken
anew), once each; the tool reports whether the two rules chose the same rows.  The alignment is the seeded family generator of
tests/_msa_select_ref.py.  There is no pass / fail ratio: the comparison side is host code."""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _msa_select_ref as M  # noqa: E402
from esm_amd import msa_select, ops  # noqa: E402


def host_counts(a, m, rows, threads):
    """count[i] for i < rows against all rows of ``a``: row chunks dealt to a thread pool (numpy releases the GIL)."""
    out = np.zeros(rows, dtype=np.int64)

    def work(lo):
        for i in range(lo, min(lo + 64, rows)):
            out[i] = int(np.count_nonzero(np.count_nonzero(a != a[i], axis=1) <= m))

    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(work, range(0, rows, 64)))
    return out


def host_greedy(a, num):
    """The notebook's rule written in numpy: float Hamming distances, a [k, N] matrix that grows by a row per step, the mean
    over its rows for the unselected columns, argmax (the first of equal maxima).  Returns the picks in pick order."""
    n, L = a.shape
    picks = [0]
    dist = np.zeros((0, n))
    every = np.arange(n)
    for _ in range(num - 1):
        d = np.count_nonzero(a != a[picks[-1]], axis=1) / float(L)
        dist = np.concatenate([dist, d[None]])
        left = np.delete(every, picks)
        picks.append(int(left[np.argmax(np.delete(dist, picks, axis=1).mean(0))]))
    return picks


def timed_device(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def spread(ts):
    return f"median {statistics.median(ts) * 1e3:10.2f} ms   min {min(ts) * 1e3:10.2f}   max {max(ts) * 1e3:10.2f}   ({len(ts)} rounds)"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[16384])
    ap.add_argument("--cols", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-rows", type=int, default=2048, help="rows the host side counts in a timed round")
    ap.add_argument("--full-check-up-to", type=int, default=16384, help="largest N whose counts are compared on every row")
    ap.add_argument("--greedy", type=int, default=128)
    ap.add_argument("--theta", type=float, default=0.2)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("msa_select_throughput: no GPU: nothing to measure")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# msa_select_throughput: {torch.cuda.get_device_name(0)}, host side numpy {np.__version__} on {args.threads} threads")
    for n in args.rows:
        L = args.cols
        a = M.family_msa(n, L, 0)
        m = msa_select.max_mismatch(args.theta, L)
        dev = torch.from_numpy(a).cuda()
        full = n <= args.full_check_up_to
        check_rows, rows = (n if full else min(args.host_rows, n)), min(args.host_rows, n)
        say(f"\n## {n} x {L}, theta {args.theta} (at most {m} mismatches), {n * n * L:.3g} byte compares")
        t = time.perf_counter()
        want = host_counts(a, m, check_rows, args.threads)
        t_check = time.perf_counter() - t
        _, got = timed_device(lambda: ops.msa_neighbor_counts(dev, m))  # warm-up
        got = got.cpu().numpy()
        if not np.array_equal(got[:check_rows], want):
            say(f"COUNTS DIFFER in {int((got[:check_rows] != want).sum())} of {check_rows} rows: nothing is timed")
            continue
        say(f"counts equal on {'all' if full else 'the first'} {check_rows} rows (min {int(got.min())}, max {int(got.max())}, "
            f"Neff {float((1.0 / got).sum()):.1f}); that host pass took {t_check * 1e3:.0f} ms, one run")
        t_dev, t_host = [], []
        for r in range(args.rounds):
            t_dev.append(timed_device(lambda: ops.msa_neighbor_counts(dev, m))[0])
            t = time.perf_counter()
            host_counts(a, m, rows, args.threads)
            t_host.append((time.perf_counter() - t) * n / rows)
        say(f"device neighbour counts   {spread(t_dev)}")
        say(f"host neighbour counts     {spread(t_host)}"
            + ("" if rows == n else f"   (the first {rows} rows against all {n}, timed and scaled by {n / rows:g})"))
        say(f"ratio of the medians: host / device = {statistics.median(t_host) / statistics.median(t_dev):.0f}")
        d = statistics.median(t_dev)
        say(f"device rate: {n * n * L / d / 1e12:.2f} T byte compares / s counting every ordered pair "
            f"({n * n * ((L + 3) // 4) * 6 / d / 1e12:.2f} T lane operations / s at 6 per dword pair)")
        if args.greedy > 1:
            timed_device(lambda: ops.msa_greedy_select(dev, 4))  # warm-up
            td, sel = timed_device(lambda: ops.msa_greedy_select(dev, args.greedy))
            sel = sel.tolist()
            t = time.perf_counter()
            ref = host_greedy(a, args.greedy)
            th = time.perf_counter() - t
            say(f"greedy pick of {args.greedy} rows: device {td * 1e3:.2f} ms, numpy (notebook rule) {th * 1e3:.0f} ms, one run each; "
                f"same rows: {'yes' if sorted(sel) == sorted(ref) else 'NO'}, same order: {'yes' if sel == ref else 'no'}")
        del dev
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
