#!/usr/bin/env python
"""What an edit of the residual stream costs (esm_amd/interventions.py, csrc/interventions.hip), and that a forward without
edits costs what it did: one model, one batch, four sides in alternating rounds of one process.

  python tools/stream_edit_throughput.py [--model 650M] [--batch 64] [--length 1020] [--rounds 5] [--calls 3]
      [--baseline-lib PARENT/libesmk.so] [--out profiles/stream_edit_throughput.log]

  forward, baseline library   ``model(tokens)`` under another build of libesmk.so (the parent commit's: --baseline-lib)
  forward                     ``model(tokens)`` under this library — the same bits, and a time inside the spread of the line above
  one edit                    ``model.forward_edited`` with one ``add`` of a vector on every token at the middle layer
  an edit at every layer      the same edit at each of the layers 0 .. L

One warm-up of every side, then --rounds rounds that alternate the sides; a round times --calls calls of a side and ends in a
device synchronise.  Medians per call with the spread [min .. max] over the rounds.  By byte count an all-token edit reads and
writes the fp32 stream once (8 B per element; with the LayerNorm fold, at a middle layer, 2 B more for the operand row):
the model's bytes are printed next to the measured difference.
"""
import argparse
import gc
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from esm_amd import StreamEdit  # noqa: E402
from esm_amd.synth import ESM2_DIMS, synth_tokens  # noqa: E402
from sample_throughput import library, load_library, make_model, report, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="650M")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--length", type=int, default=1020, help="residues; T = length + 2")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls of a side per timed round")
    ap.add_argument("--baseline-lib", default=None, help="another build of libesmk.so (the parent commit's)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_edit_throughput: needs the GPU (a CPU run measures nothing)")
    name = next(k for k in ESM2_DIMS if args.model in k)
    L, E, H = ESM2_DIMS[name]
    model = make_model(L, E, H)
    toks = synth_tokens(args.batch, args.length, seed=1).cuda()
    B, T = toks.shape
    vec = torch.randn(E, generator=torch.Generator().manual_seed(3))
    one = [StreamEdit(L // 2, "add", vec, gain=0.5, positions="all")]
    every = [StreamEdit(k, "add", vec, gain=0.5, positions="all") for k in range(L + 1)]
    from esm_amd import _native as N

    lines = ["%s (L %d, E %d, H %d) on %s; B = %d, T = %d (%d rows); %d rounds of %d calls after one warm-up, ms per call, "
             "medians [min .. max]" % (name, L, E, H, torch.cuda.get_device_name(0), B, T, B * T, args.rounds, args.calls)]
    base = base_model = None
    sides = {}
    with torch.no_grad():
        if args.baseline_lib:
            base = load_library(args.baseline_lib)
            with library(base):
                base_model = make_model(L, E, H)
                lines.append("baseline library: %s" % base.esmk_version().decode())
            lines.append("this library:     %s" % N.lib.esmk_version().decode())

            def baseline():
                with library(base):
                    return base_model(toks)["logits"]

            sides["forward, baseline library"] = baseline
        sides["forward"] = lambda: model(toks)["logits"]
        sides["one edit (layer %d)" % (L // 2)] = lambda: model.forward_edited(toks, one)["logits"]
        sides["an edit at every layer (%d)" % (L + 1)] = lambda: model.forward_edited(toks, every)["logits"]
        outs = {side: fn() for side, fn in sides.items()}  # warm-up
        lines.append("LayerNorm fold: %s" % ("on" if model.ln_fold_active() else "off"))
        if base is not None:
            lines.append("forward under the baseline library and under this one: %s" % (
                "the same logits, bit for bit" if torch.equal(outs["forward, baseline library"], outs["forward"]) else "DIFFERENT logits"))
        outs = None
        times = {side: [] for side in sides}
        for _ in range(args.rounds):
            for side, fn in sides.items():
                times[side].append(timed(lambda: [fn() for _ in range(args.calls)])[0] / args.calls)
    med = {side: statistics.median(t) for side, t in times.items()}
    for side in sides:
        lines.append("  %-32s %8.2f ms [%.2f .. %.2f]" % (side, 1e3 * med[side], 1e3 * min(times[side]), 1e3 * max(times[side])))
    names = list(sides)
    if base is not None:
        lo, hi = min(times[names[0]]), max(times[names[0]])
        lines.append("  forward / baseline: %.4f x; the median of forward lies %s the baseline's rounds [%.2f .. %.2f] ms" % (
            med["forward"] / med[names[0]], "inside" if lo <= med["forward"] <= hi else "OUTSIDE", 1e3 * lo, 1e3 * hi))
    gb = B * T * E * 8 / 1e9
    for side, n in ((names[-2], 1), (names[-1], L + 1)):
        extra = med[side] - med["forward"]
        lines.append("  %s - forward: %+.2f ms for %d edit(s) of %.2f GB each (stream read + written)%s" % (
            side, 1e3 * extra, n, gb, "; %.2f TB/s" % (n * gb / extra / 1e3) if extra > 0 else ""))
    if base is not None:  # the baseline model's engine is freed by the library that made it
        with library(base):
            base_model = None
            gc.collect()
    report(lines, args.out)


if __name__ == "__main__":
    main()
