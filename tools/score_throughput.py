#!/usr/bin/env python
"""Masked-marginal scoring of one protein: ``model.masked_marginals`` (esm_amd/scoring.py: masked copies built on the device,
batches that fill the GPU, the head of the model on the one masked row of every copy) against the reference's loop
(examples/variant-prediction/predict.py:205-215) written on the same model's ``forward``: T forwards at B = 1, each building
[1, T, V] logits and keeping one row.

  python tools/score_throughput.py [--model 650M] [--lengths 510 1020] [--rounds 5] [--out profiles/scoring_throughput.log]

Same library and same process for both sides; one warm-up of each side per shape, then --rounds timed rounds alternating the
two sides, each round ending in a device synchronise; medians and the spread.  Residues/s counts the scored positions (all T
tokens of the row).  Also recorded: the engine workspace each side grew to, the bytes of logits / log-probabilities each side
writes over the whole protein, and the largest difference between the two tables (the loop's log_softmax is torch's).
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import esm  # noqa: E402
from esm_amd.synth import ESM2_DIMS, skip_param_init, synth_esm2_state_dict, synth_tokens  # noqa: E402


def loop_rows(model, toks):
    """The reference's loop: one B = 1 forward per position, log_softmax of its logits, one row kept."""
    rows = []
    for i in range(toks.shape[1]):
        masked = toks.clone()
        masked[0, i] = model.mask_idx
        rows.append(torch.log_softmax(model(masked)["logits"], dim=-1)[:, i])
    return torch.cat(rows, dim=0)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="650M")
    ap.add_argument("--lengths", type=int, nargs="+", default=[510, 1020], help="residues; T = length + 2")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_throughput: needs the GPU (a CPU run measures nothing)")
    name = next(k for k in ESM2_DIMS if args.model in k)
    L, E, H = ESM2_DIMS[name]
    with skip_param_init():
        model = esm.ESM2(L, E, H).eval()
    model.load_state_dict(synth_esm2_state_dict(L, E, H, seed=0))
    model = model.cuda()
    with torch.no_grad():
        model(synth_tokens(1, 30).cuda())  # the engine exists from here on: its LayerNorm-fold mode can be read
    lines = ["%s (L %d, E %d, H %d) on %s; LayerNorm fold %s; %d rounds after one warm-up, medians [min .. max]" % (
        name, L, E, H, torch.cuda.get_device_name(0), "on" if model.ln_fold_active() else "off", args.rounds)]
    V = model.alphabet_size
    with torch.no_grad():
        for n_res in args.lengths:
            toks = synth_tokens(1, n_res, seed=n_res).cuda()
            T = toks.shape[1]
            sides = {"loop": lambda: loop_rows(model, toks), "masked_marginals": lambda: model.masked_marginals(toks)[0]}
            ws = {}
            for side, fn in sides.items():  # warm-up; the workspace each side grows to, from an engine without one
                if model._engine is not None:
                    model._engine.workspace = None
                ref = fn()
                ws[side] = model._engine.workspace.numel()
                sides[side] = (fn, ref)
            diff = (sides["loop"][1].double() - sides["masked_marginals"][1].double()).abs().max().item()
            times = {side: [] for side in sides}
            for _ in range(args.rounds):
                for side, (fn, _) in sides.items():
                    times[side].append(timed(fn)[0])
            med = {side: statistics.median(t) for side, t in times.items()}
            chunk = max(1, 65536 // T)
            out_bytes = {"loop": T * T * V * 4 * 2, "masked_marginals": T * V * 4 * 3}
            lines.append("T = %d (%d residues), chunk %d copies per forward" % (T, n_res, chunk))
            for side in sides:
                lines.append("  %-17s %8.1f ms [%.1f .. %.1f]  %9.0f residues/s   workspace %8.1f MiB   logits + log-prob bytes %10.2f MiB" % (
                    side, 1e3 * med[side], 1e3 * min(times[side]), 1e3 * max(times[side]), T / med[side], ws[side] / 2 ** 20,
                    out_bytes[side] / 2 ** 20))
            lines.append("  ratio loop / masked_marginals: %.2f x; max |difference| of the two tables %.3e" % (
                med["loop"] / med["masked_marginals"], diff))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
