#!/usr/bin/env python
"""Masked-marginal scoring of one protein LONGER than the model's window: ``model.masked_marginals(tokens, window="max")``
(esm_amd/windows.py: window copies built on the device by ``esmk_op_window_rows``, batches that fill the GPU, the head of the
model on the one masked row of every copy) against the host loop a user writes without it: for every position the tokens sliced
at the same optimal window (``clamp(p - R // 2, lo, hi - R)``), wrapped in <cls> / <eos>, the position masked, one B = 1
``forward`` and ``log_softmax`` of the one row.

  python tools/window_throughput.py [--residues 2500] [--rounds 5] [--out profiles/windows_throughput.log]

An ESM-1b-shaped synthetic model with the dimensions of the 650M checkpoints (L 33, E 1280, H 20, 1024 positions).  Same model and
same process for both sides; one warm-up of each side, then --rounds timed rounds alternating the two sides, each round ending
in a device synchronise; medians and the spread.  Residues/s counts the scored positions (all tokens of the row, <cls> and
<eos> included).  Also recorded: whether the two tables are the same bits (the loop's log_softmax is torch's, so they need not
be) and their largest difference.
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
from esm_amd.synth import skip_param_init, synth_esm1b_state_dict, synth_tokens  # noqa: E402
from esm_amd.windows import geometry, optimal_start  # noqa: E402


def loop_rows(model, toks, window):
    """The loop of a user without ``window=``: one wrapped window per position, one B = 1 forward, one row kept."""
    n = toks.shape[1]
    R, lo, hi = geometry(n, window, True, 1, 1)
    cls, eos = toks[:, :1], toks[:, n - 1:]
    rows = []
    for p in range(n):
        if p < lo:
            s, col = lo, 0
        elif p >= hi:
            s, col = hi - R, window - 1
        else:
            s = optimal_start(p, R, lo, hi)
            col = p - s + 1
        copy = torch.cat([cls, toks[:, s:s + R], eos], dim=1)
        copy[0, col] = model.mask_idx
        rows.append(torch.log_softmax(model(copy)["logits"], dim=-1)[:, col])
    return torch.cat(rows, dim=0)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--residues", type=int, default=2500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_throughput: needs the GPU (a CPU run measures nothing)")
    L, E, H, P = 33, 1280, 20, 1024
    margs = argparse.Namespace(arch="roberta_large", layers=L, embed_dim=E, ffn_embed_dim=4 * E, attention_heads=H, max_positions=P,
                               token_dropout=True, emb_layer_norm_before=True)
    with skip_param_init():
        model = esm.ProteinBertModel(margs, esm.Alphabet.from_architecture("roberta_large")).eval()
    model.load_state_dict(synth_esm1b_state_dict(L, E, H, seed=0, max_positions=P))
    model = model.cuda()
    toks = synth_tokens(1, args.residues, seed=args.residues).cuda()
    n = toks.shape[1]
    with torch.no_grad():
        model(toks[:, :30].contiguous())  # the engine exists from here on: its LayerNorm-fold mode can be read
        sides = {"loop": lambda: loop_rows(model, toks, P), "masked_marginals(window)": lambda: model.masked_marginals(toks, window="max")[0]}
        ref = {side: fn() for side, fn in sides.items()}  # warm-up of both sides; their tables
        same = torch.equal(ref["loop"], ref["masked_marginals(window)"])
        diff = (ref["loop"].double() - ref["masked_marginals(window)"].double()).abs().max().item()
        times = {side: [] for side in sides}
        for _ in range(args.rounds):
            for side, fn in sides.items():
                times[side].append(timed(fn)[0])
    med = {side: statistics.median(t) for side, t in times.items()}
    lines = ["ESM-1b-shaped synthetic model (L %d, E %d, H %d, %d positions) on %s; LayerNorm fold %s; %d rounds after one warm-up, "
             "medians [min .. max]" % (L, E, H, P, torch.cuda.get_device_name(0), "on" if model.ln_fold_active() else "off", args.rounds),
             "one protein of %d residues (%d tokens), windows of %d tokens, chunk %d copies per forward" % (
                 args.residues, n, P, max(1, 65536 // P))]
    for side in sides:
        lines.append("  %-25s %9.1f ms [%.1f .. %.1f]  %9.0f residues/s" % (
            side, 1e3 * med[side], 1e3 * min(times[side]), 1e3 * max(times[side]), n / med[side]))
    lines.append("  ratio loop / masked_marginals(window): %.2f x; tables %s (max |difference| %.3e)" % (
        med["loop"] / med["masked_marginals(window)"], "bit-identical" if same else "differ in the log_softmax", diff))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
