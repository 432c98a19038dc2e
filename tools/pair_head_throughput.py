#!/usr/bin/env python
"""Pair logits of lm-design's 36 + 26 output head per second: ``model.pair_logits`` (esm_amd/pair_head.py: every layer's q, k and
lse kept, one launch of csrc/pair_head.hip over all L*H channels after the last layer) against what a user writes today:
``model(tokens, need_head_weights=True)`` for the [B, L, H, T, T] attention tensor, then the two 1 x 1 projections in torch on the
device (conv1 on P + P^T, conv2 on P, as examples/lm-design/utils/linear_projection.py:119-135).

  python tools/pair_head_throughput.py [--model 650M] [--rounds 5] [--out profiles/pair_head_throughput.log]

Same model, same process.  Shapes: T = 256 x 64 sequences, and T = 1022 at the largest batch of 16, 8, 4, 2, 1 the materialised
side fits.  One warm-up of each side, then --rounds timed rounds alternating the sides, each ending in a device synchronise;
medians and the spread, the peak device bytes of each side, the largest difference between the two outputs, and the head's kernels
alone (the engine's per-class events) against the FLOP bound 2 L H C_out per pair at the 157.3 TF fp32 vector rate.  Then one
``design`` step with a ``DistogramTarget`` against one with a contact target at T = 256 x 64 chains."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import esm  # noqa: E402
from esm_amd import DistogramTarget, PairHead  # noqa: E402
from esm_amd.synth import ESM2_DIMS, skip_param_init, synth_esm2_state_dict, synth_tokens  # noqa: E402

FP32_PEAK = 157.3e12


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def materialised(model, toks, w1, b1, w2, b2):
    """The head on the attention tensor, in torch: [B, S, S, 62]."""
    attn = model(toks, need_head_weights=True)["attentions"]
    B, L, H, T, _ = attn.shape
    a = attn.reshape(B, L * H, T, T)[:, :, 1:-1, 1:-1]
    sym = a + a.transpose(-1, -2)
    out1 = torch.nn.functional.conv2d(sym, w1, b1)
    del sym
    out2 = torch.nn.functional.conv2d(a, w2, b2)
    return torch.cat([out1, out2], 1).permute(0, 2, 3, 1)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(), out


def compare(model, head, convs, toks, rounds, lines):
    B, T = toks.shape
    S = T - 2
    L, H = model.num_layers, model.attention_heads
    sides = {"pair_logits (fused)": lambda: model.pair_logits(toks, head)["all"],
             "attentions + torch projections": lambda: materialised(model, toks, *convs)}
    with torch.no_grad():
        peaks, outs = {}, {}
        for side, fn in sides.items():  # warm-up, peak bytes
            peaks[side], out = peak_of(fn)
            outs[side] = out.float().cpu() if B * S * S * 62 * 4 < (4 << 30) else None
            del out
        times = {side: [] for side in sides}
        for _ in range(rounds):
            for side, fn in sides.items():
                dt, out = timed(fn)
                times[side].append(dt)
                del out
        eng = model._engine
        eng.profile_begin()
        model.pair_logits(toks, head)
        torch.cuda.synchronize()
        prof = {p["name"]: p for p in eng.profile_end()}
    med = {side: statistics.median(t) for side, t in times.items()}
    lines.append("T = %d tokens (S = %d) x %d sequences" % (T, S, B))
    for side in sides:
        lines.append("  %-32s %9.2f ms [%.2f .. %.2f]  %8.1f sequences/s  peak %6.2f GiB" % (
            side, 1e3 * med[side], 1e3 * min(times[side]), 1e3 * max(times[side]), B / med[side], peaks[side] / 2 ** 30))
    a, b = sides
    lines.append("  ratio materialised / fused: %.2f x time, %.2f x peak bytes" % (med[b] / med[a], peaks[b] / peaks[a]))
    if outs[a] is not None and outs[b] is not None:
        lines.append("  largest |fused - materialised| = %.3e (largest |logit| %.2f)" % (
            (outs[a] - outs[b]).abs().max().item(), outs[b].abs().max().item()))
    k_ms = prof["contacts"]["ms"]
    flops = 2.0 * L * H * 62 * B * S * S
    bound_ms = 1e3 * flops / FP32_PEAK
    lines.append("  the head's two kernels alone: %.3f ms for %.1f GFLOP (%.1f TF fp32) against the bound %.3f ms at 157.3 TF: %.2f x" % (
        k_ms, flops / 1e9, flops / k_ms / 1e9, bound_ms, k_ms / bound_ms))
    total = sum(p["ms"] for p in prof.values())
    lines.append("  the whole call under the per-class events: %.2f ms (the forward without the head: %.2f ms)" % (total, total - k_ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="650M")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4, help="design steps per timed call")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pair_head_throughput: needs the GPU (a CPU run measures nothing)")
    from esm_amd import _native as N

    name = next(k for k in ESM2_DIMS if args.model in k)
    L, E, H = ESM2_DIMS[name]
    with skip_param_init():
        model = esm.ESM2(L, E, H).eval()
    model.load_state_dict(synth_esm2_state_dict(L, E, H, seed=0))
    model = model.cuda()
    g = torch.Generator().manual_seed(1)
    C = L * H
    state = {"conv1.weight": torch.randn(36, C, 1, 1, generator=g), "conv1.bias": torch.randn(36, generator=g),
             "conv2.weight": torch.randn(26, C, 1, 1, generator=g), "conv2.bias": torch.randn(26, generator=g)}
    head = PairHead.from_linear_projection({"model": state}, model)
    convs = tuple(state[k].cuda() for k in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"))
    lines = ["%s (L %d, E %d, H %d) on %s; head: 36 symmetric + 26 plain outputs on %d channels (%.1f kFLOP per pair); %d rounds after "
             "one warm-up, medians [min .. max]" % (name, L, E, H, torch.cuda.get_device_name(0), C, 2e-3 * C * 62, args.rounds),
             "library: %s" % N.lib.esmk_version().decode()]
    compare(model, head, convs, synth_tokens(64, 254, seed=1).cuda(), args.rounds, lines)
    for B in (16, 8, 4, 2, 1):  # the largest batch the materialised side fits
        toks = synth_tokens(B, 1020, seed=2).cuda()
        try:
            with torch.no_grad():
                out = materialised(model, toks, *convs)
            del out
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            continue
        compare(model, head, convs, toks, args.rounds, lines)
        break
    # one design step: the distogram term against the contact term
    toks = synth_tokens(64, 254, seed=3).cuda()
    S = 254
    rng = np.random.default_rng(3)
    contact = np.triu(rng.random((S, S)) < 0.05, 6).astype(np.uint8)
    bins = torch.from_numpy(rng.integers(0, 18, (S, S)).astype(np.uint8))
    sides = {"design, contact target": lambda: model.design(toks, contact, args.steps, seed=7),
             "design, DistogramTarget": lambda: model.design(toks, DistogramTarget(bins, head), args.steps, seed=7, min_sep=0)}
    with torch.no_grad():
        for fn in sides.values():
            fn()
        times = {side: [] for side in sides}
        for _ in range(args.rounds):
            for side, fn in sides.items():
                times[side].append(timed(fn)[0])
    lines.append("design, 64 chains of T = 256, %d steps per call (plus the energy of the start)" % args.steps)
    med = {side: statistics.median(t) for side, t in times.items()}
    for side in sides:
        lines.append("  %-32s %9.2f ms [%.2f .. %.2f]  %7.2f ms per energy forward" % (
            side, 1e3 * med[side], 1e3 * min(times[side]), 1e3 * max(times[side]), 1e3 * med[side] / (args.steps + 1)))
    a, b = sides
    lines.append("  ratio DistogramTarget / contact target: %.2f x" % (med[b] / med[a]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
