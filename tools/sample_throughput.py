#!/usr/bin/env python
"""Gibbs sampling steps per second: ``model.gibbs_sample`` (esm_amd/sampling.py: mask, layer stack, head on the drawn rows, draw
and commit on one stream; nothing fetched inside the loop) against the host loop a user writes on ``forward``, in two forms.
``host loop``: per step mask the chosen positions of every chain, one batched ``model(tokens)``, the full ``[B, T, V]`` logits
brought to the host, ``log_softmax`` of the chosen rows, ``torch.multinomial`` over the allowed tokens with a host generator, the
tokens uploaded again -- the plainest form, and the least favourable one.  ``host loop, device gather``: the same, but the
chosen rows are gathered on the device and only ``[B, per_step, V]`` comes down.

  python tools/sample_throughput.py [--model 650M] [--length 510] [--chains 64] [--per-step 1 8] [--steps 16] [--rounds 5]
      [--out profiles/sampling_throughput.log]
  python tools/sample_throughput.py --order confidence [--top-k K] [--top-p P] [--baseline-lib OTHER/libesmk.so]
      [--out profiles/sampling_confidence.log]

Same model, same process and the same number of steps for every side: every chain gets ``steps * per_step`` designable
positions, so one sweep is ``steps`` steps of ``chains * per_step`` draws.  One warm-up of each side per shape, then --rounds
timed rounds alternating the sides, each ending in a device synchronise; medians and the spread.  The sides draw from the same
distributions with different random numbers: the sequences differ, the work per step does not.

With ``--order`` the tool times ``model.inpaint`` instead: every chain gets ``steps * per_step`` <mask> positions, so filling them
is ``steps`` steps, and the sides are ``order="random"`` (one masked copy per chain and step, head on the drawn rows) and the
given order (head, draw and score on ALL remaining <mask> rows of every step, ``esmk_op_select_rows`` choosing what to commit);
``--top-k`` / ``--top-p`` apply to every side.  ``--baseline-lib`` names another build of libesmk.so (the parent commit's): a
second model is created under it, and ``order="random"`` (without a filter: an older build has none) is timed with that library
as a further side of the same alternating rounds, the library swapped in around each of its calls.
"""
import argparse
import contextlib
import ctypes
import gc
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import esm  # noqa: E402
from esm_amd import sampling  # noqa: E402
from esm_amd.synth import ESM2_DIMS, skip_param_init, synth_esm2_state_dict, synth_tokens  # noqa: E402


def host_loop(model, toks, order, per_step, allowed_idx, gen, device_gather):
    """``order`` int64 [B, steps * per_step] on the host: the positions of every chain in the order visited."""
    state = toks.clone()
    B = state.shape[0]
    rows = torch.arange(B).unsqueeze(1)
    rows_dev = rows.to(state.device)
    for s in range(order.shape[1] // per_step):
        pos = order[:, s * per_step: (s + 1) * per_step]
        pos_dev = pos.to(state.device)
        masked = state.clone()
        masked[rows_dev, pos_dev] = model.mask_idx
        logits = model(masked)["logits"]
        if device_gather:
            chosen = logits[rows_dev, pos_dev].float().cpu()  # [B, per_step, V] on the host
        else:
            chosen = logits.float().cpu()[rows, pos]  # [B, T, V] on the host
        lp = torch.log_softmax(chosen, dim=-1)[..., allowed_idx]
        draw = torch.multinomial(torch.softmax(lp, dim=-1).view(-1, allowed_idx.numel()), 1, generator=gen).view(B, -1)
        state[rows_dev, pos_dev] = allowed_idx[draw].to(state.device)
    return state


def load_library(path):
    """Another build of libesmk.so under the signatures of esm_amd/_native.py (an older build lacks the newest entries)."""
    from esm_amd import _native as N

    lib = ctypes.CDLL(path)
    for name, (res, argtypes) in N.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, argtypes
    return lib


@contextlib.contextmanager
def library(lib):
    """Every engine call inside goes to ``lib`` (esm_amd looks ``_native.lib`` up at call time)."""
    from esm_amd import _native as N

    mine, N.lib = N.lib, lib
    try:
        yield
    finally:
        N.lib = mine


def make_model(L, E, H):
    with skip_param_init():
        model = esm.ESM2(L, E, H).eval()
    model.load_state_dict(synth_esm2_state_dict(L, E, H, seed=0))
    return model.cuda()


def inpaint_rounds(args, name, dims):
    """``--order``: inpaint with the given order against the random order, of this library and of ``--baseline-lib``."""
    L, E, H = dims
    model = make_model(L, E, H)
    toks = synth_tokens(args.chains, args.length, seed=1)
    B, T = toks.shape
    kw = dict(top_k=args.top_k, top_p=args.top_p, seed=7)
    lines = ["%s (L %d, E %d, H %d) on %s; inpaint, %d chains, T = %d, %d steps per round, top_k %d, top_p %g; %d rounds after one "
             "warm-up, medians [min .. max]" % (name, L, E, H, torch.cuda.get_device_name(0), B, T, args.steps, args.top_k,
                                                  args.top_p, args.rounds)]
    base = base_model = None
    if args.baseline_lib:
        base = load_library(args.baseline_lib)
        with library(base):
            base_model = make_model(L, E, H)
            lines.append("baseline library: %s" % base.esmk_version().decode())
        from esm_amd import _native as N

        lines.append("this library:     %s" % N.lib.esmk_version().decode())
    with torch.no_grad():
        for k in args.per_step:
            g = torch.Generator().manual_seed(k)
            start = toks.clone()
            for b in range(B):
                start[b, 1 + torch.randperm(args.length, generator=g)[: args.steps * k]] = model.mask_idx
            start = start.cuda()

            def baseline():
                with library(base):
                    return base_model.inpaint(start, per_step=k, seed=7)  # an older build has no filter: the plain draw

            sides = {}
            if base is not None:
                sides["random, baseline library"] = baseline
            sides["random"] = lambda: model.inpaint(start, per_step=k, **kw)
            sides[args.order] = lambda: model.inpaint(start, per_step=k, order=args.order, **kw)
            outs = {side: fn() for side, fn in sides.items()}  # warm-up
            if base is not None and args.top_k == 0 and args.top_p >= 1.0:  # the same calls under both libraries
                lines.append("per_step = %d: random order, baseline library and this one: %s" % (
                    k, "the same tokens" if torch.equal(outs["random, baseline library"], outs["random"]) else "DIFFERENT tokens"))
            times = {side: [] for side in sides}
            for _ in range(args.rounds):
                for side, fn in sides.items():
                    times[side].append(timed(fn)[0])
            med = {side: statistics.median(t) for side, t in times.items()}
            rows = sum(B * k * (args.steps - s) for s in range(args.steps))
            lines.append("per_step = %d (%d tokens committed per step; %s scores %d rows over the %d steps, random %d)" % (
                k, B * k, args.order, rows, args.steps, B * k * args.steps))
            for side in sides:
                lines.append("  %-25s %8.1f ms [%.1f .. %.1f]  %7.2f steps/s  %8.0f tokens/s" % (
                    side, 1e3 * med[side], 1e3 * min(times[side]), 1e3 * max(times[side]), args.steps / med[side],
                    args.steps * B * k / med[side]))
            for side in list(sides)[:-1]:
                lines.append("  ratio %s / %s: %.3f x" % (args.order, side, med[args.order] / med[side]))
    if base is not None:  # the baseline model's engine is freed by the library that made it
        with library(base):
            base_model = None
            gc.collect()
    return lines


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="650M")
    ap.add_argument("--length", type=int, default=510, help="residues; T = length + 2")
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--per-step", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--steps", type=int, default=16, help="steps per timed round (one sweep over steps * per_step positions)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--order", default=None, choices=("random", "confidence", "entropy"),
                    help="time model.inpaint with this order against the random order instead of the Gibbs comparison")
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--baseline-lib", default=None, help="another build of libesmk.so: its random order is a further side")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_throughput: needs the GPU (a CPU run measures nothing)")
    name = next(k for k in ESM2_DIMS if args.model in k)
    L, E, H = ESM2_DIMS[name]
    if args.order is not None:
        return report(inpaint_rounds(args, name, (L, E, H)), args.out)
    if args.baseline_lib:
        raise SystemExit("sample_throughput: --baseline-lib goes with --order")
    model = make_model(L, E, H)
    toks = synth_tokens(args.chains, args.length, seed=1).cuda()
    B, T = toks.shape
    mask = sampling.allowed_mask(model)
    allowed_idx = torch.tensor([v for v in range(model.alphabet_size) if (mask >> v) & 1])
    lines = ["%s (L %d, E %d, H %d) on %s; %d chains, T = %d, %d steps per round; %d rounds after one warm-up, medians [min .. max]" % (
        name, L, E, H, torch.cuda.get_device_name(0), B, T, args.steps, args.rounds)]
    with torch.no_grad():
        for k in args.per_step:
            g = torch.Generator().manual_seed(k)
            order = torch.stack([1 + torch.randperm(args.length, generator=g)[: args.steps * k] for _ in range(B)])
            positions = [sorted(row.tolist()) for row in order]
            gen = torch.Generator().manual_seed(7)
            sides = {"host loop": lambda: host_loop(model, toks, order, k, allowed_idx, gen, False),
                     "host loop, device gather": lambda: host_loop(model, toks, order, k, allowed_idx, gen, True),
                     "gibbs_sample": lambda: model.gibbs_sample(toks, 1, per_step=k, positions=positions, seed=7,
                                                                top_k=args.top_k, top_p=args.top_p)}
            for fn in sides.values():
                fn()  # warm-up
            times = {side: [] for side in sides}
            for _ in range(args.rounds):
                for side, fn in sides.items():
                    times[side].append(timed(fn)[0])
            med = {side: statistics.median(t) for side, t in times.items()}
            lines.append("per_step = %d (%d draws per step)" % (k, B * k))
            for side in sides:
                lines.append("  %-25s %8.1f ms [%.1f .. %.1f]  %7.2f steps/s  %8.0f draws/s" % (
                    side, 1e3 * med[side], 1e3 * min(times[side]), 1e3 * max(times[side]), args.steps / med[side],
                    args.steps * B * k / med[side]))
            for side in list(sides)[:2]:
                lines.append("  ratio %s / gibbs_sample: %.2f x" % (side, med[side] / med["gibbs_sample"]))
    report(lines, args.out)


def report(lines, out):
    text = "\n".join(lines)
    print(text)
    if out:
        with open(os.path.join(ROOT, out) if not os.path.isabs(out) else out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
