#!/usr/bin/env python
"""Padded vs token-packed forward on a mixed-length workload.

Sequence lengths are drawn from a log-normal fitted to UniRef50-like proteins (median ~270 residues, clipped to
[30, 1022]); batches are formed the way the reference does it (esm/data.py:get_batch_indices: sort by length,
fill up to toks_per_batch) or in file order (--unsorted; what a streaming service sees).  Reports REAL residues
per second (pad positions do not count) for model.forward and model.forward_varlen on the same batches.

  python tools/bench_varlen.py --model 650M --n 2048 --toks-per-batch 65536
  python tools/bench_varlen.py --model 650M --contacts [--unsorted]   # contact maps: forward(contacts_only=True)
                                                                       # vs forward_varlen(contacts_only=True)
  python tools/bench_varlen.py --model 650M --maps                     # attention maps: forward(need_head_weights)
                                                                       # vs forward_varlen(need_head_weights, unpack=False)
With --contacts the engine workspace each path grew to (its peak over the batches) is reported as well.
--maps measures two batches, every variant inside this one process, --rounds timed rounds after one warm-up each, medians:
  mixed    the first sequences of the length mix in file order, as many as keep the PADDED fp32 maps [B,L,H,Tmax,Tmax]
           under --maps-gib: step time and peak device memory of both paths (torch.cuda.max_memory_allocated over one
           call that starts without an engine workspace: the workspace is a torch tensor, so the figure holds it, the
           outputs and the parameters);
  uniform  --uniform-b sequences of 1022 residues, where packing saves nothing: the time of the map kernel class alone
           (the engine's per-class HIP-event timing), packed / padded, next to the spread of the padded rounds.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import esm  # noqa: E402
from esm_amd.synth import ESM2_DIMS, synth_esm2_state_dict  # noqa: E402


def uniref_like_lengths(n, g):
    """n residue counts of the UniRef50-like length mix (module docstring), drawn from the generator ``g``."""
    return torch.exp(torch.randn(n, generator=g) * 0.7 + 5.6).clamp(30, 1022).long().tolist()


def make_batches(lengths, toks_per_batch, sort):
    order = sorted(range(len(lengths)), key=lambda i: lengths[i]) if sort else list(range(len(lengths)))
    batches, cur, mx = [], [], 0
    for i in order:
        n = lengths[i] + 2
        if cur and max(mx, n) * (len(cur) + 1) > toks_per_batch:
            batches.append(cur)
            cur, mx = [], 0
        cur.append(i)
        mx = max(mx, n)
    if cur:
        batches.append(cur)
    return batches


def _tokens(lengths, g):
    t = torch.full((len(lengths), max(lengths) + 2), 1, dtype=torch.int64)
    for r, n in enumerate(lengths):
        t[r, 0] = 0
        t[r, 1:n + 1] = torch.randint(4, 24, (n,), generator=g)
        t[r, n + 1] = 2
    return t


def bench_maps(model, name, L, H, args):
    import statistics

    g = torch.Generator().manual_seed(args.seed)
    mix = uniref_like_lengths(args.n, g)
    # mixed batch: file order, the largest prefix whose padded fp32 maps stay inside the budget
    lengths = []
    for n in mix:
        cand = lengths + [n]
        if len(cand) * L * H * (max(cand) + 2) ** 2 * 4 > args.maps_gib * 2 ** 30:
            break
        lengths = cand
    toks = _tokens(lengths, g)
    B, T = toks.shape
    real2 = sum((n + 2) ** 2 for n in lengths)
    print("%s (L %d, H %d), fold %s" % (name, L, H, os.environ.get("ESM_AMD_LN_FOLD", "default")))
    print("mixed batch: %d sequences, lengths %d..%d (median %d), T = %d; fp32 maps padded %.2f GiB, ragged %.2f GiB" % (
        B, min(lengths) + 2, T, sorted(lengths)[B // 2] + 2, T, B * L * H * T * T * 4 / 2 ** 30, L * H * real2 * 4 / 2 ** 30))

    def timed(fn, rounds):
        out = []
        with torch.no_grad():
            fn()  # warm-up: allocations, workspace growth, table uploads
            torch.cuda.synchronize()
            for _ in range(rounds):
                t0 = time.perf_counter()
                r = fn()
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
                del r
        return out

    def peak(fn):
        model.refresh_engine()  # drops both workspaces (and the packed image, re-packed by the call below)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        with torch.no_grad():
            r = fn()
            torch.cuda.synchronize()
        del r
        return torch.cuda.max_memory_allocated() / 2 ** 30

    dev = toks.cuda()
    padded = lambda: model(dev, need_head_weights=True)
    packed = lambda: model.forward_varlen(toks, min_saving=None, unpack=False, need_head_weights=True)
    with torch.no_grad():
        model(dev[:1, :8])
    t_pad, t_pk = timed(padded, args.rounds), timed(packed, args.rounds)
    m_pad, m_pk = peak(padded), peak(packed)
    med = statistics.median
    print("  padded forward(need_head_weights)                      : %8.1f ms (min %.1f max %.1f)  peak %6.2f GiB" % (
        med(t_pad), min(t_pad), max(t_pad), m_pad))
    print("  packed forward_varlen(need_head_weights, unpack=False) : %8.1f ms (min %.1f max %.1f)  peak %6.2f GiB  (%.2fx time, %.2fx memory)" % (
        med(t_pk), min(t_pk), max(t_pk), m_pk, med(t_pad) / med(t_pk), m_pad / m_pk))

    # uniform batch: equal full-length sequences, the map kernel class alone
    ub = args.uniform_b
    utoks = _tokens([1022] * ub, g)
    udev = utoks.cuda()

    def probs_ms(fn):
        out = []
        with torch.no_grad():
            fn()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                model.profile_begin()
                r = fn()
                prof = model.profile_end()
                del r
                out.append(sum(e["ms"] for e in prof if e["name"] == "attention_probs"))
        return out

    upad = lambda: model(udev, need_head_weights=True)
    upk = lambda: model.forward_varlen(utoks, min_saving=None, unpack=False, need_head_weights=True)
    a1, b1, a2, b2 = probs_ms(upad), probs_ms(upk), probs_ms(upad), probs_ms(upk)  # interleaved: A B A B
    pa, pb = a1 + a2, b1 + b2
    spread = (max(pa) - min(pa)) / med(pa)
    print("uniform batch: %d x 1024 tokens, map kernels of %d layers (HIP events, %d rounds per variant)" % (ub, L, len(pa)))
    print("  padded attention_probs : %8.3f ms (min %.3f max %.3f, spread %.1f %%; first / second block median %.3f / %.3f)" % (
        med(pa), min(pa), max(pa), 100 * spread, med(a1), med(a2)))
    print("  packed attention_probs : %8.3f ms (min %.3f max %.3f)  packed / padded = %.3f" % (
        med(pb), min(pb), max(pb), med(pb) / med(pa)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="650M")
    ap.add_argument("--n", type=int, default=2048, help="number of sequences")
    ap.add_argument("--toks-per-batch", type=int, default=65536)
    ap.add_argument("--unsorted", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--contacts", action="store_true", help="time the contact-map paths instead of the logits ones")
    ap.add_argument("--maps", action="store_true", help="time the attention-map paths (see the module docstring)")
    ap.add_argument("--maps-gib", type=float, default=32.0, help="--maps: budget for the padded fp32 maps of the mixed batch")
    ap.add_argument("--uniform-b", type=int, default=8, help="--maps: sequences of the uniform batch")
    ap.add_argument("--rounds", type=int, default=7, help="--maps: timed rounds per variant")
    args = ap.parse_args()
    name = next(k for k in ESM2_DIMS if k == args.model or k.split("_")[2] == args.model)
    L, E, H = ESM2_DIMS[name]
    model = esm.ESM2(L, E, H).eval()
    model.load_state_dict(synth_esm2_state_dict(L, E, H, seed=0))
    model = model.cuda()

    if args.maps:
        return bench_maps(model, name, L, H, args)

    g = torch.Generator().manual_seed(args.seed)
    lengths = uniref_like_lengths(args.n, g)
    batches = make_batches(lengths, args.toks_per_batch, not args.unsorted)
    toks = []
    for idx in batches:
        T = max(lengths[i] for i in idx) + 2
        t = torch.full((len(idx), T), 1, dtype=torch.int64)
        for r, i in enumerate(idx):
            n = lengths[i]
            t[r, 0] = 0
            t[r, 1:n + 1] = torch.randint(4, 24, (n,), generator=g)
            t[r, n + 1] = 2
        toks.append(t)
    real = sum(n + 2 for n in lengths)
    padded = sum(t.numel() for t in toks)
    print("%d sequences, %d batches, %d real tokens, %d padded (%.1f %% padding), batching %s" % (
        args.n, len(batches), real, padded, 100.0 * (padded - real) / padded, "file order" if args.unsorted else "sorted"))

    def run(fn):
        with torch.no_grad():
            fn(toks[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in toks:
                fn(t)
            torch.cuda.synchronize()
        return time.perf_counter() - t0

    if args.contacts:
        def peak(fn):
            if model._engine is not None:
                model._engine.workspace = None  # each path grows its own workspace from empty
            torch.cuda.empty_cache()
            t = run(fn)
            return t, model._engine.workspace.numel()

        t_pad, w_pad = peak(lambda t: model(t.cuda(), repr_layers=[L], contacts_only=True))
        t_var, w_var = peak(lambda t: model.forward_varlen(t, repr_layers=[L], contacts_only=True, min_saving=None))
        print("contacts padded  forward(contacts_only)        : %8.1f ms  %9.0f real residues/s  workspace %6.0f MiB" % (
            t_pad * 1e3, real / t_pad, w_pad / 2**20))
        print("contacts packed  forward_varlen(contacts_only) : %8.1f ms  %9.0f real residues/s  workspace %6.0f MiB  (%.2fx)" % (
            t_var * 1e3, real / t_var, w_var / 2**20, t_pad / t_var))
        return
    t_pad = run(lambda t: model(t.cuda(), repr_layers=[L]))
    t_var = run(lambda t: model.forward_varlen(t, repr_layers=[L]))
    t_raw = run(lambda t: model.forward_varlen(t, repr_layers=[L], unpack=False))
    print("padded  forward        : %8.1f ms  %9.0f real residues/s" % (t_pad * 1e3, real / t_pad))
    print("packed  forward_varlen : %8.1f ms  %9.0f real residues/s  (%.2fx)" % (t_var * 1e3, real / t_var, t_pad / t_var))
    print("packed, no unpack      : %8.1f ms  %9.0f real residues/s  (%.2fx)" % (t_raw * 1e3, real / t_raw, t_pad / t_raw))


if __name__ == "__main__":
    main()
