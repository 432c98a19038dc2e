#!/usr/bin/env python
"""Metropolis-Hastings design steps per second: ``model.design`` (esm_amd/design.py: proposal, one energy forward with the
residue rows' log-probabilities and the pinned contact maps, fp64 energy and acceptance on one stream; nothing fetched inside
the loop) against the loop a user writes today on ``forward``, in two forms.  ``host loop, one evaluation``: per step a uniform
site and token per chain from a host generator, ``model(x', contacts_only=True)`` for the maps plus ``model(x')`` for the logits,
the energy (mean negative log-probability of the own residues + cross-entropy of the map against the target over the target
contacts) in torch on the device, the energies brought to the host, the acceptance there, the accepted tokens written back; the
current energy is kept.  ``host loop, two evaluations``: lm-design's form, which evaluates both x and x' every step.

  python tools/design_throughput.py [--model 650M] [--length 254] [--chains 64] [--steps 32] [--rounds 5]
      [--out profiles/design_throughput.log] [--debug-own-groups]

Same model, same process, same number of steps for every side.  One warm-up of each side, then --rounds timed rounds alternating
the sides, each ending in a device synchronise; medians and the spread.  The sides use different random numbers: the sequences
differ, the work per step does not.  ``--debug-own-groups`` adds ``model.design`` with the contact head's head-group count taken
from the batch instead of pinned to that of B = 1 (``esmk_debug_set("rows_contacts_own_groups", 1)`` around the call): what the
pin costs.

  python tools/design_throughput.py --replicas 8 --w-ngram 1 [--baseline-lib OTHER/libesmk.so] [--out profiles/design_tempering.log]

times instead, in the same alternating rounds: the plain call (under ``--baseline-lib``, another build of libesmk.so such as the
parent commit's, and under this one), ladders of K chains with a swap round after every step (``replicas=K``), and the same with
the n-gram term of orders 1 - 3; and then ``esmk_op_ngram_energy`` alone at S = 254 and S = 1022.
"""
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
from esm_amd import sampling  # noqa: E402
from esm_amd.synth import ESM2_DIMS, skip_param_init, synth_esm2_state_dict, synth_tokens  # noqa: E402


def torch_energy(model, toks, contact_mask, n_contacts):
    """fp64 [B] on the device: the energy of ``design`` with the default weights, from two forwards."""
    maps = model(toks, contacts_only=True)["contacts"].double()
    logits = model(toks)["logits"].float()
    lp = torch.log_softmax(logits[:, 1:-1], dim=-1).gather(-1, toks[:, 1:-1].unsqueeze(-1)).squeeze(-1).double()
    e_lm = -lp.mean(dim=1)
    p = maps.clamp(2.0 ** -24, 1.0 - 2.0 ** -24)
    e_contact = -(torch.log(p) * contact_mask).sum(dim=(1, 2)) / n_contacts
    return e_contact + e_lm


def host_loop(model, toks, contact_mask, n_contacts, steps, allowed_idx, rng, two_evaluations):
    state = toks.clone()
    B, T = state.shape
    rows = torch.arange(B, device=state.device)
    e_cur = torch_energy(model, state, contact_mask, n_contacts).cpu().numpy()
    for _ in range(steps):
        site = torch.from_numpy(rng.integers(1, T - 1, B)).to(state.device)
        tok = allowed_idx[torch.from_numpy(rng.integers(0, allowed_idx.numel(), B))].to(state.device)
        proposed = state.clone()
        proposed[rows, site] = tok
        if two_evaluations:
            e_cur = torch_energy(model, state, contact_mask, n_contacts).cpu().numpy()
        e_prop = torch_energy(model, proposed, contact_mask, n_contacts).cpu().numpy()
        accept = rng.random(B) < np.exp(np.minimum(0.0, e_cur - e_prop))
        keep = torch.from_numpy(accept).to(state.device)
        state = torch.where(keep.unsqueeze(1), proposed, state)
        e_cur = np.where(accept, e_prop, e_cur)
    return state


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def tempering_rounds(args, name, dims):
    """``--replicas`` / ``--w-ngram`` / ``--baseline-lib``: the plain call under the baseline library and under this one, ladders of K
    chains with a swap round after every step, and the same with the n-gram term (orders 1 - 3); then ``esmk_op_ngram_energy`` on
    its own at S = 254 and S = 1022."""
    from sample_throughput import library, load_library, make_model

    from esm_amd import _native as N
    from esm_amd import ops
    from esm_amd.design import anneal_ladder, random_sequences
    from esm_amd.ngram import Background

    L, E, H = dims
    model = make_model(L, E, H)
    toks = synth_tokens(args.chains, args.length, seed=1).cuda()
    B, T = toks.shape
    S = args.length
    target = np.triu((np.random.default_rng(3).random((S, S)) < 0.05), 6).astype(np.uint8)
    K = args.replicas or 8
    ladder = anneal_ladder(0.05, 1.0, K)
    bg = Background.from_sequences(random_sequences(200, 300, seed=5), orders=(1, 2, 3))
    w_ngram = args.w_ngram or 1.0
    lines = ["%s (L %d, E %d, H %d) on %s; %d chains, T = %d, %d steps per round, energy = contact cross-entropy (pos) + LM term; "
             "%d rounds after one warm-up, medians [min .. max]" % (name, L, E, H, torch.cuda.get_device_name(0), B, T, args.steps,
                                                                      args.rounds),
             "this library:     %s" % N.lib.esmk_version().decode()]
    sides = {}
    base = base_model = None
    if args.baseline_lib:
        base = load_library(args.baseline_lib)
        with library(base):
            base_model = make_model(L, E, H)
            lines.append("baseline library: %s" % base.esmk_version().decode())

        def baseline():
            with library(base):
                return base_model.design(toks, target, args.steps, seed=7)

        sides["design, baseline library"] = baseline
    sides["design"] = lambda: model.design(toks, target, args.steps, seed=7)
    sides["design, ladders of %d, swap_every 1" % K] = lambda: model.design(toks, target, args.steps, seed=7, replicas=K,
                                                                          temperature=ladder)
    sides["design, ladders of %d + n-gram 1-3" % K] = lambda: model.design(toks, target, args.steps, seed=7, replicas=K,
                                                                         temperature=ladder, w_ngram=w_ngram, ngram=bg)
    with torch.no_grad():
        outs = {side: fn() for side, fn in sides.items()}  # warm-up
        if base is not None:
            same = all(torch.equal(a, b) for a, b in zip(outs["design, baseline library"], outs["design"]))
            lines.append("the plain call under the baseline library and under this one: %s" % (
                "the same tokens and energies" if same else "DIFFERENT results"))
        times = {side: [] for side in sides}
        for _ in range(args.rounds):
            for side, fn in sides.items():
                times[side].append(timed(fn)[0])
    med = {side: statistics.median(t) for side, t in times.items()}
    for side in sides:
        lines.append("  %-40s %8.1f ms [%.1f .. %.1f]  %7.2f steps/s  %6.2f ms/step" % (
            side, 1e3 * med[side], 1e3 * min(times[side]), 1e3 * max(times[side]), args.steps / med[side],
            1e3 * med[side] / args.steps))
    for side in sides:
        if side != "design":
            lines.append("  ratio %s / design: %.4f x" % (side, med[side] / med["design"]))
    # the n-gram op on its own: `reps` launches between two synchronises, per launch
    code = torch.from_numpy(bg.token_codes(model.alphabet)[: model.alphabet_size].copy()).cuda()
    q = {n: torch.from_numpy(t).cuda() for n, t in bg.tables.items()}
    reps = 50
    for length in (254, 1022):
        seqs = synth_tokens(args.chains, length, seed=2).cuda()
        run = lambda: [ops.ngram_energy(seqs, 1, length, code, len(bg.alphabet), q) for _ in range(reps)]  # noqa: E731
        run()
        per = [timed(run)[0] / reps for _ in range(args.rounds)]
        lines.append("  esmk_op_ngram_energy alone, %d chains, S = %4d, orders 1-3: %8.1f us per launch [%.1f .. %.1f] (%d launches per "
                     "round, enqueue included)" % (args.chains, length, 1e6 * statistics.median(per), 1e6 * min(per), 1e6 * max(per), reps))
    if base is not None:  # the baseline model's engine is freed by the library that made it
        import gc

        with library(base):
            base_model = None
            gc.collect()
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="650M")
    ap.add_argument("--length", type=int, default=254, help="residues; T = length + 2")
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--debug-own-groups", action="store_true",
                    help="also time design with the batch's own head-group count (not pinned): the cost of the pin")
    ap.add_argument("--replicas", type=int, default=0, metavar="K",
                    help="time ladders of K chains (replica exchange, a swap round per step) against the plain call instead")
    ap.add_argument("--w-ngram", type=float, default=0.0, help="weight of the n-gram term of the ladder run with it (default 1)")
    ap.add_argument("--baseline-lib", default=None, help="another build of libesmk.so: its plain call is a further side")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("design_throughput: needs the GPU (a CPU run measures nothing)")
    from esm_amd import _native as N

    name = next(k for k in ESM2_DIMS if args.model in k)
    L, E, H = ESM2_DIMS[name]
    if args.replicas or args.w_ngram or args.baseline_lib:
        text = tempering_rounds(args, name, (L, E, H))
        print(text)
        if args.out:
            with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
                fh.write(text + "\n")
        return
    with skip_param_init():
        model = esm.ESM2(L, E, H).eval()
    model.load_state_dict(synth_esm2_state_dict(L, E, H, seed=0))
    model = model.cuda()
    toks = synth_tokens(args.chains, args.length, seed=1).cuda()
    B, T = toks.shape
    S = args.length
    rng0 = np.random.default_rng(3)
    target = np.triu((rng0.random((S, S)) < 0.05), 6).astype(np.uint8)
    contact_mask = torch.from_numpy(target).double().cuda()
    n_contacts = float(target.sum())
    mask = sampling.allowed_mask(model)
    allowed_idx = torch.tensor([v for v in range(model.alphabet_size) if (mask >> v) & 1])
    rng = np.random.default_rng(7)

    def own_groups():
        N.check(N.lib.esmk_debug_set(b"rows_contacts_own_groups", 1.0))
        try:
            return model.design(toks, target, args.steps, seed=7)
        finally:
            N.check(N.lib.esmk_debug_set(b"rows_contacts_own_groups", 0.0))

    sides = {"host loop, two evaluations": lambda: host_loop(model, toks, contact_mask, n_contacts, args.steps, allowed_idx, rng, True),
             "host loop, one evaluation": lambda: host_loop(model, toks, contact_mask, n_contacts, args.steps, allowed_idx, rng, False),
             "design, uniform": lambda: model.design(toks, target, args.steps, seed=7),
             "design, lm": lambda: model.design(toks, target, args.steps, seed=7, proposal="lm")}
    if args.debug_own_groups:
        sides["design, uniform, own groups"] = own_groups
    g = {}
    with torch.cuda.device(toks.device):
        eng = model._engine_ready(toks.device)
        for pinned in (1, 0):
            out = N.ctypes.c_int32()
            N.check(N.lib.esmk_debug_contact_groups(eng.handle, B, T, pinned, N.ctypes.byref(out)))
            g[pinned] = out.value
        ws = eng.rows_contacts_bytes(B, T, B * S)
    lines = ["%s (L %d, E %d, H %d) on %s; %d chains, T = %d, %d steps per round, energy = contact cross-entropy (pos, %d target "
             "contacts) + LM term; %d rounds after one warm-up, medians [min .. max]" % (
                 name, L, E, H, torch.cuda.get_device_name(0), B, T, args.steps, int(n_contacts), args.rounds),
             "head groups of the contact head: %d pinned (B = 1), %d at B = %d; workspace of the pinned energy forward %.2f GiB" % (
                 g[1], g[0], B, ws / 2.0 ** 30)]
    with torch.no_grad():
        for fn in sides.values():
            fn()  # warm-up
        times = {side: [] for side in sides}
        for _ in range(args.rounds):
            for side, fn in sides.items():
                times[side].append(timed(fn)[0])
    med = {side: statistics.median(t) for side, t in times.items()}
    for side in sides:
        lines.append("  %-30s %8.1f ms [%.1f .. %.1f]  %7.2f steps/s  %8.0f proposals/s" % (
            side, 1e3 * med[side], 1e3 * min(times[side]), 1e3 * max(times[side]), args.steps / med[side],
            args.steps * B / med[side]))
    for side in list(sides)[:2]:
        lines.append("  ratio %s / design, uniform: %.2f x" % (side, med[side] / med["design, uniform"]))
    lines.append("  ratio design, lm / design, uniform: %.2f x" % (med["design, lm"] / med["design, uniform"]))
    if args.debug_own_groups:
        lines.append("  ratio design, uniform (pinned) / own groups: %.3f x" % (med["design, uniform"] / med["design, uniform, own groups"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
