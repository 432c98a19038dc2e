#!/usr/bin/env python
"""The categorical-Jacobian contact map of one protein: ``model.jacobian_contacts`` (esm_amd/jacobian.py: the L x 20 substituted
copies built on the device, batches that fill the GPU, the head of the model on the residue rows, the logit differences
scattered straight into J, centring / reduction / APC by the engine's kernels) against the loop a user writes on ``forward``:
one B = 20 forward per position, the ``[20, T, V]`` logits sliced on the device, then centring, symmetrising, the norm over
(a, b) and the APC with torch on the device.

  python tools/jacobian_throughput.py [--model 650M] [--lengths 256 512] [--rounds 5] [--out profiles/jacobian_throughput.log]

Same protein and same process for both sides; one warm-up of each side per length, then --rounds timed rounds alternating the
two sides, each round ending in a device synchronise; medians and the spread.  Copies/s counts the L x 20 substituted
sequences, residues/s their tokens through the layer stack.  Also recorded: the time of the engine's post-processing alone
(centre + contacts + APC on a J that is already there), the peak device memory of each side above the model, and the largest
difference between the two maps (the loop centres and reduces in fp32 with torch's own reduction orders).
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
from esm_amd import ops  # noqa: E402
from esm_amd.jacobian import candidate_columns  # noqa: E402
from esm_amd.scoring import CHUNK_TOKENS  # noqa: E402
from esm_amd.synth import ESM2_DIMS, skip_param_init, synth_esm2_state_dict, synth_tokens  # noqa: E402


def loop_contacts(model, toks, cols):
    """What a user writes on ``forward``: one B = nA forward per position, everything after it with torch on the device."""
    T = toks.shape[1]
    L, nA = T - 2, cols.numel()
    wt = model(toks)["logits"][0, 1:-1].float()[:, cols]
    J = torch.empty((L, nA, L, nA), dtype=torch.float32, device=toks.device)
    for i in range(L):
        batch = toks.repeat(nA, 1)
        batch[:, 1 + i] = cols
        J[i] = model(batch)["logits"][:, 1:-1].float()[:, :, cols] - wt
    for axis in (3, 2, 1, 0):
        J -= J.mean(dim=axis, keepdim=True)
    S = (0.5 * (J + J.permute(2, 3, 0, 1))).pow(2).sum(dim=(1, 3)).sqrt()
    S.fill_diagonal_(0.0)
    total = S.sum()
    C = S - S.sum(dim=1, keepdim=True) * S.sum(dim=0, keepdim=True) / total
    C.fill_diagonal_(0.0)
    return C


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def peak_above(fn, base):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="650M")
    ap.add_argument("--lengths", type=int, nargs="+", default=[256, 512], help="residues; T = length + 2")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jacobian_throughput: needs the GPU (a CPU run measures nothing)")
    name = next(k for k in ESM2_DIMS if args.model in k)
    L_, E, H = ESM2_DIMS[name]
    with skip_param_init():
        model = esm.ESM2(L_, E, H).eval()
    model.load_state_dict(synth_esm2_state_dict(L_, E, H, seed=0))
    model = model.cuda()
    cols = torch.tensor(candidate_columns(model), device="cuda")
    nA = cols.numel()
    lines = []
    with torch.no_grad():
        model(synth_tokens(1, 30).cuda())  # the engine exists from here on: its LayerNorm-fold mode can be read
        lines.append("%s (L %d, E %d, H %d) on %s; LayerNorm fold %s; %d rounds after one warm-up, medians [min .. max]" % (
            name, L_, E, H, torch.cuda.get_device_name(0), "on" if model.ln_fold_active() else "off", args.rounds))
        for n_res in args.lengths:
            toks = synth_tokens(1, n_res, seed=n_res).cuda()
            T = toks.shape[1]
            sides = {"loop": lambda: loop_contacts(model, toks, cols), "jacobian_contacts": lambda: model.jacobian_contacts(toks)}
            ref, peak = {}, {}
            for side, fn in sides.items():  # warm-up (the engine workspace grows here), then the peak of a second run
                fn()
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                ref[side], peak[side] = peak_above(fn, base)
            diff = (ref["loop"].double() - ref["jacobian_contacts"].double()).abs().max().item()
            scale = ref["jacobian_contacts"].abs().max().item()
            times = {side: [] for side in sides}
            for r in range(args.rounds):
                for side, fn in sides.items():
                    times[side].append(timed(fn)[0])
                lines.append("  round %d: loop %9.1f ms   jacobian_contacts %9.1f ms" % (
                    r, 1e3 * times["loop"][-1], 1e3 * times["jacobian_contacts"][-1]))
            J = model.categorical_jacobian(toks)
            post = statistics.median(timed(lambda: ops.apc(ops.jacobian_contacts(ops.jacobian_center(J))))[0] for _ in range(3))
            del J
            med = {side: statistics.median(t) for side, t in times.items()}
            copies = n_res * nA
            lines.append("T = %d (%d residues), %d copies, J = %.2f GB; engine chunk %d copies per forward, loop %d" % (
                T, n_res, copies, n_res * n_res * nA * nA * 4 / 1e9, max(1, CHUNK_TOKENS // T), nA))
            for side in sides:
                lines.append("  %-17s %9.1f ms [%.1f .. %.1f]  %8.0f copies/s  %9.0f residues/s   peak memory above the model %8.1f MiB" % (
                    side, 1e3 * med[side], 1e3 * min(times[side]), 1e3 * max(times[side]), copies / med[side],
                    copies * T / med[side], peak[side] / 2 ** 20))
            spread = {side: max(t) - min(t) for side, t in times.items()}
            gain = med["loop"] - med["jacobian_contacts"]
            bound = max(spread.values())
            lines.append("  ratio loop / jacobian_contacts: %.2f x; loop - jacobian_contacts = %+.1f ms; spread (max - min) of the %d "
                         "rounds: loop %.1f ms, jacobian_contacts %.1f ms" % (
                             med["loop"] / med["jacobian_contacts"], 1e3 * gain, args.rounds, 1e3 * spread["loop"],
                             1e3 * spread["jacobian_contacts"]))
            lines.append("  engine post-processing alone (centre + contacts + APC): %.1f ms; max |difference| of the two maps %.3e "
                         "(largest |entry| %.3e)" % (1e3 * post, diff, scale))
            lines.append("  verdict: jacobian_contacts is %s (%+.1f ms against a spread of %.1f ms, the larger of the two sides)" % (
                "FASTER than the loop beyond the spread of the rounds" if gain > bound
                else "SLOWER than the loop beyond the spread of the rounds" if -gain > bound
                else "NOT DISTINGUISHABLE from the loop: the difference is inside the spread of the rounds", 1e3 * gain, 1e3 * bound))
            del ref
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
