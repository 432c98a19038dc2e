#!/usr/bin/env python
"""SAE features of a library: ``model.sae_features`` (esm_amd/sae.py: per chunk the f16x3 operand image, the dense GEMM, the
row-wise top-k and the per-sequence maximum on one stream, no [n, F] matrix beyond a chunk of scratch) against the loop a user
writes today on this project: ``forward(repr_layers=[layer])``, then ``relu((rep - b_dec) @ W.T + b_enc)``, ``torch.topk`` and
``amax`` per sequence in fp32 torch on the device, chunked over rows only as far as ``--baseline-bytes`` forces it.

  python tools/sae_throughput.py [--model esm2_t33_650M_UR50D] [--layer 24] [--features 10240 65536] [--shapes 64x1022 64x256]
      [--top-k 32] [--rounds 5] [--out profiles/sae_throughput.log]

Synthetic weights (esm_amd/synth.py) and a random SAE whose encoder bias is set from the measured spread of z so that about
``--active`` of the features fire per row (real dictionaries: tens to a few hundred of 10^4); ``--active 0.5`` is the dense
worst case of the selection.  Same model, same process; one warm-up of every side, then --rounds timed rounds alternating the
sides, each ending in a device synchronise; medians [min .. max].  Reported per (F, shape): both sides, the forward alone, the
SAE launches alone (on a captured representation), peak bytes above the model on both sides, the largest difference of the
top-k values and the share of rows whose index sets differ (torch's fp32 products are rounded differently: differences at
near-ties are expected; reported, not asserted)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import esm  # noqa: E402
from esm_amd import SparseAutoencoder, ops  # noqa: E402
from esm_amd import sae as S  # noqa: E402
from esm_amd.synth import ESM2_DIMS, skip_param_init, synth_esm2_state_dict, synth_tokens  # noqa: E402


def make_model(L, E, H):
    with skip_param_init():
        model = esm.ESM2(L, E, H).eval()
    model.load_state_dict(synth_esm2_state_dict(L, E, H, seed=0))
    return model.cuda()


def make_sae(model, toks, layer, F, active, seed=0):
    """a random SAE (tied, row-normalised decoder); b_enc = -q sigma_f with q the normal quantile of ``active`` and sigma_f the
    spread of feature f's pre-activation over the rows of one sequence batch"""
    E = model.embed_dim
    g = torch.Generator().manual_seed(seed + F)
    w_enc = torch.randn(F, E, generator=g) / E ** 0.5
    w_dec = w_enc / w_enc.norm(dim=1, keepdim=True)
    b_dec = 0.1 * torch.randn(E, generator=g)
    rep = model(toks[:2], repr_layers=[layer])["representations"][layer][:, 1:-1].reshape(-1, E).float()
    z = (rep - b_dec.cuda()) @ w_enc.cuda().t()
    q = float(torch.distributions.Normal(0.0, 1.0).icdf(torch.tensor(1.0 - active)))
    b_enc = (-z.mean(0) - q * z.std(0)).cpu()
    return SparseAutoencoder(w_enc, b_enc, w_dec, b_dec)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def peak_above(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def torch_side(model, toks, layer, dev_sae, top_k, max_bytes, rep=None):
    """the loop a user writes today; (values [n, k], indices [n, k], protein max [B, F])"""
    if rep is None:
        rep = model(toks, repr_layers=[layer])["representations"][layer]
    B, T, E = rep.shape
    w, b_enc, b_dec = dev_sae
    F = w.shape[0]
    x = rep[:, 1:-1]
    seqs = max(1, min(B, int(max_bytes // ((T - 2) * F * 4))))  # whole sequences per chunk: amax stays a plain reduction
    vals, idxs, pmax = [], [], []
    for lo in range(0, B, seqs):
        acts = torch.relu((x[lo:lo + seqs] - b_dec) @ w.t() + b_enc)
        v, i = torch.topk(acts, top_k, dim=-1)
        vals.append(v.reshape(-1, top_k))
        idxs.append(i.reshape(-1, top_k))
        pmax.append(acts.amax(dim=1))
    return torch.cat(vals), torch.cat(idxs), torch.cat(pmax)


def fmt(ts):
    return "%8.2f ms [%7.2f .. %7.2f]" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts))


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--model", default="esm2_t33_650M_UR50D", choices=sorted(ESM2_DIMS))
    p.add_argument("--layer", type=int, default=24)
    p.add_argument("--features", type=int, nargs="+", default=[10240, 65536])
    p.add_argument("--shapes", nargs="+", default=["64x1022", "64x256"], help="B x T, T with <cls> and <eos>")
    p.add_argument("--top-k", type=int, default=32)
    p.add_argument("--active", type=float, nargs="+", default=[0.01], help="share of the features that fire per row")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--max-bytes", type=int, default=2 << 30, help="sae_features' scratch budget")
    p.add_argument("--baseline-bytes", type=int, default=64 << 30, help="the torch side's [rows, F] fp32 matrix per chunk")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sae_throughput: needs the GPU (a timing taken anywhere else says nothing)")
    L, E, H = ESM2_DIMS[args.model]
    model = make_model(L, E, H)
    lines = ["%s (L %d, E %d, H %d) on %s; SAE on representation %d, top_k %d, protein_max on, positions residues; %d rounds after one "
             "warm-up, alternating, medians [min .. max]; LDS candidates %d"
             % (args.model, L, E, H, torch.cuda.get_device_name(0), args.layer, args.top_k, args.rounds, ops.sae_cand())]
    for shape in args.shapes:
        B, T = (int(v) for v in shape.split("x"))
        toks = synth_tokens(B, T - 2, seed=1).cuda()
        for F in args.features:
            for active in args.active:
                sae = make_sae(model, toks, args.layer, F, active)
                dev_sae = (sae.w_enc.cuda(), sae.b_enc.cuda(), sae.b_dec.cuda())
                rep = model(toks, repr_layers=[args.layer])["representations"][args.layer]
                rows = S.scored_rows(model, toks, "residues")
                sides = {
                    "sae_features": lambda: model.sae_features(toks, sae, args.layer, top_k=args.top_k, protein_max=True,
                                                               max_bytes=args.max_bytes),
                    "torch loop": lambda: torch_side(model, toks, args.layer, dev_sae, args.top_k, args.baseline_bytes),
                    "forward alone": lambda: model(toks, repr_layers=[args.layer]),
                    "SAE launches alone": lambda: S.features_of_rows(sae, rep, rows, args.top_k, protein_max=True,
                                                                     max_bytes=args.max_bytes),
                    "torch SAE alone": lambda: torch_side(model, toks, args.layer, dev_sae, args.top_k, args.baseline_bytes, rep=rep),
                }
                times = {name: [] for name in sides}
                for fn in sides.values():
                    fn()
                for _ in range(args.rounds):
                    for name, fn in sides.items():
                        times[name].append(timed(fn)[0])
                peak_e, ours = peak_above(sides["sae_features"])
                peak_t, (tv, ti, tmax) = peak_above(sides["torch loop"])
                n = ours["rows"].shape[0]
                n_act = ours["n_active"].float()
                ti = torch.where(tv > 0, ti, torch.full_like(ti, -1))  # unused slots as sae_features reports them
                dv = (ours["values"] - tv).abs().max().item()
                differ = (ours["indices"].long().sort(dim=1).values != ti.sort(dim=1).values).any(dim=1).float().mean().item()
                dmax = (ours["protein_max"] - tmax).abs().max().item()
                chunks = len(S.plan_chunks(n, F, E, args.max_bytes))
                lines.append("")
                lines.append("F = %d, B x T = %d x %d (%d rows, %d chunk%s), %.3g of the features wanted active: mean n_active %.1f, "
                             "max %d, %.2f %% of the rows above the LDS candidates (radix select)"
                             % (F, B, T, n, chunks, "" if chunks == 1 else "s", active, n_act.mean().item(), int(n_act.max().item()),
                                100.0 * (n_act > ops.sae_cand()).float().mean().item()))
                for name in sides:
                    lines.append("    %-20s %s" % (name, fmt(times[name])))
                lines.append("    peak bytes above the model: sae_features %.2f GB, torch loop %.2f GB" % (peak_e / 1e9, peak_t / 1e9))
                lines.append("    top-k values: largest difference %.3e; rows whose index sets differ %.3f %%; protein_max largest "
                             "difference %.3e" % (dv, 100.0 * differ, dmax))
                print("\n".join(lines[-9:]), flush=True)
                sides = sae = dev_sae = rep = ours = tv = ti = tmax = None
                torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
