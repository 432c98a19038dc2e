#!/usr/bin/env python
"""Masked-marginal scoring of one protein: ``model.masked_marginals`` (esm_amd/scoring.py: masked copies built on the device,
batches that fill the GPU, the head of the model on the one masked row of every copy) against the reference's loop
(examples/variant-prediction/predict.py:205-215) written on the same model's ``forward``: T forwards at B = 1, each building
[1, T, V] logits and keeping one row.

  python tools/score_throughput.py [--model 650M] [--lengths 510 1020] [--rounds 5] [--out profiles/scoring_throughput.log]
  python tools/score_throughput.py --variants 512 [--lengths 510] --out profiles/scoring_variants.log
  python tools/score_throughput.py --msa [--msa-shapes 16x257 400x301] --out profiles/msa_scoring_throughput.log

  python tools/score_throughput.py --varlen-library 256 --out profiles/scoring_varlen.log

Same library and same process for both sides; one warm-up of each side per shape, then --rounds timed rounds alternating the
two sides, each round ending in a device synchronise; medians and the spread.  Residues/s counts the scored positions (all T
tokens of the row).  Also recorded: the engine workspace each side grew to, the bytes of logits / log-probabilities each side
writes over the whole protein, and the largest difference between the two tables (the loop's log_softmax is torch's).

--variants N: N random double mutants of one protein ('A42G:K50R' rows of a deep mutational scan) scored with the
masked-marginal score of the ESM-1v paper (both positions masked in one forward, log p(mt) - log p(wt) summed over them):
``model.score_variants`` (joint masks built on the device, batches that fill the GPU, the head on the masked rows, the sums
by ``esmk_op_score_rows``) against what a user had before it: one B = 1 ``model.forward`` per distinct position set,
log_softmax of its logits, the two rows kept, the terms summed on the host.  Variants/s counts the scored table rows.

--msa: masked marginals of the first row of one MSA with the MSA Transformer (dimensions of esm_msa1b_t12_100M):
``model.msa_masked_marginals`` (esm_amd/msa_scoring.py: masked copies of the MSA batched until the GPU is full, the head on
the one masked cell of every copy) against the reference's MSA loop (predict.py:167-178) on the same model's ``forward``: C
forwards at B = 1, each building [1, R, C, V] logits and keeping one cell.  Two shapes R x C: a shallow MSA, where batching
should pay, and a deep one at the reference's default scale (--msa-samples 400), where one copy already fills the GPU and
what remains is the smaller head and the logits tensor that is not built.

--varlen-library N: the pseudo-log-likelihood of a library of N sequences of DIFFERENT lengths (N draws, seeded, from the
UniRef-like length mix of tools/bench_varlen.py: log-normal, median ~270 residues, clipped to [30, 1022], in file order):
``model.pseudo_log_likelihood(tokens, varlen=True)`` (masked copies token-packed, each as long as its own sequence) against
``varlen=False`` (every copy padded to the longest sequence of its call) on the same model, --library-per-call sequences per
call as ``python -m esm_amd.score_sequences`` makes them.  Every round of both sides is printed, with the medians and the
spread; a ratio inside the spread of the rounds is reported as such, not as a gain.
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


def random_doubles(seq, n, seed):
    """n double mutants of ``seq`` in 1-based numbering, positions and mutant residues uniformly at random."""
    g = torch.Generator().manual_seed(seed)
    letters = "ACDEFGHIKLMNPQRSTVWY"
    out = []
    for _ in range(n):
        i, j = sorted(torch.randperm(len(seq), generator=g)[:2].tolist())
        parts = []
        for idx in (i, j):
            choice = [c for c in letters if c != seq[idx]]
            parts.append("%s%d%s" % (seq[idx], idx + 1, choice[int(torch.randint(0, len(choice), (1,), generator=g))]))
        out.append(":".join(parts))
    return out


def loop_variant_scores(model, alphabet, toks, variants):
    """One B = 1 forward per distinct position set (first appearance first), log_softmax of its logits, the set's rows kept;
    fp32 terms gathered on the device, summed per variant on the host in fp64."""
    from esm_amd.scoring import parse_variant

    parsed = [sorted(parse_variant(v, 1), key=lambda part: part[1]) for v in variants]
    first_row, rows, n_rows = {}, [], 0
    for parts in parsed:
        key = tuple(1 + idx for _, idx, _ in parts)
        if key in first_row:
            continue
        first_row[key] = n_rows
        n_rows += len(key)
        masked = toks.clone()
        masked[0, list(key)] = model.mask_idx
        rows.append(torch.log_softmax(model(masked)["logits"], dim=-1)[0, list(key)])
    table = torch.cat(rows, dim=0)
    idx = torch.tensor([first_row[tuple(1 + i for _, i, _ in parts)] + j for parts in parsed for j in range(len(parts))])
    wt = torch.tensor([alphabet.get_idx(w) for parts in parsed for w, _, _ in parts])
    mt = torch.tensor([alphabet.get_idx(m) for parts in parsed for _, _, m in parts])
    sub = table[idx.to(table.device)]
    terms = (sub.gather(1, mt.to(table.device).unsqueeze(1)) - sub.gather(1, wt.to(table.device).unsqueeze(1))).view(-1).tolist()
    scores, at = [], 0
    for parts in parsed:
        scores.append(sum(terms[at:at + len(parts)], 0.0))
        at += len(parts)
    return scores


def variants_mode(args, model):
    """--variants N: the lines of the report, one block per length."""
    from esm_amd.scoring import CHUNK_TOKENS, parse_variant

    alphabet = esm.Alphabet.from_architecture("ESM-1b")
    lines = []
    with torch.no_grad():
        for n_res in args.lengths:
            toks = synth_tokens(1, n_res, seed=n_res)
            seq = "".join(alphabet.get_tok(int(t)) for t in toks[0, 1:-1])
            toks = toks.cuda()
            T = toks.shape[1]
            variants = random_doubles(seq, args.variants, seed=n_res)
            sides = {"loop": lambda: loop_variant_scores(model, alphabet, toks, variants),
                     "score_variants": lambda: model.score_variants(alphabet, seq, variants, offset_idx=1)}
            n_sets = len({tuple(sorted(idx for _, idx, _ in parse_variant(v, 1))) for v in variants})
            ref = {side: fn() for side, fn in sides.items()}  # warm-up of both sides; their scores
            diff = max(abs(a - b) for a, b in zip(ref["loop"], ref["score_variants"]))
            times = {side: [] for side in sides}
            for _ in range(args.rounds):
                for side, fn in sides.items():
                    times[side].append(timed(fn)[0])
            med = {side: statistics.median(t) for side, t in times.items()}
            lines.append("T = %d (%d residues), %d random double mutants, %d distinct position sets, chunk %d copies per forward" % (
                T, n_res, len(variants), n_sets, max(1, CHUNK_TOKENS // T)))
            for side in sides:
                lines.append("  %-15s %8.1f ms [%.1f .. %.1f]  %8.0f variants/s  %8.2f ms per distinct set" % (
                    side, 1e3 * med[side], 1e3 * min(times[side]), 1e3 * max(times[side]), len(variants) / med[side],
                    1e3 * med[side] / n_sets))
            lines.append("  ratio loop / score_variants: %.2f x; max |difference| of the two score columns %.3e" % (
                med["loop"] / med["score_variants"], diff))
    return lines


def masks_mode(args, model):
    """The default mode: ``model.masked_marginals`` against the loop; the lines of the report, one block per length."""
    V = model.alphabet_size
    lines = []
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
    return lines


def msa_loop_rows(model, toks):
    """The reference's MSA loop: one B = 1 forward of the whole MSA per column, log_softmax of its logits, one cell kept."""
    rows = []
    for i in range(toks.shape[2]):
        masked = toks.clone()
        masked[0, 0, i] = model.mask_idx
        rows.append(torch.log_softmax(model(masked)["logits"], dim=-1)[:, 0, i])
    return torch.cat(rows, dim=0)


def msa_mode(args):
    """--msa: the lines of the report, one block per shape."""
    from esm_amd.scoring import CHUNK_TOKENS
    from esm_amd.synth import MSA_DIMS, synth_msa_state_dict, synth_msa_tokens

    name = "esm_msa1b_t12_100M_UR50S"
    L, E, H, F = MSA_DIMS[name]
    margs = argparse.Namespace(layers=L, embed_dim=E, ffn_embed_dim=F, attention_heads=H, dropout=0.1, attention_dropout=0.1,
                               activation_dropout=0.1, max_positions=1024, embed_positions_msa=True, embed_positions_msa_dim=E,
                               max_tokens=2 ** 14, max_tokens_per_msa=2 ** 14)
    with skip_param_init():
        model = esm.MSATransformer(margs, esm.Alphabet.from_architecture("msa_transformer")).eval()
    model.load_state_dict(synth_msa_state_dict(L, E, H, F, seed=0))
    model = model.cuda()
    V = model.alphabet_size
    lines = ["%s (L %d, E %d, H %d) on %s; %d rounds after one warm-up, medians [min .. max]" % (
        name, L, E, H, torch.cuda.get_device_name(0), args.rounds)]
    with torch.no_grad():
        for shape in args.msa_shapes:
            R, C = (int(v) for v in shape.lower().split("x"))
            toks = synth_msa_tokens(1, R, C, seed=R).cuda()
            sides = {"loop": lambda: msa_loop_rows(model, toks), "msa_masked_marginals": lambda: model.msa_masked_marginals(toks)}
            ws = {}
            for side, fn in sides.items():  # warm-up; the workspace each side grows to, from an engine without one
                if model._engine is not None:
                    model._engine.workspace = None
                ref = fn()
                ws[side] = model._engine.workspace.numel()
                sides[side] = (fn, ref)
            same = torch.equal(sides["loop"][1], sides["msa_masked_marginals"][1])
            diff = (sides["loop"][1].double() - sides["msa_masked_marginals"][1].double()).abs().max().item()
            times = {side: [] for side in sides}
            for _ in range(args.rounds):
                for side, (fn, _) in sides.items():
                    times[side].append(timed(fn)[0])
            med = {side: statistics.median(t) for side, t in times.items()}
            chunk = max(1, CHUNK_TOKENS // (R * C))
            # logits + log-probabilities written over the whole MSA: C forwards of [R, C, V] logits and their log_softmax
            # against C rows of logits and log-probabilities (and the table they are scattered into)
            out_bytes = {"loop": C * R * C * V * 4 * 2, "msa_masked_marginals": C * V * 4 * 3}
            lines.append("MSA %d x %d (%d tokens), chunk %d copies per forward" % (R, C, R * C, chunk))
            for side in sides:
                lines.append("  %-21s %9.1f ms [%.1f .. %.1f]  %8.1f columns/s   workspace %8.1f MiB   logits + log-prob bytes %10.2f MiB" % (
                    side, 1e3 * med[side], 1e3 * min(times[side]), 1e3 * max(times[side]), C / med[side], ws[side] / 2 ** 20,
                    out_bytes[side] / 2 ** 20))
            spread = {side: max(t) - min(t) for side, t in times.items()}
            extra = med["msa_masked_marginals"] - med["loop"]
            lines.append("  ratio loop / msa_masked_marginals: %.2f x; msa_masked_marginals - loop = %+.1f ms; spread (max - min) of the "
                         "%d rounds: loop %.1f ms, msa_masked_marginals %.1f ms; tables %s (max |difference| %.3e)" % (
                             med["loop"] / med["msa_masked_marginals"], 1e3 * extra, args.rounds, 1e3 * spread["loop"],
                             1e3 * spread["msa_masked_marginals"], "bit-identical" if same else "DIFFER", diff))
            # the gate of a shape where one copy fills the GPU: not slower than the loop by more than the rounds scatter
            bound = max(spread.values())
            lines.append("  verdict: msa_masked_marginals is %s (%+.1f ms against a spread of %.1f ms, the larger of the two sides)" % (
                "NOT SLOWER than the loop beyond the spread of the rounds" if extra <= bound
                else "SLOWER than the loop by more than the spread of the rounds", 1e3 * extra, 1e3 * bound))
    return lines


def library_mode(args, model):
    """--varlen-library N: the lines of the report."""
    g = torch.Generator().manual_seed(args.seed)
    from bench_varlen import uniref_like_lengths  # tools/ is the script's directory: the one length mix of both tools

    lengths = uniref_like_lengths(args.varlen_library, g)
    calls = []
    for lo in range(0, len(lengths), args.library_per_call):
        part = lengths[lo:lo + args.library_per_call]
        t = torch.full((len(part), max(part) + 2), 1, dtype=torch.int64)
        for r, n in enumerate(part):
            t[r, 0] = 0
            t[r, 1:n + 1] = torch.randint(4, 24, (n,), generator=g)
            t[r, n + 1] = 2
        calls.append(t.cuda())
    copies = sum(lengths)  # one masked copy per residue
    packed_tokens = sum(n * (n + 2) for n in lengths)
    padded_tokens = sum(sum(part) * (max(part) + 2) for part in
                        (lengths[lo:lo + args.library_per_call] for lo in range(0, len(lengths), args.library_per_call)))
    sides = {"padded": lambda: [model.pseudo_log_likelihood(t) for t in calls],
             "packed": lambda: [model.pseudo_log_likelihood(t, varlen=True) for t in calls]}
    lines = ["pseudo-log-likelihood of %d sequences (seed %d; %d .. %d residues, median %d), %d per call: %d masked copies; "
             "tokens through the layer stack: packed %d, padded %d (%.1f %% of them padding)" % (
                 len(lengths), args.seed, min(lengths), max(lengths), sorted(lengths)[len(lengths) // 2], args.library_per_call,
                 copies, packed_tokens, padded_tokens, 100.0 * (padded_tokens - packed_tokens) / padded_tokens)]
    with torch.no_grad():
        ref = {side: torch.cat(fn()) for side, fn in sides.items()}  # warm-up of both sides; their scores
        rel = ((ref["packed"] - ref["padded"]).abs() / ref["padded"].abs()).max().item()
        times = {side: [] for side in sides}
        for r in range(args.rounds):
            for side, fn in sides.items():
                times[side].append(timed(fn)[0])
            lines.append("  round %d: padded %9.1f ms   packed %9.1f ms" % (r, 1e3 * times["padded"][-1], 1e3 * times["packed"][-1]))
    med = {side: statistics.median(t) for side, t in times.items()}
    for side in sides:
        lines.append("  %-7s median %9.1f ms [%.1f .. %.1f]  %9.0f masked copies/s  %7.2f sequences/s" % (
            side, 1e3 * med[side], 1e3 * min(times[side]), 1e3 * max(times[side]), copies / med[side], len(lengths) / med[side]))
    spread = {side: max(t) - min(t) for side, t in times.items()}
    gain = med["padded"] - med["packed"]
    bound = max(spread.values())
    lines.append("  ratio padded / packed: %.2f x; padded - packed = %+.1f ms; spread (max - min) of the %d rounds: padded %.1f ms, "
                 "packed %.1f ms; largest relative difference of the two score columns %.3e (the padded sum has no fixed order)" % (
                     med["padded"] / med["packed"], 1e3 * gain, args.rounds, 1e3 * spread["padded"], 1e3 * spread["packed"], rel))
    lines.append("  verdict: packed is %s (%+.1f ms against a spread of %.1f ms, the larger of the two sides)" % (
        "FASTER than padded beyond the spread of the rounds" if gain > bound
        else "SLOWER than padded beyond the spread of the rounds" if -gain > bound
        else "NOT DISTINGUISHABLE from padded: the difference is inside the spread of the rounds", 1e3 * gain, 1e3 * bound))
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
    ap.add_argument("--lengths", type=int, nargs="+", default=None,
                    help="residues; T = length + 2 (default 510 1020; with --variants 510)")
    ap.add_argument("--variants", type=int, default=0, metavar="N",
                    help="score N random double mutants of one protein: model.score_variants against one B = 1 forward per "
                         "distinct position set")
    ap.add_argument("--msa", action="store_true",
                    help="MSA Transformer (100M dims): model.msa_masked_marginals against one B = 1 forward per column")
    ap.add_argument("--msa-shapes", nargs="+", default=["16x257", "400x301"], metavar="RxC", help="MSA depth x columns (with <cls>)")
    ap.add_argument("--varlen-library", type=int, default=0, metavar="N",
                    help="pseudo-log-likelihood of N sequences of the UniRef-like length mix: varlen=True against varlen=False")
    ap.add_argument("--library-per-call", type=int, default=256, help="(with --varlen-library) sequences per call")
    ap.add_argument("--seed", type=int, default=0, help="(with --varlen-library) seed of the length mix and the residues")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.lengths is None:
        args.lengths = [510] if args.variants else [510, 1020]
    if not torch.cuda.is_available():
        raise SystemExit("score_throughput: needs the GPU (a CPU run measures nothing)")
    if args.msa:
        return report(msa_mode(args), args.out)
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
    if args.varlen_library:
        lines += library_mode(args, model)
    else:
        lines += variants_mode(args, model) if args.variants else masks_mode(args, model)
    report(lines, args.out)


def report(lines, out):
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
