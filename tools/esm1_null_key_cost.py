"""What the null key / value pair of the ESM-1 models costs (one measurement, no threshold; DESIGN.md quotes it).

    python tools/esm1_null_key_cost.py [--out profiles/esm1_null_key_cost.log]

1. steady-state ms per forward at the ESM-1 t34 dimensions (L = 34, E = 1280, H = 20, plain path, null-key attention)
   against the ESM-1b dimensions (L = 33, the engine's default mode), B = 64 x T = 1022, fp16 operands, logits only;
2. esmk_op_attention_biaskv against esmk_op_attention (mode 0) on the same q / k / v, B = 64, H = 20, T = 1022.
Synthetic weights; HIP events around `steps` back-to-back calls after `warmup` calls; each figure is the median of
`rounds` such rounds, the two candidates of a comparison alternating round by round."""
import argparse
import statistics
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--length", type=int, default=1022)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import esm
    from esm_amd import ops
    from esm_amd.synth import esm1_args, skip_param_init, synth_esm1_state_dict, synth_esm1b_state_dict, synth_tokens

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    E, H, B, T = 1280, 20, args.batch, args.length
    say(f"device {torch.cuda.get_device_name(0)}; torch {torch.__version__}; B = {B}, T = {T}, fp16 operands; "
        f"{args.rounds} rounds of {args.steps} calls after {args.warmup} warm-up calls, medians")
    with skip_param_init():
        m1 = esm.ProteinBertModel(esm1_args(34, E, H), esm.Alphabet.from_architecture("protein_bert_base")).eval()
        m1.load_state_dict(synth_esm1_state_dict(34, E, H, seed=1), strict=True)
        a1b = argparse.Namespace(arch="roberta_large", layers=33, embed_dim=E, ffn_embed_dim=4 * E, attention_heads=H,
                                 max_positions=1024, token_dropout=True, emb_layer_norm_before=True)
        m1b = esm.ProteinBertModel(a1b, esm.Alphabet.from_architecture("roberta_large")).eval()
        m1b.load_state_dict(synth_esm1b_state_dict(33, E, H, seed=1), strict=True)
    m1, m1b = m1.cuda(), m1b.cuda()
    toks1b = synth_tokens(B, T - 2, seed=2).cuda()
    toks1 = toks1b.clone()
    toks1[:, 0] = 32
    toks1[:, -1] = 5
    res = {"esm1": [], "esm1b": []}
    with torch.no_grad():
        for _ in range(args.rounds):
            res["esm1"].append(timed(lambda: m1(toks1), args.warmup, args.steps))
            res["esm1b"].append(timed(lambda: m1b(toks1b), args.warmup, args.steps))
    t1, t1b = statistics.median(res["esm1"]), statistics.median(res["esm1b"])
    say(f"forward ESM-1 t34 dims (L = 34, plain path, null-key attention): {t1:.2f} ms  = {t1 / 34:.3f} ms / layer   rounds {[round(x, 2) for x in res['esm1']]}")
    say(f"forward ESM-1b dims   (L = 33, LayerNorm fold {'on' if m1b.ln_fold_active() else 'off'}):             {t1b:.2f} ms  = {t1b / 33:.3f} ms / layer   rounds {[round(x, 2) for x in res['esm1b']]}")
    say(f"per layer ESM-1 / ESM-1b: {(t1 / 34) / (t1b / 33):.4f}")
    del m1, m1b
    torch.cuda.empty_cache()
    g = torch.Generator(device="cuda").manual_seed(0)
    qk, _ = ops.to_log2_domain(torch.randn(B, H, T, 64, device="cuda", generator=g) * 0.6, torch.float16)
    k = (torch.randn(B, H, T, 64, device="cuda", generator=g) * 0.6).half()
    vt = ops.make_vt(torch.randn(B, H, T, 64, device="cuda", generator=g).half())
    bk = (torch.randn(H, 64, device="cuda", generator=g) * 0.6).half()
    bv = torch.randn(H, 64, device="cuda", generator=g).half()
    r = {"plain": [], "null": []}
    for _ in range(args.rounds):
        r["plain"].append(timed(lambda: ops.attention(qk, k, vt), 3, 20))
        r["null"].append(timed(lambda: ops.attention_biaskv(qk, k, vt, bk, bv), 3, 20))
    tp, tn = statistics.median(r["plain"]), statistics.median(r["null"])
    say(f"esmk_op_attention (mode 0):  {tp * 1e3:.1f} us   rounds {[round(x * 1e3, 1) for x in r['plain']]}")
    say(f"esmk_op_attention_biaskv:    {tn * 1e3:.1f} us   rounds {[round(x * 1e3, 1) for x in r['null']]}   (also allocates and writes lse)")
    say(f"null key / plain: {tn / tp:.4f}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
