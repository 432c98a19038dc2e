#!/usr/bin/env python
"""Protein search on pooled embeddings (esm_amd/search.py): (i) ``EmbeddingIndex.search`` on a random index — images, the dense
GEMM per database block and the streaming top-k merge — against the loop a user writes today (unit vectors in fp32, ``torch``
matmul in chunks, ``torch.topk`` per chunk and a merge of the running lists); (ii) the early exit ``model.embed_layer(layer=k)``
against ``model.forward(repr_layers=[k])`` of the same build.

  python tools/search_throughput.py [--vectors 1048576] [--embed-dim 1280] [--queries 256 1] [--top-k 100] [--rounds 5]
      [--model esm2_t33_650M_UR50D] [--batch 64] [--seq-len 1022] [--skip-search] [--skip-exit] [--out profiles/search_throughput.log]

The index holds random fp32 rows (the forward is not part of (i)).  One warm-up of every side, then --rounds timed rounds
alternating the sides in one process, each ending in a device synchronise; medians [min .. max].  The GEMM and the merge of the
search's first block are timed with device events; the merge alone is compared with ``torch.topk`` on the same fp32 block and
with one read of the block at the device's copy rate (4.05 TB/s, profiles/stream_edit_throughput.log).  Both sides' ids are
compared (torch's fp32 product is rounded differently from the f16x3 GEMM: the share of equal ids is reported, not asserted)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from esm_amd import _native as N  # noqa: E402
from esm_amd import ops  # noqa: E402
from esm_amd import search as S  # noqa: E402

COPY_RATE = 4.05e12  # bytes / s of a device copy's read side, profiles/stream_edit_throughput.log


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def fmt(ts):
    return "%9.2f ms [%8.2f .. %8.2f]" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts))


def alternate(sides, rounds):
    times = {name: [] for name in sides}
    for fn in sides.values():
        fn()
    for _ in range(rounds):
        for name, fn in sides.items():
            times[name].append(timed(fn)[0])
    return times


def torch_search(q, unit_db, k, chunk):
    """the loop a user writes: fp32 matmul per chunk of the (unit) database, topk, merge with the running lists"""
    qn = torch.nn.functional.normalize(q, dim=1)
    val = idx = None
    for lo in range(0, unit_db.shape[0], chunk):
        s = qn @ unit_db[lo:lo + chunk].t()
        v, i = s.topk(min(k, s.shape[1]), dim=1)
        i = i + lo
        if val is not None:
            v, pick = torch.cat([val, v], 1).topk(k, dim=1)
            i = torch.cat([idx, i], 1).gather(1, pick)
        val, idx = v, i
    return val, idx


def device_events(fn, rounds):
    ts = []
    for r in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if r:
            ts.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(ts)


def search_part(args, lines):
    n, E, k = args.vectors, args.embed_dim, args.top_k
    g = torch.Generator(device="cuda").manual_seed(args.seed)
    vectors = np.empty((n, E), dtype=np.float32)
    unit = torch.empty((n, E), dtype=torch.float32, device="cuda")
    for lo in range(0, n, 1 << 16):
        x = torch.randn((min(1 << 16, n - lo), E), generator=g, device="cuda")
        vectors[lo:lo + x.shape[0]] = x.cpu().numpy()
        unit[lo:lo + x.shape[0]] = torch.nn.functional.normalize(x, dim=1)
    index = S.EmbeddingIndex(vectors, [""] * n, np.ones(n, dtype=np.int64))
    t_image, _ = timed(lambda: index.to("cuda"))
    lines.append("(i) search: %d random fp32 vectors, E = %d, k = %d, max_bytes = %d; the device image takes %.2f GB (%.1f KB per vector), "
                 "built in %.2f s (upload included)" % (n, E, k, args.max_bytes, index.image_bytes() / 1e9, index.image_bytes() / n / 1e3, t_image))
    for Q in args.queries:
        q = torch.randn((Q, E), generator=g, device="cuda")
        qc, nb = S.plan_search(n, Q, args.max_bytes)
        sides = {"index.search": lambda: index.search(q, k, max_bytes=args.max_bytes),
                 "torch matmul + topk + merge": lambda: torch_search(q, unit, k, nb)}
        times = alternate(sides, args.rounds)
        ours, theirs = sides["index.search"](), sides["torch matmul + topk + merge"]()
        equal = float((ours["ids"].long() == theirs[1]).float().mean())
        lines.append("")
        lines.append("    Q = %d: blocks of %d vectors (%d block%s, fp32 scratch %.2f GB)" % (Q, nb, -(-n // nb), "" if n <= nb else "s", 4 * qc * nb / 1e9))
        for name in sides:
            lines.append("      %-28s %s   %8.2f G similarities/s" % (name, fmt(times[name]), Q * n / statistics.median(times[name]) / 1e9))
        lines.append("      index.search over the torch loop: %.2f x; ids equal to torch's at %.2f %% of the %d x %d slots" % (
            statistics.median(times["torch matmul + topk + merge"]) / statistics.median(times["index.search"]), 100 * equal, Q, k))
        # the first block's launches by device events
        width = min(nb, S._up(n, S.BLOCK_ALIGN))
        cols = min(nb, n)
        img_q = ops.align_rows(q, None, cosine=True, b_side=False)
        blk = torch.empty((Q, width), dtype=torch.float32, device="cuda")
        val = torch.empty((Q, k), dtype=torch.float32, device="cuda")
        ids = torch.empty((Q, k), dtype=torch.int32, device="cuda")
        t_gemm = device_events(lambda: ops.linear(img_q, index.image[:width], None, N.EPI_STORE_F32, out=blk), args.rounds)
        t_merge = device_events(lambda: ops.topk_merge(blk, k, val, ids, n_cols=cols, first=True), args.rounds)
        t_topk = device_events(lambda: blk[:, :cols].topk(k, dim=1), args.rounds)
        read = 4.0 * Q * cols
        lines.append("      first block [%d, %d], device events: GEMM %.3f ms (%.1f TFLOP/s of 2 Q N 3 Ep), merge %.3f ms (%.2f TB/s read; one read at "
                     "the copy rate: %.3f ms, %.2f x that), torch.topk on the same block %.3f ms (merge / torch.topk = %.2f)" % (
                         Q, cols, 1e3 * t_gemm, 2.0 * Q * width * index.image.shape[1] / t_gemm / 1e12, 1e3 * t_merge, read / t_merge / 1e12,
                         1e3 * read / COPY_RATE, t_merge / (read / COPY_RATE), 1e3 * t_topk, t_merge / t_topk))
    del index, unit
    torch.cuda.empty_cache()


def exit_part(args, lines):
    import esm
    from esm_amd.synth import ESM2_DIMS, skip_param_init, synth_esm2_state_dict, synth_tokens

    L, E, H = ESM2_DIMS[args.model]
    with skip_param_init():
        model = esm.ESM2(L, E, H).eval()
    model.load_state_dict(synth_esm2_state_dict(L, E, H, seed=0))
    model = model.cuda()
    toks = synth_tokens(args.batch, args.seq_len, seed=1).cuda()
    lines.append("")
    lines.append("(ii) early exit: %s dims (L = %d, E = %d), synthetic weights, %d x %d tokens, fold %s" % (
        args.model, L, E, toks.shape[0], toks.shape[1], "on" if (model(toks[:1]) is not None and model.ln_fold_active()) else "off"))
    with torch.no_grad():
        for k in (L // 2, 3 * L // 4):
            sides = {"forward(repr_layers=[%d])" % k: lambda: model(toks, repr_layers=[k])["representations"][k],
                     "embed_layer(layer=%d)" % k: lambda: model.embed_layer(toks, k)}
            times = alternate(sides, args.rounds)
            names = list(sides)
            same = torch.equal(sides[names[0]](), sides[names[1]]())
            ratio = statistics.median(times[names[1]]) / statistics.median(times[names[0]])
            lines.append("")
            for name in names:
                lines.append("      %-28s %s" % (name, fmt(times[name])))
            lines.append("      embed_layer / forward = %.3f (k / L = %.3f; the embedding stage, the output copy and, on the forward's side, the "
                         "head make the difference); same bits: %s" % (ratio, k / L, same))


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--vectors", type=int, default=1 << 20)
    p.add_argument("--embed-dim", type=int, default=1280)
    p.add_argument("--queries", type=int, nargs="+", default=[256, 1])
    p.add_argument("--top-k", type=int, default=100)
    p.add_argument("--max-bytes", type=int, default=2 << 30)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--model", default="esm2_t33_650M_UR50D")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--seq-len", type=int, default=1022)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--skip-search", action="store_true")
    p.add_argument("--skip-exit", action="store_true")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("search_throughput: needs the GPU (a timing taken anywhere else says nothing)")
    lines = ["protein search on %s; %d rounds after one warm-up, alternating in one process, medians [min .. max]" % (
        torch.cuda.get_device_name(0), args.rounds), ""]
    if not args.skip_search:
        search_part(args, lines)
    if not args.skip_exit:
        exit_part(args, lines)
    lines.append("")
    lines.append("    not measured: EmbeddingIndex.build on real sequences, search_and_align, the command line, other k, E and index sizes")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
