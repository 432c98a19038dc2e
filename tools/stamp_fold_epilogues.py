"""Per-tile cycle stamps (esmk_debug_gemm_timing) of gemm9's LayerNorm-fold epilogues at the layer shapes of ESM-2 650M,
next to plain launches of the same shapes as the floor:

    fc1 fold consumer (EPI_GELU_T + ln_rstd)      against  fc1 plain GELU_T and plain STORE_T
    out-proj / fc2 fold producer (EPI_RESID_F32 + ln_part)   against  the plain EPI_RESID_F32 launch

    python tools/stamp_fold_epilogues.py [--B 64] [--rounds 3]

One line per launch: main-loop cycles per K tile and "epilogue done - main loop done" per tile (mean / median / min /
max over all workgroups and tiles), and the HIP-event time of the launch.  Compare two libraries inside one call only
(boxes differ by +-3 %): run it once per library, as tools/ab_two_libraries.sh swaps them.
"""
import argparse
import ctypes
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from esm_amd import _native as nat  # noqa: E402
from esm_amd import ops  # noqa: E402


def linear_ln(a, w, bias, bias2, out, epi, rstd=None, h16=None, part=None, mean=None):
    M, K = a.shape
    Nn = w.shape[0]
    nat.check(nat.lib.esmk_op_linear_ln(nat.ptr(a), nat.ptr(w), nat.ptr(bias), nat.ptr(bias2), nat.ptr(out), M, Nn, K, epi,
                                        nat.dtype_code(a.dtype), nat.ptr(rstd), nat.ptr(h16), h16.shape[1] if h16 is not None else 0,
                                        nat.ptr(part), part.shape[1] if part is not None else 0, nat.ptr(mean), 0, nat.cur_stream()))


def timeit(fn, iters=10):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def stamps(fn, ntiles, nk):
    buf = torch.zeros(256 * 32 * 4, dtype=torch.int64, device="cuda")
    nat.check(nat.lib.esmk_debug_gemm_timing(ctypes.c_void_p(buf.data_ptr())))
    fn()
    torch.cuda.synchronize()
    nat.check(nat.lib.esmk_debug_gemm_timing(ctypes.c_void_p(0)))
    t = buf.view(256, 32, 4)[:, :max(1, ntiles), :3].double().cpu()
    t = t[t[:, 0, 0] > 0]
    loop = (t[:, :, 1] - t[:, :, 0]).mean().item() / nk
    epi = (t[:, :, 2] - t[:, :, 1]).flatten()
    return loop, epi.mean().item(), epi.median().item(), epi.min().item(), epi.max().item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    T, E, F = 1024, 1280, 5120
    M = args.B * T
    dt = torch.float16
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    print("library", nat.lib.esmk_version().decode().split("src:")[-1], torch.cuda.get_device_name(0), flush=True)
    nat.check(nat.lib.esmk_debug_gemm_impl(9, 0))

    def report(name, fn, N, K):
        ms = statistics.median(timeit(fn) for _ in range(args.rounds))
        nt = min(32, (M // 256) * (N // 256) // 256)
        loop, mean, med, lo, hi = stamps(fn, nt, K // 64)
        print(f"{name:34s} {ms * 1e3:8.1f} us  cycles/K-tile {loop:7.1f}  epilogue mean {mean:7.0f} median {med:7.0f} min {lo:7.0f} max {hi:7.0f}",
              flush=True)

    # fc1: N = F, K = E
    a = rnd(M, E).to(dt)
    w = (rnd(F, E) / math.sqrt(E)).to(dt)
    bias, bias2 = rnd(F), rnd(F)
    rstd = 0.5 + torch.rand(M, device="cuda", generator=g)
    out = torch.empty(M, F, dtype=dt, device="cuda")
    report("fc1 fold consumer (GELU)", lambda: linear_ln(a, w, bias, bias2, out, nat.EPI_GELU_T, rstd=rstd), F, E)
    report("fc1 plain GELU_T", lambda: ops.linear(a, w, bias, nat.EPI_GELU_T, out=out), F, E)
    report("fc1 plain STORE_T", lambda: ops.linear(a, w, bias, nat.EPI_STORE_T, out=out), F, E)
    del a, w, out
    # out-proj (K = E) and fc2 (K = F): N = E
    for name, K in (("out-proj", E), ("fc2", F)):
        a = rnd(M, K).to(dt)
        w = (rnd(E, K) / math.sqrt(K)).to(dt)
        bias = rnd(E)
        x = torch.zeros(M, E, device="cuda")
        h16 = torch.zeros(M, E, dtype=dt, device="cuda")
        part = torch.zeros(M, E // 128, 2, device="cuda")
        mean = torch.zeros(M, device="cuda")
        report(f"{name} fold producer", lambda: linear_ln(a, w, bias, None, x, nat.EPI_RESID_F32, h16=h16, part=part, mean=mean), E, K)
        report(f"{name} plain RESID_F32", lambda: ops.linear(a, w, bias, nat.EPI_RESID_F32, out=x), E, K)
        del a, w, x, h16, part, mean


if __name__ == "__main__":
    main()
