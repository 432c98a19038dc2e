"""The whole forward at the smallest batches whose activations pass 2^32 bytes (tests/_index_width.py ENGINE_CASES), held
to the property test_kernels_gpu.py::test_small_batch_forward_equals_large_batch_rows asserts at small sizes: a sequence's
bits do not depend on its batch.  The sequences around the boundary, at both ends and in the middle of a batch of 206 (or
104) must come out bit-equal when they run as a batch of a handful, where no offset is anywhere near 2^31.

    esm2_t36_3B dims (2 layers, E 2560, head_dim 64), B = 206, T = 1024: the FFN activation [B*T, 10240] fp16 is 4.0 GiB,
        byte 2^32 and element 2^31 fall in sequence 204; the fp32 stream [B*T, 2560] passes 2^31 bytes in the same
        sequence.  With the LayerNorm fold (the default at these dims) and without.
    esm2_t48_15B dims (1 layer, E 5120, head_dim 128), B = 104: the FFN activation [B*T, 20480] passes 2^32 bytes in
        sequence 102, the stream 2^31 bytes in the same sequence.
    token-packed, 3B dims: 220 sequences of 900 .. 1024 tokens, more than 209,716 packed rows.
Every case prints esmk_workspace_bytes and is gated on it: workspace + outputs + 6 GiB for the model and the small batch
is the declared peak (at most 24 GiB), and that plus 2 GiB must be free.

MEASURED on an MI355X: workspace, wall time, torch.cuda.max_memory_allocated()
    3B dims, B 206, fold     8.08 GiB   1.09 s   14.63 GiB        3B dims, B 206, plain   7.04 GiB   0.94 s   13.59 GiB
    15B dims, B 104          7.11 GiB   1.99 s   14.71 GiB        3B dims, packed         8.18 GiB   1.10 s   15.08 GiB"""
import gc
import time

import pytest
import torch

import _index_width as W
from esm_amd import _native as N
from esm_amd.packing import pack_plan
from test_ln_fold_gpu import build, run_mode

pytestmark = pytest.mark.gpu
PAD, EOS = 1, 2
# next to the workspace and the outputs: fp32 parameters and packed image (15B dims, one layer: 1.9 GiB), tokens, the
# batch of a handful with its own workspace, the boolean temporaries of the finite checks (measured: 4.5 GiB at most)
MODEL_BYTES = 6 * 2 ** 30


@pytest.fixture(autouse=True)
def _measure(request):
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print(f"\n[index width] {request.node.name}: {time.perf_counter() - t0:.2f} s, max_memory_allocated "
          f"{torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    gc.collect()
    torch.cuda.empty_cache()


def tokens(B, T, seed, short):
    """random residues; `short`: {sequence: length} get <eos> at length - 1 and trailing pads"""
    g = torch.Generator().manual_seed(seed)
    toks = torch.randint(4, 24, (B, T), generator=g, dtype=torch.int64)
    toks[:, 0] = 0
    toks[:, -1] = EOS
    for b, n in short.items():
        toks[b, n - 1] = EOS
        toks[b, n:] = PAD
    return toks


def gate(name, model, B, T, out_bytes, packed_rows=0):
    """B, T: the padded batch; packed_rows > 0: B segments in that many packed rows (esmk_packed_workspace_bytes)"""
    eng = model._engine
    if packed_rows:
        ws = eng._query(N.lib.esmk_packed_workspace_bytes, B, packed_rows, N.OUT_LOGITS)
        what = f"esmk_packed_workspace_bytes({B}, {packed_rows})"
    else:
        ws, what = eng.workspace_bytes(B, T, N.OUT_LOGITS), f"esmk_workspace_bytes({B}, {T})"
    peak = ws + out_bytes + MODEL_BYTES
    print(f"\n{name}: {what} = {ws} ({ws / 2 ** 30:.2f} GiB), declared peak {peak / 2 ** 30:.2f} GiB")
    assert peak <= W.GATE_BYTES, (name, peak)
    reason = W.memory_gate(name, peak, torch.cuda.mem_get_info()[0])
    if reason:
        pytest.skip(reason)


def padded_case(case, picks, short, fold):
    L, E, H, B, T = (case.shape[x] for x in ("L", "E", "H", "B", "T"))
    model, _ = build(L, E, H, seed=7)
    toks = tokens(B, T, seed=8, short=short)

    def f():
        few = model(toks[picks].cuda(), repr_layers=[L])   # first: the engine exists for the gate, nothing large is live yet
        gate(case.name, model, B, T, B * T * (E + 33) * 4)
        big = model(toks.cuda(), repr_layers=[L])
        return few, big

    few, big = run_mode(model, fold, f)
    assert model.ln_fold_active() is (fold and H * 64 == E)
    for name, b, f_ in (("logits", big["logits"], few["logits"]), ("representations", big["representations"][L], few["representations"][L])):
        assert b.numel() < 2 ** 30 and bool(torch.isfinite(b).all()), name
        for i, s in enumerate(picks):
            assert torch.equal(b[s], f_[i]), f"{case.name}: {name} of sequence {s} differ between the batch of {B} and the batch of {len(picks)}"
    del model, few, big


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "plain"])
def test_3b_dims_batch_206(fold):
    case = W.ENGINE_CASES["engine_3b"]
    assert W.boundary_sequences(case) == 204
    padded_case(case, [0, 1, 102, 103, 204, 205], {1: 700, 103: 1000, 205: 333}, fold)


def test_15b_dims_batch_104():
    case = W.ENGINE_CASES["engine_15b"]
    assert W.boundary_sequences(case) == 102
    padded_case(case, [0, 51, 52, 102, 103], {51: 900, 103: 410}, False)


def test_3b_dims_token_packed():
    """forward_varlen(min_saving=None): the packed row space passes row 209,716, where the FFN activation passes 2^32 bytes
    and the stream 2^31; the first sequence, the two around that row and the last are bit-equal to the padded engine on
    each alone"""
    L, E, H = 2, 2560, 40
    lengths = [900 + (i * 37) % 125 for i in range(220)]
    T = max(lengths)
    toks = tokens(len(lengths), T, seed=9, short={b: n for b, n in enumerate(lengths) if n < T})
    plan = pack_plan(toks, PAD)
    edge = W.boundary_unit(W.B32, 4 * E * 2)
    assert edge == 209_715 and plan.rows > edge + 1024 and plan.rows <= W.MAX_ROWS
    starts = plan.segments[:, 0].tolist()
    at = max(b for b, s in enumerate(starts) if s <= edge)
    assert 0 < at < len(lengths) - 2
    picks = [0, at, at + 1, len(lengths) - 1]
    model, _ = build(L, E, H, seed=7)
    with torch.no_grad():
        alone = [model(toks[b:b + 1, :lengths[b]].cuda(), repr_layers=[L]) for b in picks]
        gate("engine_3b_packed", model, len(lengths), T, 2 * len(lengths) * T * (E + 33) * 4, packed_rows=plan.rows)
        pk = model.forward_varlen(toks, repr_layers=[L], min_saving=None)
    for name, p in (("logits", pk["logits"]), ("representations", pk["representations"][L])):
        assert p.numel() < 2 ** 30 and bool(torch.isfinite(p).all()), name
    for b, one in zip(picks, alone):
        n = lengths[b]
        assert torch.equal(pk["representations"][L][b, :n], one["representations"][L][0]), b
        assert torch.equal(pk["logits"][b, :n], one["logits"][0]), b
    del model, pk, alone
