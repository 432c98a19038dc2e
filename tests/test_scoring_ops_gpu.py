"""The two single-kernel entries of variant scoring (csrc/scoring.hip), one op at a time: the row log-softmax against
torch.log_softmax of the same fp32 values taken in fp64, and the masked batch builder against the clone-and-assign loop
of the reference (examples/variant-prediction/predict.py:208-209)."""
import pytest
import torch

from _scoring_ref import check_rows
from esm_amd import _native as N
from esm_amd import ops

pytestmark = pytest.mark.gpu


def logits_of(kind, n, V, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "ordinary":
        return 4.0 * torch.randn((n, V), generator=g)
    if kind == "spike":  # one entry at +80, the rest near -80: without the max subtraction exp() overflows or the sum is 0
        x = -80.0 + 0.5 * torch.randn((n, V), generator=g)
        x[torch.arange(n), torch.randint(0, V, (n,), generator=g)] = 80.0
        return x
    if kind == "equal":
        return torch.randn((n, 1), generator=g).expand(n, V).contiguous()
    x = torch.cat([logits_of(k, n, V, seed + j) for j, k in enumerate(("ordinary", "spike", "equal"))])
    return x[torch.randperm(3 * n, generator=g)[:n]].contiguous()


@pytest.mark.parametrize("V", [33, 35])
@pytest.mark.parametrize("n", [1, 63, 65])
def test_log_softmax_rows_against_fp64(n, V):
    for kind in ("ordinary", "spike", "equal", "mixed"):
        x = logits_of(kind, n, V, seed=7 * n + V).cuda()
        g = torch.Generator().manual_seed(n)
        target = torch.randint(0, V, (n,), generator=g, dtype=torch.int32).cuda()
        out, tgt = ops.log_softmax_rows(x, target)
        check_rows(out, x, f"log_softmax n={n} V={V} {kind}")
        # the target output is the gathered entry of the full output, bit for bit
        assert torch.equal(tgt, out.gather(1, target.long().unsqueeze(1)).squeeze(1))
        assert torch.equal(ops.log_softmax_rows(x), out)  # without the second output: the same rows
        if kind == "spike":
            assert (out.amax(-1) > -1e-6).all() and (out.amin(-1) < -150).all()


@pytest.mark.parametrize("n", [70, 1])
def test_mask_rows_equals_clone_and_assign(n):
    T, MASK = 70, 32
    g = torch.Generator().manual_seed(3)
    tokens = torch.randint(4, 24, (1, T), generator=g, dtype=torch.int64)
    cases = [torch.randperm(T, generator=g)] if n == T else [torch.tensor([0]), torch.tensor([T - 1])]
    for pos in cases:
        assert n != T or (0 in pos.tolist() and T - 1 in pos.tolist())
        want = []
        for i in pos.tolist():
            masked = tokens.clone()
            masked[0, i] = MASK
            want.append(masked)
        want = torch.cat(want)
        got = ops.mask_rows(tokens.cuda(), pos.to(torch.int32).cuda(), mask_idx=MASK)
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
        assert torch.equal(ops.mask_rows(tokens[0].cuda(), pos.to(torch.int32).cuda(), mask_idx=MASK).cpu(), want)  # [T] row


def test_mask_rows_with_source_index():
    """[B, T] plus a per-row source index: row i is sequence src[i] with its position masked."""
    B, T, MASK = 3, 70, 33
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(4, 24, (B, T), generator=g, dtype=torch.int64)
    src = torch.randint(0, B, (T,), generator=g)
    pos = torch.randperm(T, generator=g)
    want = tokens[src].clone()
    want[torch.arange(T), pos] = MASK
    got = ops.mask_rows(tokens.cuda(), pos.to(torch.int32).cuda(), src.to(torch.int32).cuda(), mask_idx=MASK)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("n,T", [(7, 300), (8200, 5)])
def test_mask_rows_loop_trips_grid_wrap_and_clamps(n, T):
    """T = 300: a copy is longer than one trip of its workgroup's 256 lanes and no multiple of it; n = 8200: the copies wrap the
    grid of 8192 workgroups.  A position of -1 or T masks nothing, a source row of -2 or B + 3 is clamped, and the row behind
    the last copy is not written."""
    B, MASK, SENT = 3, 32, -7
    g = torch.Generator().manual_seed(n)
    tokens = torch.randint(4, 24, (B, T), generator=g, dtype=torch.int64)
    pos = torch.randint(0, T, (n,), generator=g, dtype=torch.int32)
    src = torch.randint(0, B, (n,), generator=g, dtype=torch.int32)
    pos[:6] = torch.tensor([-1, T, 0, T - 1, T - 1, min(256, T - 1)], dtype=torch.int32)
    src[:6] = torch.tensor([1, 2, -2, B + 3, 0, 1], dtype=torch.int32)
    pos[n - 1], src[n - 1] = T - 1, B - 1  # the last copy of the last trip
    for with_src in (True, False):
        want = tokens[src.long().clamp(0, B - 1)].clone() if with_src else tokens[:1].expand(n, T).clone()
        hit = (pos >= 0) & (pos < T)
        want[torch.arange(n)[hit], pos[hit].long()] = MASK
        out = torch.full((n + 1, T), SENT, dtype=torch.int64, device="cuda")
        tok_d, pos_d, src_d = tokens.cuda(), pos.cuda(), src.cuda() if with_src else None
        N.check(N.lib.esmk_op_mask_rows(N.ptr(tok_d), N.ptr(src_d), N.ptr(pos_d), N.ptr(out), B, T, n, MASK, N.cur_stream()))
        assert torch.equal(out[:n].cpu(), want), with_src
        assert (out[n] == SENT).all(), "a store behind the last copy"
        assert torch.equal(ops.mask_rows(tok_d, pos_d, src_d, mask_idx=MASK).cpu(), want)
