"""The kernels of the categorical Jacobian (esm_amd/csrc/jacobian.hip) one launch at a time on random inputs, no model:
substituted copies and the scatter of logit differences exactly, centring, the coupling map and the average product correction
against the fp64 restatements and the bounds of tests/_jacobian_ref.py."""
import pytest
import torch

import _jacobian_ref as R
from esm_amd import _native as N
from esm_amd import ops

pytestmark = pytest.mark.gpu
SHAPES = [(L, nA) for L in (1, 23, 70) for nA in (1, 3, 20, 32)]
V = 33


def rand_j(L, nA, seed, kind="plain"):
    g = torch.Generator().manual_seed(seed)
    J = torch.randn((L, nA, L, nA), generator=g, dtype=torch.float32) * 3.0
    if kind == "offset":  # one large constant: any single pass removes it, and its size must not enter the error
        J += 1000.0
    if kind == "axes":  # per axis a large term that is constant along THAT axis only: no other pass removes it
        for axis, scale in zip(range(4), (300.0, 200.0, 100.0, 50.0)):
            shape = list(J.shape)
            shape[axis] = 1
            J += scale * torch.randn(shape, generator=g)
    return J.cuda()


# ---- esmk_op_substitute_rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 65])
@pytest.mark.parametrize("with_src", [False, True])
def test_substitute_rows_is_exact(n, with_src):
    B, T = 3, 37
    g = torch.Generator().manual_seed(n)
    tokens = torch.randint(0, V, (B, T), generator=g, dtype=torch.int64)
    src = torch.randint(-2, B + 2, (n,), generator=g, dtype=torch.int32)  # -2, -1, B, B + 1: clamped
    pos = torch.randint(0, T, (n,), generator=g, dtype=torch.int32)
    tok = torch.randint(0, V, (n,), generator=g, dtype=torch.int32)
    for k, (p, t) in enumerate([(-1, 5), (T, 5), (T + 5, 5), (3, -1), (3, V), (3, 40)]):  # substitute nothing
        if k < n:
            pos[-1 - k], tok[-1 - k] = p, t
    want = torch.empty((n, T), dtype=torch.int64)
    for i in range(n):
        want[i] = tokens[min(max(int(src[i]), 0), B - 1) if with_src else 0]
        if 0 <= int(pos[i]) < T and 0 <= int(tok[i]) < V:
            want[i, int(pos[i])] = int(tok[i])
    got = ops.substitute_rows(tokens.cuda(), pos.cuda(), tok.cuda(), src.cuda() if with_src else None, vocab=V)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    if not with_src:  # a single sequence [T] is row 0
        assert torch.equal(ops.substitute_rows(tokens[0].cuda(), pos.cuda(), tok.cuda(), vocab=V).cpu(), want)


@pytest.mark.parametrize("n,T", [(9, 300), (8200, 5)])
def test_substitute_rows_loop_trips_grid_wrap_and_clamps(n, T):
    """T = 300: a copy is longer than one trip of its workgroup's 256 lanes and no multiple of it; n = 8200: the copies wrap the
    grid of 8192 workgroups.  A position of -1 or T and a token of -1 or V substitute nothing, a source row of -2 or B + 3 is
    clamped, and the row behind the last copy is not written."""
    B, SENT = 3, -7
    g = torch.Generator().manual_seed(n)
    tokens = torch.randint(0, V, (B, T), generator=g, dtype=torch.int64)
    pos = torch.randint(0, T, (n,), generator=g, dtype=torch.int32)
    tok = torch.randint(0, V, (n,), generator=g, dtype=torch.int32)
    src = torch.randint(0, B, (n,), generator=g, dtype=torch.int32)
    pos[:8] = torch.tensor([-1, T, 3, 3, 0, T - 1, T - 1, min(256, T - 1)], dtype=torch.int32)
    tok[:8] = torch.tensor([5, 5, -1, V, 0, V - 1, 7, 9], dtype=torch.int32)
    src[:8] = torch.tensor([1, 2, 0, 1, -2, B + 3, 0, 1], dtype=torch.int32)
    pos[n - 1], tok[n - 1], src[n - 1] = T - 1, V - 1, B - 1  # the last copy of the last trip
    for with_src in (True, False):
        want = tokens[src.long().clamp(0, B - 1)].clone() if with_src else tokens[:1].expand(n, T).clone()
        hit = (pos >= 0) & (pos < T) & (tok >= 0) & (tok < V)
        want[torch.arange(n)[hit], pos[hit].long()] = tok[hit].long()
        out = torch.full((n + 1, T), SENT, dtype=torch.int64, device="cuda")
        tok_d, pos_d, new_d, src_d = tokens.cuda(), pos.cuda(), tok.cuda(), src.cuda() if with_src else None
        N.check(N.lib.esmk_op_substitute_rows(N.ptr(tok_d), N.ptr(src_d), N.ptr(pos_d), N.ptr(new_d), N.ptr(out), B, T, n, V,
                                              N.cur_stream()))
        assert torch.equal(out[:n].cpu(), want), with_src
        assert (out[n] == SENT).all(), "a store behind the last copy"
        assert torch.equal(ops.substitute_rows(tok_d, pos_d, new_d, src_d, vocab=V).cpu(), want)


# ---- esmk_op_jacobian_scatter -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,nA", SHAPES)
def test_jacobian_scatter_is_bit_equal(L, nA):
    g = torch.Generator().manual_seed(100 * L + nA)
    copies = L * nA
    copy0 = min(2, copies - 1)  # non-zero wherever there is more than one copy
    n = min(7, copies - copy0)
    logits = (torch.randn((n * L, V), generator=g) * 5.0).cuda()
    wt = (torch.randn((L, V), generator=g) * 5.0).cuda()
    cols = torch.randperm(V, generator=g)[:nA].to(torch.int32).cuda()
    J = torch.full((L, nA, L, nA), -7.5, dtype=torch.float32).cuda()
    assert ops.jacobian_scatter(logits, wt, cols, J, copy0=copy0) is J
    want = torch.full((copies, L, nA), -7.5, dtype=torch.float32).cuda()
    want[copy0:copy0 + n] = logits.view(n, L, V)[:, :, cols.long()] - wt[:, cols.long()]
    assert torch.equal(J.view(copies, L, nA), want)  # the chunk's slice, and nothing outside it


def test_jacobian_scatter_clamps_columns():
    L, nA = 5, 4
    g = torch.Generator().manual_seed(3)
    logits, wt = torch.randn((L * nA * L, V), generator=g).cuda(), torch.randn((L, V), generator=g).cuda()
    cols = torch.tensor([-3, 7, V, 2 ** 31 - 1], dtype=torch.int32).cuda()
    J = ops.jacobian_scatter(logits, wt, cols, torch.zeros((L, nA, L, nA)).cuda())
    c = torch.tensor([0, 7, V - 1, V - 1]).cuda()
    assert torch.equal(J.view(L * nA, L, nA), logits.view(L * nA, L, V)[:, :, c] - wt[:, c])


# ---- esmk_op_jacobian_center ------------------------------------------------------------------------------------------------
def check_center(J, what):
    ref, ms = R.center_ref(J)
    bound = R.center_bound(ms)
    got = ops.jacobian_center(J.clone())
    assert got.dtype == torch.float32 and got.shape == J.shape and torch.isfinite(got).all()
    R.report(f"jacobian_center {what}", (got.double() - ref).abs().max().cpu(), bound)
    means = torch.stack([got.double().mean(dim=axis).abs().max() for axis in range(4)]).cpu()
    R.report(f"jacobian_center {what}: means along the four axes", means, bound)
    assert torch.equal(ops.jacobian_center(J.clone()), got)  # the same bits from a second call


@pytest.mark.parametrize("L,nA", SHAPES)
def test_jacobian_center_against_fp64(L, nA):
    check_center(rand_j(L, nA, seed=7 * L + nA), f"L={L} nA={nA}")


@pytest.mark.parametrize("kind", ["offset", "axes"])
@pytest.mark.parametrize("L,nA", [(23, 20), (70, 3)])
def test_jacobian_center_removes_large_offsets(L, nA, kind):
    """Kind "offset": +1000 everywhere, which must not enter the error.  Kind "axes": a pass that is skipped or run along the
    wrong axis leaves values and means of hundreds behind."""
    check_center(rand_j(L, nA, seed=L + nA, kind=kind), f"L={L} nA={nA} {kind}")


def test_jacobian_center_of_an_unaligned_view():
    """A tensor that does not start on a 16-byte boundary takes the 4-byte path: the same values."""
    L, nA = 23, 20
    J = rand_j(L, nA, seed=5)
    buf = torch.empty((J.numel() + 1,), dtype=torch.float32).cuda()
    view = buf[1:].view(L, nA, L, nA)
    view.copy_(J)
    assert view.data_ptr() % 16 == 4
    assert torch.equal(ops.jacobian_center(view), ops.jacobian_center(J.clone()))


# ---- esmk_op_jacobian_contacts, esmk_op_apc -----------------------------------------------------------------------------------
@pytest.mark.parametrize("L,nA", SHAPES)
def test_jacobian_contacts_and_apc_against_fp64(L, nA):
    Jc = rand_j(L, nA, seed=11 * L + nA)
    S = ops.jacobian_contacts(Jc)
    assert S.dtype == torch.float32 and tuple(S.shape) == (L, L) and torch.isfinite(S).all()
    S_ref = R.contacts_ref(Jc)
    R.report(f"jacobian_contacts L={L} nA={nA}", (S.double() - S_ref).abs().cpu(), R.contacts_bound(S_ref).cpu())
    assert torch.equal(S, S.t())  # symmetric bit for bit
    assert torch.equal(ops.jacobian_contacts(Jc), S)
    C = ops.apc(S.clone())
    C_ref = R.apc_ref(S)
    R.report(f"apc L={L} nA={nA}", (C.double() - C_ref).abs().cpu(), R.apc_bound(S, C_ref).cpu())
    assert torch.isfinite(C).all() and bool((C.diagonal() == 0).all())
    assert torch.equal(ops.apc(S.clone()), C)


def test_apc_of_an_asymmetric_matrix():
    """Row and column sums are different things: a matrix that is not symmetric tells them apart."""
    L = 70
    S = torch.rand((L, L), generator=torch.Generator().manual_seed(2)).cuda() * torch.arange(1, L + 1).cuda()
    C = ops.apc(S.clone())
    C_ref = R.apc_ref(S)
    R.report("apc asymmetric", (C.double() - C_ref).abs().cpu(), R.apc_bound(S, C_ref).cpu())


@pytest.mark.parametrize("L,nA", [(1, 20), (23, 20)])
def test_all_zero_input_gives_zeros(L, nA):
    Jc = torch.zeros((L, nA, L, nA), dtype=torch.float32).cuda()
    assert bool((ops.jacobian_center(Jc.clone()) == 0).all())
    S = ops.jacobian_contacts(Jc)
    assert bool((S == 0).all())
    C = ops.apc(S)  # s == 0: nothing to correct, and no 0 / 0
    assert bool((C == 0).all())
