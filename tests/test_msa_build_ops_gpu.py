"""``esmk_op_msa_project`` and ``esmk_op_msa_pair_identity`` (esm_amd/csrc/msa_build.hip) against tests/_msa_build_ref.py, exactly:
bytes, integers and fp32 bit patterns.  The projection at the edges of its dword fill (Lq around 64, 257, 1022), with one, a
few and more hits than one round of workgroups holds, on random valid local and global paths, on the degenerate ones, with a
padded row stride and a sentinel row, and on tables that lie; the identity at the edges of its 64 x 64 tile and its 128-column
chunk, on both load paths, with every special row and byte value, in row blocks and with bytes behind column L that must not
be read."""
import numpy as np
import pytest
import torch

import _msa_build_ref as ref
from _msa_build_ref import LETTERS, case, random_path, tables
from esm_amd import ops

pytestmark = pytest.mark.gpu


# ---- the projection ---------------------------------------------------------------------------------------------------------
def run_project(cols, col_offsets, blob, seq_off, lens, query, ld):
    """The device's (msa [P, ld], stats [P, 6]) in buffers prefilled with 0xEE / -77 that hold one row more; the extra rows are
    checked to be untouched."""
    P = len(col_offsets) - 1
    dev = "cuda"
    buf = torch.full((P + 1, ld), 0xEE, dtype=torch.uint8, device=dev)
    sbuf = torch.full((P + 1, 6), -77, dtype=torch.int32, device=dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cols_t = t(cols) if len(cols) else torch.zeros((0, 2), dtype=torch.int32, device=dev)
    blob_t = t(blob) if len(blob) else torch.zeros((0,), dtype=torch.uint8, device=dev)
    ops.msa_project(cols_t, t(col_offsets), blob_t, t(seq_off), t(lens), t(query), ld=ld, msa=buf[:P], stats=sbuf[:P])
    torch.cuda.synchronize()
    buf, sbuf = buf.cpu().numpy(), sbuf.cpu().numpy()
    assert (buf[P] == 0xEE).all() and (sbuf[P] == -77).all(), "the row behind the last hit was written"
    return buf[:P], sbuf[:P]


def check_project(cols, col_offsets, blob, seq_off, lens, query, ld, what):
    want_msa, want_stats = ref.project(cols, col_offsets, blob, seq_off, lens, query, ld=ld)
    msa, stats = run_project(cols, col_offsets, blob, seq_off, lens, query, ld)
    assert np.array_equal(stats, want_stats), (what, np.argwhere(stats != want_stats)[:4])
    assert np.array_equal(msa, want_msa), (what, np.argwhere(msa != want_msa)[:4])
    return msa, stats


@pytest.mark.parametrize("P", [1, 5, 300])
@pytest.mark.parametrize("Lq", [1, 63, 64, 65, 257, 1022])
def test_project_matches_the_reference(Lq, P):
    rng = np.random.default_rng(1000 * Lq + P)
    paths, seqs, query = case(rng, Lq, P, cap=96 if P == 300 else None, special=P == 5)
    cols, col_offsets, blob, seq_off, lens = tables(paths, seqs)
    up4 = (Lq + 3) // 4 * 4
    msa, stats = check_project(cols, col_offsets, blob, seq_off, lens, query, up4, (Lq, P))
    if P == 5:
        assert stats[0].tolist() == [0, 0, 0, 0, -1, -1] and stats[1].tolist() == [0, 0, 0, 0, -1, -1]
        assert stats[2].tolist()[:1] == [1] and stats[2, 4] == stats[2, 5] == Lq // 2
        assert stats[3, 0] == Lq and (msa[3, :Lq] != ref.GAP).all() and stats[3, 2] == 0  # the end insertions are not inside
        assert (msa[:2, :Lq] == ref.GAP).all()
    check_project(cols, col_offsets, blob, seq_off, lens, query, up4 + 8, (Lq, P, "ld > Lq"))


def test_project_no_hits_launches_nothing():
    dev = "cuda"
    msa, stats = ops.msa_project(torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int64, device=dev),
                                 torch.zeros((0,), dtype=torch.uint8, device=dev), torch.zeros((0,), dtype=torch.int64, device=dev),
                                 torch.zeros((0,), dtype=torch.int32, device=dev), torch.full((7,), 65, dtype=torch.uint8, device=dev))
    assert tuple(msa.shape) == (0, 8) and tuple(stats.shape) == (0, 6)


def test_project_lying_tables_write_nothing_outside_their_rows():
    rng = np.random.default_rng(7)
    Lq, P = 65, 8
    paths, seqs, query = case(rng, Lq, P)
    paths = [random_path(rng, Lq, len(s), local=False) for s in seqs]  # long paths to spoil
    paths[0][2] = (Lq, 1)                       # i >= Lq
    paths[0][3] = (Lq + 1000, -1)
    paths[1][1] = (1, len(seqs[1]))             # j >= seq_len
    paths[1][2] = (-1, len(seqs[1]) + 7)
    paths[2][0] = (-2, 0)                       # negatives other than -1
    paths[2][1] = (0, -2)
    paths[2][2] = (-100, -100)
    paths[2][3] = (-1, -1)
    paths[3][1] = (-2 ** 31, 2 ** 31 - 1)
    cols, col_offsets, blob, seq_off, lens = tables(paths, seqs)
    total = len(cols)
    check_project(cols, col_offsets, blob, seq_off, lens, query, 68, "spoiled columns")
    off = col_offsets.copy()
    off[4] = off[3] - 5                         # descending
    check_project(cols, off, blob, seq_off, lens, query, 68, "descending col_offsets")
    off = col_offsets.copy()
    off[-1] = total + 1000                      # beyond the total
    off[-2] = total + 10
    off[0] = -9
    check_project(cols, off, blob, seq_off, lens, query, 68, "col_offsets beyond the total")
    so, ln = seq_off.copy(), lens.copy()
    so[5] = len(blob) + 5                       # beyond the blob
    so[6] = -3
    so[7] = len(blob) - 2                       # the blob ends inside the hit
    ln[2] = 2 ** 31 - 1
    ln[3] = -4
    msa, stats = check_project(cols, col_offsets, blob, so, ln, query, 68, "seq_off beyond the blob")
    assert stats[5, 0] == 0 and stats[6, 0] == 0 and (msa[5:7, :Lq] == ref.GAP).all() and stats[3, 0] == 0


# ---- pairwise identity ------------------------------------------------------------------------------------------------------
def random_msa(rng, N, L, gap=ref.GAP, p_gap=0.3, letters=LETTERS[:4]):
    m = rng.choice(letters, (N, L))
    m[rng.random((N, L)) < p_gap] = gap
    return m.astype(np.uint8)


def run_identity(m, L, ld, gap=ref.GAP, min_overlap=1, base=0, tail=None, blocks=None):
    """The device's S [N, ldS] of the matrix ``m`` [N, L] laid out with row stride ``ld`` at a base offset of ``base`` bytes;
    the bytes behind column L are ``tail``.  ``blocks``: the rows per call (None: one call).  S starts as NaN."""
    N = m.shape[0]
    host = np.full((N, ld), 0xEE if tail is None else tail, dtype=np.uint8)
    host[:, :L] = m
    flat = torch.zeros((base + N * ld,), dtype=torch.uint8, device="cuda")
    flat[base:] = torch.from_numpy(host.reshape(-1)).cuda()
    view = flat[base:].view(N, ld)
    assert view.data_ptr() % 4 == base % 4
    ldS = (N + 3) // 4 * 4
    out = torch.full((N, ldS), float("nan"), dtype=torch.float32, device="cuda")
    nb = N if blocks is None else blocks
    for i0 in range(0, N, nb):
        ops.msa_pair_identity(view, L=L, gap=gap, min_overlap=min_overlap, i0=i0, nb=min(nb, N - i0), out=out[i0:i0 + min(nb, N - i0)])
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got).any(), what
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), (what, np.argwhere(got.view(np.int32) != want.view(np.int32))[:4])


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 130])
def test_pair_identity_matches_the_reference(N):
    for L in (1, 3, 4, 5, 127, 128, 129, 1022):
        rng = np.random.default_rng(100 * N + L)
        m = random_msa(rng, N, L)
        if N >= 63:
            m[3] = ref.GAP                      # an all-gap row
            m[5] = m[4]                         # identical rows
            m[6], m[7] = ref.GAP, ref.GAP       # disjoint support: 0, not NaN
            m[6, :L // 2], m[7, L // 2:] = LETTERS[0], LETTERS[1]
        want = ref.pair_identity(m, L)
        up4 = (L + 3) // 4 * 4
        same_bits(run_identity(m, L, L), want, (N, L, "ld == L"))
        # the bytes behind column L would match if they were read
        same_bits(run_identity(m, L, up4 + 4, tail=LETTERS[0]), want, (N, L, "ld rounded up, a tail that matches"))
        same_bits(run_identity(m, L, up4 + 4, tail=LETTERS[0], base=1), want, (N, L, "a base offset by one byte"))
        if N >= 63:
            assert want[6, 7] == 0.0 and (want[3, :N] == 0.0).all() and (L < 127 or want[4, 5] == 1.0)


def test_pair_identity_min_overlap_gap_byte_and_every_byte_value():
    rng = np.random.default_rng(5)
    N, L = 70, 300
    m = random_msa(rng, N, L)
    both = int(((m[0] != ref.GAP) & (m[1] != ref.GAP)).sum())
    assert both > 8
    for mo in (both - 1, both, both + 1):
        want = ref.pair_identity(m, L, min_overlap=mo)
        assert (want[0, 1] > 0) == (mo <= both)
        same_bits(run_identity(m, L, L, min_overlap=mo), want, ("min_overlap", mo))
    # every byte value present, and gap bytes other than '-': 0, 0x80 (only bit 7), 0xff
    m = rng.integers(0, 256, (N, L)).astype(np.uint8)
    m[0, :256] = np.arange(256, dtype=np.uint8)
    m[1, :256] = np.arange(256, dtype=np.uint8)[::-1]
    m[2] = m[0]
    for gap in (ref.GAP, 0, 0x80, 0xFF, ord("A")):
        g = m.copy()
        g[rng.random((N, L)) < 0.3] = gap
        want = ref.pair_identity(g, L, gap=gap, min_overlap=3)
        same_bits(run_identity(g, L, L + 4, gap=gap, min_overlap=3), want, ("gap byte", gap))
        same_bits(run_identity(g, L, L + 1, gap=gap, min_overlap=3), want, ("gap byte, odd ld", gap))


@pytest.mark.parametrize("nb", [1, 64, 65])
def test_pair_identity_row_blocks_equal_one_shot(nb):
    rng = np.random.default_rng(11)
    N, L = 130, 129
    m = random_msa(rng, N, L)
    one = run_identity(m, L, 132)
    same_bits(one, ref.pair_identity(m, L), "one shot")
    same_bits(run_identity(m, L, 132, blocks=nb), one, ("blocks of", nb))
