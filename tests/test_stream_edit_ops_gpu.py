"""stream_edit_kernel through ``esmk_op_stream_edit`` (esm_amd/csrc/interventions.hip), one launch at a time, against the numpy
float32 reference of tests/_stream_edit_ref.py:

  x'              AXPBY bit for bit; PROJECT bit for bit on decided rows (the committed inputs leave none undecided)
  y, mean, rstd   of the edited rows: the bits ``esmk_op_rowstats`` gives on x'
  canaries        rows that are not selected keep their bits in all four buffers; columns [E, ldy) of y keep theirs in every row

E in {96 with ldy 128, 128, 1280, 5120} (the four register-chunk counts of the kernel; E = 96 leaves half of the lanes of the
second chunk without a column), N = 9 rows (more than one workgroup of four waves; crosses rowstats' 2-rows-per-wave and
8-rows-per-block edges), row lists of length 0, 1 and 7 with row 0, row N - 1 and the out-of-range values -1 and N, the token
selector on a token vector with <cls>, <pad>, <mask> and <eos>, sources as one vector (src_ld 0) and as rows (src_ld E) with
and without an index, fp16 and bf16 operands."""
import numpy as np
import pytest
import torch

import _stream_edit_ref as R
from esm_amd import _native as N
from esm_amd import ops

pytestmark = pytest.mark.gpu
Y_CANARY = {torch.float16: 0x7ABC, torch.bfloat16: 0x7ABC}  # bit patterns no rounding of these inputs produces
S_CANARY = -12345.678


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def edits_of(E):
    """(name, reference dict) of every edit of one size: the reference dict holds host arrays."""
    x, src, vec, index = R.ops_inputs(E)
    out = []
    for rows in R.OPS_ROW_LISTS:
        n = len(rows)
        base = dict(op=R.AXPBY, token_set=0, rows=np.array(rows, dtype=np.int32), src=None, src_index=None)
        out += [(f"scale rows{n}", dict(base, keep=0.5, gain=0.0)),
                (f"zero rows{n}", dict(base, keep=0.0, gain=0.0)),
                (f"add vec rows{n}", dict(base, keep=1.0, gain=1.5, src=vec)),
                (f"set rows rows{n}", dict(base, keep=0.0, gain=1.0, src=src[:max(n, 1)])),
                (f"axpby index rows{n}", dict(base, keep=-0.25, gain=0.3, src=src, src_index=index[:n]))]
    sel = dict(op=R.AXPBY, rows=None, token_set=R.OPS_TOKEN_SET, src=None, src_index=None)
    out += [("scale tokens", dict(sel, keep=1.0, gain=0.0)),  # the identity edit
            ("add vec tokens", dict(sel, keep=1.0, gain=-2.0, src=vec)),
            ("set rows tokens", dict(sel, keep=0.0, gain=1.0, src=src)),
            ("axpby index tokens", dict(sel, keep=0.7, gain=0.1, src=src, src_index=np.arange(R.OPS_N, dtype=np.int32)[::-1].copy())),
            ("add vec all", dict(sel, keep=1.0, gain=1.0, src=vec, token_set=(1 << 33) - 1 - 2))]
    out += [(f"project {i}", e) for i, e in enumerate(R.ops_project_cases(E))]
    zero_dir = np.array(src)
    zero_dir[3] = 0.0  # <s, s> = 0 on row 3: that row is left alone, in every buffer
    out.append(("project zero direction", dict(R.ops_project_cases(E)[1], src=zero_dir)))
    return x, out


def run(x_host, edit, E, ldy, dtype, fold):
    """One launch; returns (x', y, mean, rstd) as they are on the device afterwards."""
    x = dev(x_host)
    tokens = dev(R.OPS_TOKENS)
    y = mean = rstd = None
    if fold:
        y = torch.full((R.OPS_N, ldy), 0, dtype=torch.int16, device="cuda").fill_(Y_CANARY[dtype]).view(dtype)
        mean = torch.full((R.OPS_N,), S_CANARY, dtype=torch.float32, device="cuda")
        rstd = torch.full((R.OPS_N,), S_CANARY, dtype=torch.float32, device="cuda")
    src = None if edit["src"] is None else dev(np.asarray(edit["src"], dtype=np.float32))
    rows = None if edit["rows"] is None else dev(np.asarray(edit["rows"], dtype=np.int32))
    index = None if edit["src_index"] is None else dev(np.asarray(edit["src_index"], dtype=np.int32))
    ops.stream_edit(x, edit["op"], edit["keep"], edit["gain"], rows=rows, tokens=tokens, token_set=edit["token_set"], src=src,
                    src_index=index, y=y, mean=mean, rstd=rstd)
    return x, y, mean, rstd


def rowstats(x, ldy, dtype):
    n, E = x.shape
    y = torch.zeros((n, ldy), dtype=dtype, device="cuda")
    mean = torch.empty(n, dtype=torch.float32, device="cuda")
    rstd = torch.empty(n, dtype=torch.float32, device="cuda")
    N.check(N.lib.esmk_op_rowstats(N.ptr(x), N.ptr(y), N.ptr(mean), N.ptr(rstd), n, E, ldy, N.dtype_code(dtype), N.cur_stream()))
    return y, mean, rstd


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("E,ldy", R.OPS_SIZES)
def test_stream_edit_op(E, ldy, dtype):
    x_host, edits = edits_of(E)
    projected = undecided = 0
    for name, edit in edits:
        want, edited, ok = R.apply_edit(x_host, R.OPS_TOKENS, edit)
        if name == "project zero direction":
            assert 3 not in edited.tolist() and 3 in R.selected_rows(edit, R.OPS_TOKENS)[0].tolist()
        if edit["op"] == R.PROJECT:
            projected += edited.size
            undecided += int((~ok).sum())
        rest = np.setdiff1d(np.arange(R.OPS_N), edited)
        for fold in (True, False):
            x, y, mean, rstd = run(x_host, edit, E, ldy, dtype, fold)
            got = x.cpu().numpy()
            good = edited[ok]
            assert np.array_equal(got[good].view(np.uint32), want[good].view(np.uint32)), (name, fold, "x'")
            assert np.array_equal(got[rest].view(np.uint32), x_host[rest].view(np.uint32)), (name, fold, "unselected rows of x")
            if not fold:
                continue
            y_ref, mean_ref, rstd_ref = rowstats(x, ldy, dtype)  # on the x' the kernel wrote
            yb, mb, rb = bits(y), bits(mean), bits(rstd)
            assert np.array_equal(yb[edited, :E], bits(y_ref)[edited, :E]), (name, "y of the edited rows")
            assert np.array_equal(mb[edited], bits(mean_ref)[edited]), (name, "mean")
            assert np.array_equal(rb[edited], bits(rstd_ref)[edited]), (name, "rstd")
            canary = np.int16(Y_CANARY[dtype])
            assert (yb[:, E:] == canary).all(), (name, "columns [E, ldy) of y")
            assert (yb[rest] == canary).all(), (name, "unselected rows of y")
            s_canary = np.float32(S_CANARY).view(np.int32)
            assert (mb[rest] == s_canary).all() and (rb[rest] == s_canary).all(), (name, "unselected rows of mean / rstd")
    print(f"\nstream_edit E={E} ldy={ldy} {dtype}: {len(edits)} edits, {projected} projected rows, {undecided} undecided")
    assert undecided <= R.UNDECIDED_CAP * projected


def test_set_makes_the_rows_the_source_bits():
    """keep 0, gain 1: x' = 0 * x + 1 * s is s itself (patching): exactly, for finite x and s != -0."""
    x_host, src, _, _ = R.ops_inputs(128)
    edit = dict(op=R.AXPBY, keep=0.0, gain=1.0, rows=None, token_set=(1 << 33) - 1, src=src, src_index=None)
    x, _, _, _ = run(x_host, edit, 128, 128, torch.float16, False)
    assert np.array_equal(x.cpu().numpy().view(np.uint32), src.view(np.uint32))
