"""The copy runner (esm_amd/copies.py) and the scoring orchestration on top of it, without a GPU and without the library: a stub
``esm_amd.ops`` written in plain torch from the docstrings of ops.py, and a fake model whose row-selected forward gives every
selected row a ``[V]`` vector that depends on nothing but the tokens of that row's own sequence or segment (up to its last
non-pad token) and the row's column inside it.  Under that fake the padded, token-packed and windowed forms must give what a
loop gives that builds every copy one at a time, whatever the chunk size, and must make the calls the chunk plan says."""
import math
import sys
import types

import pytest
import torch

import _windows_ref as ref
import esm_amd
from esm_amd import copies, scoring, windows

V, CLS, PAD, EOS, MASK = 33, 0, 1, 2, 32
TOKENS = torch.tensor([[CLS, 5, 6, 7, 8, EOS, PAD, PAD, PAD],
                       [CLS, 9, 10, 11, 12, 13, 14, 15, EOS]])
LENGTHS = (6, 9)
T = 9
WINDOW = 7  # sequence 0 fits, sequence 1 is windowed: R = 5 body tokens, body range [1, 8)
CHUNKS = (1, 3, None)
CHUNK_ROWS = (16, 48, None)
SETS = ([1, 3], [2, 4], [5], [1, 5], [6, 7], [4])
SET_SRC = (0, 1, 0, 1, 1, 1)


# ---- the stub of esm_amd.ops ---------------------------------------------------------------------------------------------
def _rows_of(tokens, src_rows, n):
    tokens = tokens.view(1, -1) if tokens.dim() == 1 else tokens
    return tokens, ([0] * n if src_rows is None else src_rows.tolist())


def mask_rows(tokens, positions, src_rows=None, mask_idx=32):
    tokens, rows = _rows_of(tokens, src_rows, positions.numel())
    out = tokens[rows].clone()
    out[torch.arange(len(rows)), positions.long()] = mask_idx
    return out


def mask_rows_multi(tokens, pos_offsets, positions, src_rows=None, mask_idx=32):
    tokens, rows = _rows_of(tokens, src_rows, pos_offsets.numel() - 1)
    out = tokens[rows].clone()
    for i in range(len(rows)):
        out[i, positions[int(pos_offsets[i]):int(pos_offsets[i + 1])].long()] = mask_idx
    return out


def mask_rows_packed(tokens, src_rows, seg_starts, seg_lens, pos_offsets, positions, rows, mask_idx=32, pad_idx=1, out=None):
    assert rows % 64 == 0
    out = torch.full((rows,), pad_idx, dtype=torch.int64)
    for i, (b, s, n) in enumerate(zip(src_rows.tolist(), seg_starts.tolist(), seg_lens.tolist())):
        seg = tokens[b, :n].clone()
        seg[positions[int(pos_offsets[i]):int(pos_offsets[i + 1])].long()] = mask_idx
        out[s:s + n] = seg
    return out


def window_rows(tokens, src_rows, starts, mask_offsets, mask_positions, Tw, head_tok=-1, tail_tok=-1, mask_idx=32):
    return torch.tensor(ref.window_rows_ref(tokens.tolist(), src_rows.tolist(), starts.tolist(), mask_offsets.tolist(),
                                            mask_positions.tolist(), Tw, head_tok, tail_tok, mask_idx), dtype=torch.int64)


def sum_target_rows(logprobs, target, offsets):
    out = torch.zeros((offsets.numel() - 1,), dtype=torch.float64)
    for s in range(out.numel()):
        for r in range(int(offsets[s]), int(offsets[s + 1])):
            out[s] += logprobs[r, int(target[r])].double()
    return out


STUB_OPS = types.ModuleType("esm_amd.ops")
for _fn in (mask_rows, mask_rows_multi, mask_rows_packed, window_rows, sum_target_rows):
    setattr(STUB_OPS, _fn.__name__, _fn)


@pytest.fixture(autouse=True)
def stub_ops(monkeypatch):
    """The callers import ``ops`` inside their functions: the stub stands in for it, and monkeypatch puts the real module (or
    its absence) back when the test ends."""
    monkeypatch.setitem(sys.modules, "esm_amd.ops", STUB_OPS)
    monkeypatch.setattr(esm_amd, "ops", STUB_OPS, raising=False)


# ---- the fake model --------------------------------------------------------------------------------------------------------
def row_vector(seq, col):
    """The fake's log-probabilities of column ``col`` of a sequence (a list of ints): eighths, exact in fp32 and in any sum."""
    while seq and seq[-1] == PAD:
        seq = seq[:-1]
    key = sum((k + 1) * (t + 3) for k, t in enumerate(seq))
    return ((key * 7 + col * 13 + torch.arange(V) * (key % 5 + 1)) % 101).float() / 8


class FakeWeight:
    is_cuda = True  # the only device gate of scoring._device_weight
    device = torch.device("cpu")


class FakeModel:
    alphabet_size, padding_idx, mask_idx, cls_idx, eos_idx, prepend_bos, append_eos = V, PAD, MASK, CLS, EOS, True, True

    def __init__(self, packs=True):
        self.embed_tokens = types.SimpleNamespace(weight=FakeWeight())
        self.packs = packs
        self.calls = []  # (copies, tokens) of every forward call

    def _packs(self):
        return self.packs

    def _selected_rows(self, tok, sel_rows, return_logits, *extra):
        assert sel_rows.dtype == torch.int32 and sel_rows.numel() > 0
        if extra:  # token-packed: one row space, the host segment table
            seg, = extra
            assert tok.ndim == 1 and tok.numel() % 64 == 0 and seg.dtype == torch.int32
            self.calls.append((seg.shape[0], tok.numel()))
            rows = []
            for r in sel_rows.tolist():
                start, n = next((s, n) for s, n in seg.tolist() if s <= r < s + n)
                rows.append(row_vector(tok[start:start + n].tolist(), r - start))
        else:
            assert tok.ndim == 2
            self.calls.append((tok.shape[0], tok.numel()))
            rows = [row_vector(tok[r // tok.shape[1]].tolist(), r % tok.shape[1]) for r in sel_rows.tolist()]
        lp = torch.stack(rows)
        return (lp, lp + 0.5) if return_logits else lp


# ---- the loop that builds every copy one at a time ----------------------------------------------------------------------
def copy_of(b, positions, window):
    """(the copy of sequence b with ``positions`` masked as a list, the column of every position in it)."""
    row, n = TOKENS[b].tolist(), LENGTHS[b]
    if window is None or n <= window:
        copy = list(row)
        for p in positions:
            copy[p] = MASK
        return copy, list(positions)
    R, lo, hi = ref.geometry(n, window, True, 1, 1)
    if positions[0] < lo or positions[0] >= hi:  # the source's <cls> / <eos>: the first / last window, its own special token
        p, = positions
        s = lo if p < lo else hi - R
        copy = ref.window_copy(row, s, window, True, 1, 1, CLS, EOS)
        col = 0 if p < lo else window - 1
        copy[col] = MASK
        return copy, [col]
    s = ref.start_of_set(positions, R, lo, hi)
    copy = ref.window_copy(row, s, window, True, 1, 1, CLS, EOS)
    for p in positions:
        copy[p - s + 1] = MASK
    return copy, [p - s + 1 for p in positions]


def loop_masked_marginals(window=None):
    out = torch.zeros((2, T, V))
    for b, n in enumerate(LENGTHS):
        for p in range(n):
            copy, (col,) = copy_of(b, [p], window)
            out[b, p] = row_vector(copy, col)
    return out


def loop_pll(table):
    out = torch.zeros((2,), dtype=torch.float64)
    for b, n in enumerate(LENGTHS):
        for p in range(1, n - 1):
            out[b] += table[b, p, TOKENS[b, p]].double()
    return out


def loop_wt_marginals(window=None):
    out = torch.zeros((2, T, V))
    for b, n in enumerate(LENGTHS):
        row = TOKENS[b].tolist()
        if window is None or n <= window:
            for p in range(n):
                out[b, p] = row_vector(row, p)
            continue
        R, lo, hi = ref.geometry(n, window, True, 1, 1)
        starts = ref.grid(R, lo, hi)
        for p in range(n):
            w = 0 if p < lo else len(starts) - 1 if p >= hi else ref.owner_of(p, starts, R)
            col = 0 if p < lo else window - 1 if p >= hi else p - starts[w] + 1
            out[b, p] = row_vector(ref.window_copy(row, starts[w], window, True, 1, 1, CLS, EOS), col)
    return out


def loop_masked_joint(window=None):
    rows = []
    for b, ps in zip(SET_SRC, SETS):
        copy, cols = copy_of(b, ps, window)
        rows += [row_vector(copy, c) for c in cols]
    return torch.stack(rows)


def forms():
    """(name, keyword arguments) of every form and chunk size."""
    for chunk in CHUNKS:
        yield "padded", dict(chunk=chunk)
        yield "window", dict(chunk=chunk, window=WINDOW)
    for chunk_rows in CHUNK_ROWS:
        yield "packed", dict(varlen=True, chunk_rows=chunk_rows)
    yield "window+packed", dict(varlen=True, chunk_rows=16, window=WINDOW, chunk=3)


# ---- 1. brute force --------------------------------------------------------------------------------------------------------
def test_masked_marginals_and_pseudo_log_likelihood_equal_the_loop():
    plain = loop_masked_marginals()
    for name, kw in forms():
        want = loop_masked_marginals(kw.get("window"))
        assert torch.equal(scoring.masked_marginals(FakeModel(), TOKENS, **kw), want), (name, kw)
        assert torch.equal(scoring.pseudo_log_likelihood(FakeModel(), TOKENS, **kw), loop_pll(want)), (name, kw)
        if "window" not in kw:
            assert torch.equal(want, plain)
    # a model without a token-packed forward runs varlen=True padded
    assert torch.equal(scoring.masked_marginals(FakeModel(packs=False), TOKENS, varlen=True), plain)
    assert torch.equal(scoring.pseudo_log_likelihood(FakeModel(packs=False), TOKENS, varlen=True), loop_pll(plain))
    # listed positions: the other rows stay zero
    got = scoring.masked_marginals(FakeModel(), TOKENS, positions=[[2], [0, 8]], chunk=1)
    want = torch.zeros_like(plain)
    for b, p in ((0, 2), (1, 0), (1, 8)):
        want[b, p] = plain[b, p]
    assert torch.equal(got, want)
    assert torch.equal(scoring.masked_marginals(FakeModel(), TOKENS, positions=[]), torch.zeros_like(plain))


def test_wt_marginals_equal_the_loop():
    for kw in (dict(), dict(varlen=True), dict(varlen=True, chunk_rows=16), dict(window=WINDOW), dict(window=WINDOW, varlen=True)):
        assert torch.equal(scoring.wt_marginals(FakeModel(), TOKENS, **kw), loop_wt_marginals(kw.get("window"))), kw
    for chunk in CHUNKS:
        assert torch.equal(windows.wt_marginals(FakeModel(), TOKENS, WINDOW, chunk=chunk), loop_wt_marginals(WINDOW)), chunk


def test_masked_joint_equals_the_loop():
    offsets = torch.tensor([0, 2, 4, 5, 7, 9, 10])
    pos = torch.tensor([p for ps in SETS for p in ps])
    for name, kw in forms():
        want = loop_masked_joint(kw.get("window"))
        got = scoring.masked_joint(FakeModel(), TOKENS, SETS, src=SET_SRC, **kw)
        assert len(got) == 3 and torch.equal(got[0], offsets) and torch.equal(got[1], pos), (name, kw)
        assert got[0].dtype == got[1].dtype == torch.int64 and torch.equal(got[2], want), (name, kw)
        got = scoring.masked_joint(FakeModel(), TOKENS, SETS, src=SET_SRC, return_logits=True, **kw)
        assert len(got) == 4 and torch.equal(got[0], offsets) and torch.equal(got[1], pos), (name, kw)
        assert torch.equal(got[2], want) and torch.equal(got[3], want + 0.5), (name, kw)
    got = scoring.masked_joint(FakeModel(), TOKENS, [], src=[], return_logits=True)
    assert [tuple(t.shape) for t in got] == [(1,), (0,), (0, V), (0, V)]


# ---- 2. call counts --------------------------------------------------------------------------------------------------------
def test_call_counts_follow_the_chunk_plan():
    n_copies = sum(LENGTHS)
    for chunk in CHUNKS:
        cap = copies.copies_per_call(chunk, T)
        model = FakeModel()
        scoring.masked_marginals(model, TOKENS, chunk=chunk)
        assert len(model.calls) == math.ceil(n_copies / cap) and max(c for c, _ in model.calls) <= cap
        assert sum(c for c, _ in model.calls) == n_copies
        model = FakeModel()
        scoring.masked_joint(model, TOKENS, SETS, src=SET_SRC, chunk=chunk)
        assert [c for c, _ in model.calls] == [min(cap, len(SETS) - lo) for lo in range(0, len(SETS), cap)]
        # windowed: sequence 0 runs padded at its own width; sequence 1 as 7 body copies, one <cls> copy and one <eos> copy
        model = FakeModel()
        scoring.masked_marginals(model, TOKENS, chunk=chunk, window=WINDOW)
        want = [math.ceil(6 / copies.copies_per_call(chunk, 6)), math.ceil(7 / copies.copies_per_call(chunk, WINDOW)), 1, 1]
        assert len(model.calls) == sum(want) and max(c for c, _ in model.calls) <= copies.copies_per_call(chunk, 6)
    lengths = [LENGTHS[b] for b in (0, 1) for _ in range(LENGTHS[b])]  # one copy per position, as long as its sequence
    for chunk_rows in CHUNK_ROWS:
        plan = scoring.plan_packed_chunks(lengths, scoring.CHUNK_TOKENS if chunk_rows is None else chunk_rows)
        model = FakeModel()
        scoring.masked_marginals(model, TOKENS, varlen=True, chunk_rows=chunk_rows)
        assert model.calls == [(hi - lo, rows) for lo, hi, _, rows in plan]
    assert len(scoring.plan_packed_chunks(lengths, 16)) == n_copies and len(scoring.plan_packed_chunks(lengths, 48)) == 5
    # a packed chunk without selected rows is planned but not run
    model = FakeModel()
    src, sel_off = torch.tensor([0, 1, 0]), torch.tensor([0, 2, 2, 3])
    none = torch.zeros((4,), dtype=torch.int64)
    lp = scoring._packed_copies(model, TOKENS, torch.tensor(LENGTHS), src, none, torch.zeros((0,), dtype=torch.int64), sel_off,
                                torch.tensor([1, 4, 5]), chunk_rows=16)
    assert len(scoring.plan_packed_chunks([6, 9, 6], 16)) == 3 and model.calls == [(1, 64), (1, 64)]
    row = TOKENS[0].tolist()
    assert torch.equal(lp, torch.stack([row_vector(row, 1), row_vector(row, 4), row_vector(row, 5)]))


# ---- 3. the runner alone ---------------------------------------------------------------------------------------------------
class Recorder:
    """A layout of ``n`` copies, ``chunk`` per call, that notes what the runner asks of it; row r of a call is ``[sel[r]] * 2``."""

    def __init__(self, n, chunk):
        self.built, self.ran, self.returned = [], [], []
        self.chunks = copies.even_chunks(n, chunk)

    def build(self, lo, hi):
        self.built.append((lo, hi))
        return lo, hi

    def forward(self, made, sel, return_logits):
        self.ran.append((made, sel.tolist(), return_logits))
        lp = sel.float().unsqueeze(1).repeat(1, 2)
        self.returned.append(lp)
        return (lp, lp + 100) if return_logits else lp


def test_runner_alone():
    cpu = torch.device("cpu")
    sel = torch.arange(4, dtype=torch.int32)
    for n, off, rows in ((0, torch.zeros((1,), dtype=torch.int64), sel), (2, torch.zeros((3,), dtype=torch.int64), sel[:0])):
        layout = Recorder(n, 1)
        got = copies.run_copies(layout, n, off, rows, 5, cpu)
        assert got.shape == (0, 5) and got.dtype == torch.float32 and not layout.built and not layout.ran
        lp, logits = copies.run_copies(layout, n, off, rows, 5, cpu, return_logits=True)
        assert lp.shape == logits.shape == (0, 5) and lp is not logits and not layout.built and not layout.ran
    # three chunks, the middle one without a selected row
    layout = Recorder(3, 1)
    got = copies.run_copies(layout, 3, torch.tensor([0, 1, 1, 4]), sel, 2, cpu)
    assert layout.built == [(0, 1), (2, 3)]
    assert layout.ran == [((0, 1), [0], False), ((2, 3), [1, 2, 3], False)]
    assert torch.equal(got, torch.tensor([[0., 0.], [1., 1.], [2., 2.], [3., 3.]]))
    # one chunk that ran: its tensor, not a copy of it
    assert got is not layout.returned[0]
    layout = Recorder(3, 3)
    assert copies.run_copies(layout, 3, torch.tensor([0, 1, 1, 4]), sel, 2, cpu) is layout.returned[0]
    layout = Recorder(3, 1)
    assert copies.run_copies(layout, 3, torch.tensor([0, 0, 4, 4]), sel, 2, cpu) is layout.returned[0] and layout.built == [(1, 2)]
    # return_logits: the pair, both in chunk order
    layout = Recorder(3, 2)
    lp, logits = copies.run_copies(layout, 3, torch.tensor([0, 1, 3, 4]), sel, 2, cpu, return_logits=True)
    assert layout.built == [(0, 2), (2, 3)] and all(flag for _, _, flag in layout.ran)
    assert torch.equal(lp, sel.float().unsqueeze(1).repeat(1, 2)) and torch.equal(logits, lp + 100)
    # a Layout of three callables is served as well
    layout = copies.Layout(lambda: [(0, 2)], lambda lo, hi: hi - lo, lambda made, rows, flag: rows.float().unsqueeze(1) * made)
    assert torch.equal(copies.run_copies(layout, 2, torch.tensor([0, 1, 2]), sel[:2], 1, cpu), torch.tensor([[0.], [2.]]))


def test_runner_with_an_msa_shaped_layout():
    R, C, row, chunk = 3, 5, 1, 2
    msa = torch.arange(4, 4 + R * C).view(R, C)
    sets = [[0, 2], [4], [1, 2, 3]]
    offsets, pos = copies.set_offsets(sets)
    assert offsets.tolist() == [0, 2, 3, 6] and pos.tolist() == [0, 2, 4, 1, 2, 3] and offsets.dtype == pos.dtype == torch.int64
    cell32, off32 = (pos + row * C).to(torch.int32), offsets.to(torch.int32)
    seen = []

    def build(lo, hi):
        return mask_rows_multi(msa.view(1, R * C), off32[lo:hi + 1], cell32, None, MASK).view(hi - lo, R, C)

    def forward(made, sel, return_logits):
        seen.append((tuple(made.shape), sel.tolist()))
        return made.view(-1)[sel.long()].float().unsqueeze(1)  # the token at every selected cell

    layout = copies.Layout(copies.even_chunks(len(sets), chunk), build, forward)
    sel = copies.local_rows(offsets, chunk, R * C, pos + row * C, torch.device("cpu"))
    assert sel.dtype == torch.int32
    got = copies.run_copies(layout, len(sets), offsets, sel, 1, torch.device("cpu"))
    want = [[(i - lo) * R * C + row * C + c for i in range(lo, hi) for c in sets[i]] for lo, hi in ((0, 2), (2, 3))]
    assert seen == [((2, R, C), want[0]), ((1, R, C), want[1])]
    assert torch.equal(got, torch.full((6, 1), float(MASK)))  # the selected cells are the masked ones


# ---- 4. the chunk default ------------------------------------------------------------------------------------------------
def test_copies_per_call():
    assert scoring.CHUNK_TOKENS is copies.CHUNK_TOKENS
    for width in (1, 9, 1024, copies.CHUNK_TOKENS, copies.CHUNK_TOKENS + 1, 10 ** 6):
        assert copies.copies_per_call(None, width) == max(1, copies.CHUNK_TOKENS // width)
        assert copies.copies_per_call(3, width) == 3
    for bad in (0, -1):
        with pytest.raises(ValueError, match="chunk must be positive"):
            copies.copies_per_call(bad, 9)
        for fn in (scoring.masked_marginals, scoring.pseudo_log_likelihood):
            with pytest.raises(ValueError, match="chunk must be positive"):
                fn(FakeModel(), TOKENS, chunk=bad)
            with pytest.raises(ValueError, match="chunk must be positive"):
                fn(FakeModel(), TOKENS, chunk=bad, window=WINDOW)
        for kw in (dict(), dict(window=WINDOW)):
            with pytest.raises(ValueError, match="chunk must be positive"):
                scoring.masked_joint(FakeModel(), TOKENS, SETS, src=SET_SRC, chunk=bad, **kw)
