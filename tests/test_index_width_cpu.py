"""tests/_index_width.py without a GPU: the arithmetic of the case table (every tensor declared as crossing passes its
boundary by a whole tile, ends in a ragged tile, stays inside the entries' 2^24-row limit and the 24 GiB gate), the
sample set, the memory gate, and the discrimination of the check itself: with the boundary moved to 2^12 bytes a tiny
numpy op that wraps its store offsets, its load offsets, or a single row outside the sample set is rejected."""
import numpy as np
import pytest

import _index_width as W


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_case_table_arithmetic(name):
    case = W.CASES[name]
    assert case.tensors, name
    assert W.table_errors(case) == []
    for t in case.tensors:
        for b in t.boundaries():
            assert t.nbytes > b  # the tensor really holds the boundary


def test_the_shapes_are_the_documented_ones():
    """the rows the issue names: where each boundary falls"""
    row = lambda name, tensor, kind: W.boundary_unit(W.boundary_bytes(kind, W.CASES[name].tensor(tensor).itemsize),
                                                     W.CASES[name].tensor(tensor).unit_bytes)
    assert row("dense_t", "out", W.BYTES32) == row("dense_t", "out", W.ELEMS31) == 419_430
    assert row("fc1_15b", "out", W.BYTES32) == 104_857
    assert row("dense_f32", "out", W.BYTES32) == 209_715
    assert row("resid_elems", "out", W.ELEMS31) == 419_430 and W.CASES["resid_elems"].tensor("out").nbytes > 8 * 2 ** 30
    assert row("a_operand", "a", W.BYTES32) == 838_860
    assert row("gelu_x3", "out", W.BYTES32) == 139_810
    assert row("attention_d64", "q", W.BYTES32) == 524_288 and row("attention_d128", "ctx", W.BYTES32) == 262_144
    for name in ("attention_d64", "attention_d128"):
        s = W.CASES[name].shape
        assert s["B"] * s["H"] % 8 == 4  # the remainder branch of the XCD-grouped grid runs at the far end
    assert row("layernorm", "x", W.BYTES32) == 209_715 and row("layernorm", "y", W.BYTES31) == 209_715


@pytest.mark.parametrize("name", sorted(W.ENGINE_CASES))
def test_engine_case_arithmetic(name):
    """B * T is a multiple of the tile by construction (T = 1024): the ragged end is sequences with trailing pads"""
    case = W.ENGINE_CASES[name]
    assert W.table_errors(case, ragged_tile=False) == []
    assert case.shape["B"] * case.shape["T"] <= W.MAX_ROWS
    seq = W.boundary_sequences(case)
    assert seq == {"engine_3b": 204, "engine_15b": 102}[name]
    assert seq + 1 < case.shape["B"]  # a whole sequence lies behind the boundary
    assert W.boundary_sequences(case, "stream", W.BYTES31) == seq


def test_table_errors_speak_up():
    short = W.Case("short", "x", {}, (W.Crossing("out", 419_500, 10240, 2, (W.BYTES32,)),), 0)
    assert any("less than a tile" in e for e in W.table_errors(short))
    whole = W.Case("whole", "x", {}, (W.Crossing("out", 419_840, 10240, 2, (W.BYTES32,)),), 25 * 2 ** 30)
    errs = W.table_errors(whole)
    assert any("whole tile" in e for e in errs) and any("gate" in e for e in errs)
    many = W.Case("many", "x", {}, (W.Crossing("out", 2 ** 24 + 1, 512, 2, (W.BYTES32,)),), 0)
    assert any("2^24" in e for e in W.table_errors(many))


def test_sample_units_hold_the_boundary_rows_and_the_end():
    for case in W.CASES.values():
        for t in case.tensors:
            s = W.sample_units(t.units, t.unit_bytes, t.boundaries())
            assert s == sorted(set(s)) and s[0] == 0 and s[1] == 1 and s[-1] == t.units - 1
            assert set(range(t.units - W.TILE, t.units)) <= set(s)
            for b in t.boundaries():
                u = W.boundary_unit(b, t.unit_bytes)
                assert u * t.unit_bytes <= b < (u + 1) * t.unit_bytes
                assert set(range(u // W.TILE * W.TILE, min(t.units, u // W.TILE * W.TILE + W.TILE))) <= set(s)
            assert len(s) <= 2 + W.TILE * (len(t.kinds) + 1)


def test_chunk_list_tiles_the_units_below_the_limit():
    for case in W.CASES.values():
        widest = max(t.unit_bytes for t in case.tensors)
        n = case.tensors[0].units
        ch = W.chunk_list(n, widest)
        assert ch[0][0] == 0 and ch[-1][1] == n and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        assert all((u1 - u0) * widest < W.CHUNK_BYTES for u0, u1 in ch) and len(ch) >= 2
    ch = W.chunk_list(206 * 1024, 20480, multiple=1024)
    assert all((u1 - u0) % 1024 == 0 for u0, u1 in ch)


def test_memory_gate_names_both_numbers():
    assert W.memory_gate("x", 10 * 2 ** 30, 12 * 2 ** 30) is None
    reason = W.memory_gate("x", 10 * 2 ** 30, 12 * 2 ** 30 - 1)
    assert str(12 * 2 ** 30 - 1) in reason and str(10 * 2 ** 30) in reason


# ---- discrimination: the boundary is 2^12 bytes, the chunks stay below 2^10 --------------------------------------------
BOUNDARY = 2 ** 12
COLS = 2                       # fp32 rows of 8 bytes: row 512 begins at the boundary
ROWS = 1400                    # passes it by more than a tile, ends in a ragged one
OUTSIDE = 900                  # a row in no sample set
SENT = np.int32(W.SENT32)


def tiny_op(x, out, wrap_store=0, wrap_load=0, wrap_row=None):
    """out[r] = 3 x[r] + 1 on rows of COLS fp32; wrap_*: byte offsets taken modulo that number (a 32-bit offset in small);
    wrap_row: that row alone stores through the wrapped offset"""
    rb = COLS * 4
    xf, of = x.reshape(-1), out.reshape(-1)
    for r in range(x.shape[0]):
        src = r * rb % wrap_load if wrap_load else r * rb
        dst = r * rb % wrap_store if wrap_store and wrap_row in (None, r) else r * rb
        of[dst // 4:dst // 4 + COLS] = 3 * xf[src // 4:src // 4 + COLS] + 1


def run_check(**wrap):
    rng = np.random.default_rng(7)
    x = rng.standard_normal((ROWS, COLS)).astype(np.float32)  # i.i.d.: any two rows differ
    full = np.full((ROWS + 1, COLS), SENT, dtype=np.int32)
    tiny_op(x, full[:ROWS].view(np.float32), **wrap)
    samples = W.sample_units(ROWS, COLS * 4, [BOUNDARY])
    assert OUTSIDE not in samples and 512 in samples and ROWS - 1 in samples

    def run_chunk(u0, u1):
        out = np.full((u1 - u0, COLS), SENT, dtype=np.int32)
        tiny_op(x[u0:u1], out.view(np.float32), **wrap)  # offsets inside a chunk stay below every wrap
        return out

    def reference(u0, u1, units):
        got = full[units].view(np.float32).astype(np.float64)
        assert np.abs(got - (3 * x[units].astype(np.float64) + 1)).max() <= 2.0 ** -22 * 4

    chunks = W.chunk_list(ROWS, COLS * 4, limit=2 ** 10)
    assert len(chunks) > 8
    W.check_units(full, ROWS, SENT, chunks, run_chunk, samples, reference, max_elems=300)


def test_check_accepts_the_correct_op():
    run_check()


def test_check_rejects_wrapped_stores():
    with pytest.raises(W.IndexWidthError) as e:
        run_check(wrap_store=BOUNDARY)
    assert {"a", "c"} <= e.value.parts  # early rows overwritten, late rows never stored


def test_check_rejects_wrapped_loads():
    with pytest.raises(W.IndexWidthError) as e:
        run_check(wrap_load=BOUNDARY)
    assert "a" in e.value.parts and "c" not in e.value.parts


def test_chunk_equality_covers_rows_outside_the_sample_set():
    """one row in no sample set stores through a wrapped offset: the reference on the samples sees the overwritten early
    row only if it is sampled (it is not: row 900 lands on row 388), the chunk equality and the sentinel see both"""
    assert OUTSIDE * COLS * 4 % BOUNDARY // (COLS * 4) == 388
    assert 388 not in W.sample_units(ROWS, COLS * 4, [BOUNDARY])
    with pytest.raises(W.IndexWidthError) as e:
        run_check(wrap_store=BOUNDARY, wrap_row=OUTSIDE)
    assert e.value.parts == {"a", "c"}
    # and without a sentinel (an op that updates in place) the chunk equality alone still rejects it
    rng = np.random.default_rng(7)
    x = rng.standard_normal((ROWS, COLS)).astype(np.float32)
    full = np.full((ROWS + 1, COLS), SENT, dtype=np.int32)
    tiny_op(x, full[:ROWS].view(np.float32), wrap_store=BOUNDARY, wrap_row=OUTSIDE)
    full[OUTSIDE] = 0  # as if the row had held a residual

    def run_chunk(u0, u1):
        out = np.zeros((u1 - u0, COLS), dtype=np.int32)
        tiny_op(x[u0:u1], out.view(np.float32))
        return out

    with pytest.raises(W.IndexWidthError) as e:
        W.check_units(full, ROWS, SENT, W.chunk_list(ROWS, COLS * 4, limit=2 ** 10), run_chunk, written=False, max_elems=300)
    assert e.value.parts == {"a"}


def test_check_rejects_a_store_behind_the_end():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((ROWS, COLS)).astype(np.float32)
    full = np.full((ROWS + 1, COLS), SENT, dtype=np.int32)
    tiny_op(x, full[:ROWS].view(np.float32))
    full[ROWS, 1] = 0

    def run_chunk(u0, u1):
        out = np.zeros((u1 - u0, COLS), dtype=np.int32)
        tiny_op(x[u0:u1], out.view(np.float32))
        return out

    with pytest.raises(W.IndexWidthError) as e:
        W.check_units(full, ROWS, SENT, W.chunk_list(ROWS, COLS * 4, limit=2 ** 10), run_chunk, max_elems=300)
    assert e.value.parts == {"c"}
