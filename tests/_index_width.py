"""Shapes, boundary arithmetic and the check of the index-width tests: every kernel family once at the smallest shape
whose byte offsets pass 2^31 and 2^32 (and whose element index passes 2^31), every output element checked.

csrc/engine_internal.h states the rule under test: row counts travel as int, every row * ld product is widened to 64
bits.  tests/test_index_width_cpu.py evaluates the case table and proves that the check discriminates (a tiny numpy op
that wraps its offsets at 2^12 bytes); tests/test_index_width_ops_gpu.py and tests/test_index_width_engine_gpu.py run
the cases.  Importing this module needs no GPU and no kernel.

A tensor is counted in UNITS of `unit_bytes`: rows of a row-major matrix, or (batch, head) planes of a [B,H,T,D] layout.
The check (`check_units`) has three parts:
  (a) chunk equality: the op runs again on consecutive chunks of units, each below CHUNK_BYTES per tensor, into a small
      scratch buffer; every chunk is bit-equal to the same units of the full run.  This is what covers ALL units.  It
      rests on properties the suite asserts elsewhere: a GEMM row's bits do not depend on M, tile height or kernel, an
      attention (b, h) on its batch, a row kernel's row on its neighbours.
  (b) fp64 reference on the sampled units (`sample_units`: 0, 1, the 256-unit tile around each boundary, the last 256),
      with the op's existing reference and tolerance: the chunks themselves are right.
  (c) no sentinel left inside the output, the guard units behind its end untouched.
A store that wraps leaves sentinel units behind (c) and overwrites early ones (a); a load that wraps computes a late unit
from an early one, and the inputs are i.i.d. random, so the bits differ (a).

The arrays the check sees are INTEGER views of the buffers (bits), sliced so that no comparison spans 2^30 elements or
more: the tests do not lean on torch's own large-index kernels.  numpy arrays and torch tensors both serve."""
import dataclasses

B31, B32 = 2 ** 31, 2 ** 32
TILE = 256               # rows of a GEMM tile: a crossing tensor passes its boundary by a whole tile and ends in a ragged one
BH_TILE = 8              # (batch, head) units of one XCD group of the attention grids
MAX_ROWS = 2 ** 24       # ESMK_MAX_ROWS (csrc/engine_internal.h)
MAX_ELEMS = 2 ** 30 - 1  # a slice handed to torch / numpy stays below 2^30 elements
CHUNK_BYTES = 2 ** 30    # a chunk of the re-run stays below this many bytes per tensor
GATE_BYTES = 24 * 2 ** 30
GATE_MARGIN = 2 * 2 ** 30
SENT16 = 0x7BFF          # tests/test_precision_ops_gpu.py SENT16 (fp16 65504); fp32: the bits of its float("nan")
SENT32 = 0x7FC00000

BYTES31, BYTES32, ELEMS31 = "2^31 bytes", "2^32 bytes", "2^31 elements"


def boundary_bytes(kind, itemsize):
    return {BYTES31: B31, BYTES32: B32, ELEMS31: B31 * itemsize}[kind]


def boundary_unit(boundary, unit_bytes):
    """the unit [u * unit_bytes, (u + 1) * unit_bytes) that holds byte offset `boundary`"""
    return boundary // unit_bytes


def sample_units(n, unit_bytes, boundaries, tile=TILE):
    """units 0 and 1, the whole `tile` around the unit of each boundary (bytes), the last `tile` units; sorted"""
    s = {0, min(1, n - 1)}
    for b in boundaries:
        u = boundary_unit(b, unit_bytes)
        if u < n:
            s.update(range(u // tile * tile, min(n, u // tile * tile + tile)))
    s.update(range(max(0, n - tile), n))
    return sorted(s)


def chunk_list(n, unit_bytes, multiple=1, limit=CHUNK_BYTES):
    """consecutive [u0, u1) covering [0, n): each below `limit` bytes of the widest tensor (unit_bytes), a multiple of
    `multiple` units long (whole sequences where rows map to (b, t))"""
    per = (limit - 1) // unit_bytes // multiple * multiple
    assert per > 0, (unit_bytes, multiple, limit)
    return [(u0, min(n, u0 + per)) for u0 in range(0, n, per)]


# ---- the case table ---------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Crossing:
    """one tensor of a case that must cross: `units` units of `unit_bytes` bytes of `itemsize`-byte elements"""
    name: str
    units: int
    unit_bytes: int
    itemsize: int
    kinds: tuple            # of BYTES31 / BYTES32 / ELEMS31
    tile: int = TILE        # TILE for rows, BH_TILE for (batch, head) units
    rows: int = 0           # rows the entry sees (checked against MAX_ROWS); 0: `units`
    ragged: bool = True     # False: the shape cannot end in a ragged tile (H = 40 planes per sequence, T = 1024 rows)

    @property
    def nbytes(self):
        return self.units * self.unit_bytes

    def boundaries(self):
        return [boundary_bytes(k, self.itemsize) for k in self.kinds]


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    op: str
    shape: dict
    tensors: tuple          # of Crossing
    peak_bytes: int         # device bytes the test holds at its peak (declared; the gate compares it with free memory)

    def tensor(self, name):
        return next(t for t in self.tensors if t.name == name)


def _gemm(name, op, M, N, K, out_item, kinds, extra=0, a_kinds=()):
    """a dense GEMM case: out [M,N] of out_item-byte elements, a [M,K] 16-bit; peak = a + out + a chunk of scratch and
    the fp32 temporaries of a random chunk (+ extra)"""
    t = [Crossing("out", M, N * out_item, out_item, kinds)] if kinds else []
    if a_kinds:
        t.append(Crossing("a", M, K * 2, 2, a_kinds))
    peak = M * K * 2 + (M + 1) * N * out_item + 4 * CHUNK_BYTES + extra
    return Case(name, op, dict(M=M, N=N, K=K), tuple(t), peak)


def _attn(name, B, H, T, D):
    plane = T * D * 2
    t = tuple(Crossing(n, B * H, plane, 2, (BYTES31, BYTES32, ELEMS31), BH_TILE, rows=B * T) for n in ("q", "k", "vt", "ctx"))
    peak = 4 * (B + 1) * H * plane + (B + 1) * H * T * 4 + 4 * CHUNK_BYTES  # the chunks read views of q, k, vt
    return Case(name, "ops.attention", dict(B=B, H=H, T=T, D=D), t, peak)


def _rows(name, op, rows, E, tensors, peak):
    return Case(name, op, dict(rows=rows, E=E), tensors, peak)


_ALL = (BYTES31, BYTES32, ELEMS31)
_R, _E = 210_000, 5120

CASES = {c.name: c for c in (
    # dense GEMM, operand-dtype out: row 419,430 holds byte 2^32 and element 2^31
    _gemm("dense_t", "ops.linear store_t / gelu_t", 419_800, 5120, 64, 2, _ALL),
    # fc1 of esm2_t48_15B: rows of 40,960 bytes
    _gemm("fc1_15b", "ops.linear gelu_t", 105_200, 20480, 64, 2, _ALL),
    # fp32 out: 2^32 bytes at row 209,715
    _gemm("dense_f32", "ops.linear store_f32 / gelu_f32 / resid_f32", 210_000, 5120, 64, 4, (BYTES31, BYTES32)),
    # the residual's element index: 8.0 GiB of fp32
    _gemm("resid_elems", "ops.linear resid_f32", 419_800, 5120, 64, 4, _ALL),
    # the A operand: rows of 5120 bytes, N = 64
    _gemm("a_operand", "ops.linear store_t", 840_000, 64, 2560, 2, (), a_kinds=_ALL),
    # f16x2: K = 64 read as 128 (hi | lo); f16x3: rows of 3 N, K3 = 192.  140,000 rows would pass 2^32 bytes (row
    # 139,810) by 190 rows only: 140,200 passes it by a whole tile and still ends in a ragged one
    _gemm("split_t", "ops.linear_split store_t / gelu_t", 419_800, 5120, 64, 2, _ALL),
    Case("gelu_x3", "ops.linear_gelu_x3", dict(M=140_200, N=5120, K=192),
         (Crossing("out", 140_200, 3 * 5120 * 2, 2, _ALL),), 140_200 * 192 * 2 + 140_201 * 3 * 5120 * 2 + 4 * CHUNK_BYTES),
    # attention: (b, h) planes of T x D; B * H % 8 == 4, so the remainder branch of the grid runs at the far end
    _attn("attention_d64", 104_900, 5, 64, 64),
    _attn("attention_d128", 52_500, 5, 64, 128),
    # q / k (RoPE) and V^T epilogues, esm2_t36_3B dims: planes (b * H + h) >= 32,768 of q, k [B,H,T,64] and vt [B,H,64,T]
    # lie past 2^32 bytes, in sequence 819 of 821; the A operand [B*T, E] crosses with them.  With H = 40 and T = 1024
    # both the plane count and the row count are whole tiles at every B: the ragged end is the odd sequence count.
    Case("qkv_rope", "esmk_op_qkv_rope2 / esmk_op_qkv_rope_ln", dict(B=821, H=40, T=1024, E=2560),
         tuple(Crossing(n, 821 * 40, 1024 * 64 * 2, 2, _ALL, BH_TILE, rows=821 * 1024, ragged=False) for n in ("q", "k", "vt")),
         4 * 822 * 1024 * 2560 * 2 + 6 * CHUNK_BYTES),
    # LayerNorm fold: the producer (residual epilogue that also writes h16 = T(out - mean_prev), rows of N + 64, and the
    # partial sums ln_part [M, N / 128 + 1, 2]) and the consumer (fc1 with the row's rstd)
    Case("ln_producer", "ops.linear_ln epilogue 4", dict(M=419_800, N=2560, K=64),
         (Crossing("out", 419_800, 2560 * 4, 4, (BYTES31, BYTES32)), Crossing("h16", 419_800, 2624 * 2, 2, (BYTES31,))),
         419_801 * (2560 * 4 + 2624 * 2 + 21 * 8) + 419_800 * 64 * 2 + 4 * CHUNK_BYTES),
    _gemm("ln_consumer", "ops.linear_ln epilogue 2", 210_000, 10240, 64, 2, _ALL),
    # [B, L, H, T, T] fp32 of 4.2 GiB: the padded attention maps (one layer of 33 written: plane (b * 33 + 32) * 20 + h
    # passes 16,384, i.e. 2^32 bytes, in sequence 24 of 26) and the input of the unfused contact head.  26 * 660 planes
    # are whole groups of 8 at every B; neither kernel groups planes.
    Case("maps_padded", "ops.attention_probs", dict(B=26, L=33, H=20, T=256),
         (Crossing("probs", 26 * 660, 256 * 256 * 4, 4, (BYTES31, BYTES32), BH_TILE, rows=26 * 256, ragged=False),),
         27 * 660 * 256 * 256 * 4 + 3 * CHUNK_BYTES),
    Case("contacts", "ops.contacts", dict(B=26, L=33, H=20, T=256),
         (Crossing("attn", 26 * 660, 256 * 256 * 4, 4, (BYTES31, BYTES32), BH_TILE, rows=26 * 256, ragged=False),),
         26 * 660 * 256 * 256 * 4 + 4 * CHUNK_BYTES),
    # learned positions of ESM-1b, in place on the fp32 stream [B, T, E] (rows = B * T: whole tiles at T = 1024, the ragged end
    # is a last sequence with trailing pads)
    Case("add_positions", "ops.add_positions", dict(B=820, T=1024, E=1280),
         (Crossing("x", 820 * 1024, 1280 * 4, 4, (BYTES31, BYTES32), ragged=False),), 821 * 1024 * 1280 * 4 + 4 * CHUNK_BYTES),
    # the fused contact head and the pair head on stacked q, k [L, B, H, T, 64] (4.0 GiB each): plane (l * B + b) * H + h
    # passes 262,144, i.e. 2^32 bytes, in layer 32 at sequence 307 of 400 (264,000 planes: whole groups of 8 at every B)
    Case("contacts_fused", "ops.contacts_fused / ops.pair_head", dict(L=33, B=400, H=20, T=128),
         tuple(Crossing(n, 33 * 400 * 20, 128 * 64 * 2, 2, _ALL, BH_TILE, rows=400 * 128, ragged=False) for n in ("q", "k")),
         2 * 33 * 400 * 20 * 128 * 64 * 2 + 5 * CHUNK_BYTES),
    # token-packed attention, head_dim 64: q, k [H, rows, 64] (rows of 128 bytes: 2^32 bytes in head 39), ctx [rows, H * 64]
    # (rows of 5120 bytes: 2^32 bytes at row 838,860).  838,912 rows would pass that row by 51 only: 839,232 rows (6556
    # segments of 128 and one of 64) pass it by a whole tile and end in a ragged one.  V^T [H, 64, rows + 64] passes 2^32
    # bytes in its last two (head, dim) rows only and is not counted.
    Case("attention_packed", "ops.attention_packed", dict(H=40, rows=839_232, D=64),
         (Crossing("q", 40 * 839_232, 128, 2, _ALL, rows=839_232, ragged=False), Crossing("k", 40 * 839_232, 128, 2, _ALL, rows=839_232, ragged=False),
          Crossing("ctx", 839_232, 40 * 64 * 2, 2, _ALL)),
         4 * 40 * 839_296 * 128 + 6 * CHUNK_BYTES),
    # MSA column maps [1, 12, 12, 513, 128, 128] fp32 of the full-size MSA configuration (4.5 GiB), layer 11 written: its
    # planes ((11 * 12 + h) * 513 + c >= 67,716) all lie past plane 65,536, i.e. 2^32 bytes
    Case("maps_msa", "ops.attention_probs(msa_C=513)", dict(Bm=1, L=12, H=12, C=513, R=128),
         (Crossing("col_maps", 12 * 12 * 513, 128 * 128 * 4, 4, (BYTES31, BYTES32), BH_TILE, rows=513 * 128, ragged=False),),
         (12 * 12 * 513 + 1) * 128 * 128 * 4 + 3 * CHUNK_BYTES),
    # LayerNorm launches of the layer loop: x, y32 fp32 cross 2^32 bytes, y (16 bit) 2^31 bytes; ldy > E: y rows of E + 64
    _rows("layernorm", "ops.layernorm / ops.layernorm_ex", _R, _E,
          (Crossing("x", _R, _E * 4, 4, (BYTES31, BYTES32)), Crossing("y32", _R, _E * 4, 4, (BYTES31, BYTES32)),
           Crossing("y", _R, _E * 2, 2, (BYTES31,)), Crossing("y_ldy", _R, (_E + 64) * 2, 2, (BYTES31,))),
          2 * (_R + 1) * _E * 4 + (_R + 1) * (_E + 64) * 2 + 4 * CHUNK_BYTES),
    # the other row kernels of the layer loop on one fp32 [210,000, 5120] buffer (B 210 x T 1000 where rows map to (b, t)):
    # embed, scale_rows, zero_gap_rows, rowstats (y 16 bit: 2^31 bytes), gather_rows, blend_rows, pool_rows, masked_row_mean
    _rows("row_kernels", "ops.embed / scale_rows / zero_gap_rows / rowstats / gather_rows / blend_rows / pool_rows / masked_row_mean", _R, _E,
          (Crossing("x", _R, _E * 4, 4, (BYTES31, BYTES32)), Crossing("y", _R, _E * 2, 2, (BYTES31,))),
          (_R + 1) * _E * 4 + (_R + 1) * _E * 2 + 5 * CHUNK_BYTES),
)}

# the whole forward (tests/test_index_width_engine_gpu.py): B sequences of T tokens; the FFN activation [B*T, 4E] in the
# operand dtype and the fp32 residual stream [B*T, E] are the tensors that cross.  peak_bytes is filled in from
# esmk_workspace_bytes by the test itself (printed), bounded here by what the shapes imply.
ENGINE_T = 1024


def _engine(name, L, E, H, B, ffn_kinds, x_kinds, note):
    rows = B * ENGINE_T
    t = (Crossing("ffn", rows, 4 * E * 2, 2, ffn_kinds), Crossing("stream", rows, E * 4, 4, x_kinds))
    return Case(name, note, dict(L=L, E=E, H=H, B=B, T=ENGINE_T), t, 0)


ENGINE_CASES = {c.name: c for c in (
    _engine("engine_3b", 2, 2560, 40, 206, (BYTES31, BYTES32, ELEMS31), (BYTES31,), "esm2_t36_3B dims, fold on and off"),
    _engine("engine_15b", 1, 5120, 40, 104, (BYTES31, BYTES32, ELEMS31), (BYTES31,), "esm2_t48_15B dims, head_dim 128"),
)}


def boundary_sequences(case, name="ffn", kind=BYTES32):
    """the sequence whose rows hold the boundary of tensor `name` of an engine case"""
    t = case.tensor(name)
    return boundary_unit(boundary_bytes(kind, t.itemsize), t.unit_bytes) // case.shape["T"]


def table_errors(case, ragged_tile=True):
    """what the CPU test asserts of a case; a list of complaints (empty: fine)"""
    bad = []
    for t in case.tensors:
        for k in t.kinds:
            u = boundary_unit(boundary_bytes(k, t.itemsize), t.unit_bytes)
            if t.units < u + 1 + t.tile:
                bad.append(f"{case.name}.{t.name}: {t.units} units pass {k} (unit {u}) by less than a tile of {t.tile}")
        if ragged_tile and t.ragged and t.units % t.tile == 0:
            bad.append(f"{case.name}.{t.name}: {t.units} units end on a whole tile of {t.tile}")
        if (t.rows or t.units) > MAX_ROWS:
            bad.append(f"{case.name}.{t.name}: more than 2^24 rows")
    if case.peak_bytes > GATE_BYTES:
        bad.append(f"{case.name}: declares {case.peak_bytes} bytes, more than the gate of {GATE_BYTES}")
    return bad


def memory_gate(case_name, peak_bytes, free_bytes):
    """None when the case may run, else the skip reason (naming both numbers)"""
    need = peak_bytes + GATE_MARGIN
    if free_bytes < need:
        return (f"{case_name}: {free_bytes} bytes of device memory free, the case needs its declared peak of {peak_bytes} "
                f"+ {GATE_MARGIN} = {need}")
    return None


# ---- the check ----------------------------------------------------------------------------------------------------------
class IndexWidthError(AssertionError):
    """raised by check_units; .parts: the failed parts of the check, a subset of {"a", "b", "c"}"""

    def __init__(self, parts, messages):
        super().__init__("; ".join(messages))
        self.parts = frozenset(parts)


def _per_unit(arr):
    n = 1
    for d in arr.shape[1:]:
        n *= int(d)
    return n


def _slices(u0, u1, per_unit, max_elems):
    step = max(1, max_elems // max(per_unit, 1))
    return [(s, min(u1, s + step)) for s in range(u0, u1, step)]


def _first_unit(mask):
    """index along dim 0 of the first true element of a boolean array (numpy or torch)"""
    idx = mask.reshape(mask.shape[0], -1).any(1).nonzero()
    return int(idx[0][0] if isinstance(idx, tuple) else idx[0, 0])


def check_units(full, n, sentinel, chunks, run_chunk, samples=(), reference=None, written=True, max_elems=MAX_ELEMS, what="out"):
    """full: integer view (bits) of the output of the full run, units along dim 0, n units + at least one guard unit
    behind them, pre-filled with `sentinel` before the run.  chunks: chunk_list(n, ...).  run_chunk(u0, u1): the bits the
    op gives for units [u0, u1) run on their own (shape of full[u0:u1]).  reference(u0, u1, units): called after each
    chunk with the sampled units inside it, raises AssertionError where the full run misses the fp64 reference.
    written=False: the op updates `full` in place (residual epilogue), so only the guards can hold the sentinel.
    An op with several outputs passes tuples for full, sentinel and what (written: one flag or a tuple), and its
    run_chunk returns a tuple: every chunk runs once.
    Raises IndexWidthError naming every failed part; all units of all chunks are compared before it does."""
    many = isinstance(full, (tuple, list))
    fulls = list(full) if many else [full]
    sents = list(sentinel) if many else [sentinel]
    names = list(what) if many else [what]
    writ = list(written) if isinstance(written, (tuple, list)) else [written] * len(fulls)
    parts, msgs = set(), []
    for f, sent, name, wr in zip(fulls, sents, names, writ):
        per = _per_unit(f)
        assert f.shape[0] > n, "no guard unit behind the output"
        # (c) guards untouched, nothing unwritten
        for s0, s1 in _slices(n, f.shape[0], per, max_elems):
            hit = f[s0:s1] != sent
            if bool(hit.any()):
                parts.add("c")
                msgs.append(f"(c) {name}: guard unit {s0 + _first_unit(hit) - n} behind the end was written")
                break
        if wr:
            for s0, s1 in _slices(0, n, per, max_elems):
                hit = f[s0:s1] == sent
                if bool(hit.any()):
                    parts.add("c")
                    msgs.append(f"(c) {name}: unit {s0 + _first_unit(hit)} still holds the sentinel (first of its slice)")
                    break
    # (a) chunk equality, (b) reference on the sampled units
    samples = sorted(samples)
    covered, seen = 0, 0
    n_bad = [0] * len(fulls)
    for u0, u1 in chunks:
        assert u0 == covered and u1 > u0, "chunks must tile [0, n)"
        covered = u1
        gots = run_chunk(u0, u1)
        gots = list(gots) if many else [gots]
        assert len(gots) == len(fulls)
        for j, (f, got, name) in enumerate(zip(fulls, gots, names)):
            assert tuple(got.shape) == tuple(f[u0:u1].shape), (name, tuple(got.shape), tuple(f[u0:u1].shape))
            for s0, s1 in _slices(u0, u1, _per_unit(f), max_elems):
                diff = f[s0:s1] != got[s0 - u0:s1 - u0]
                if bool(diff.any()):
                    if n_bad[j] == 0:
                        msgs.append(f"(a) {name}: unit {s0 + _first_unit(diff)} of the full run differs from chunk [{u0}, {u1}) run alone")
                    parts.add("a")
                    n_bad[j] += 1
        if reference is not None:
            inside = [u for u in samples if u0 <= u < u1]
            seen += len(inside)
            if inside:
                try:
                    reference(u0, u1, inside)
                except AssertionError as e:
                    parts.add("b")
                    msgs.append(f"(b) {names[0]}: sampled units of chunk [{u0}, {u1}) miss the reference: {e}")
    assert covered == n, "chunks must tile [0, n)"
    assert reference is None or seen == len(samples), "a sampled unit lies outside [0, n)"
    if parts:
        raise IndexWidthError(parts, msgs)
