"""What packed scoring decides on the host, without a GPU: the chunk planner (``esm_amd.scoring.plan_packed_chunks``), the
argument checks of esmk_forward_packed_rows / esmk_packed_rows_workspace_bytes and of the two single-op entries (all refused
before the library touches the HIP runtime; buffers are fake non-null addresses, as in tests/test_c_abi_validation_cpu.py), the
plain-Python reference of the mask builder on a case worked by hand, and the argument errors of
``python -m esm_amd.score_sequences``."""
import ctypes
import random

import pytest
import torch

from _scoring_packed_ref import MASK, PAD, mask_rows_packed_ref, sum_target_rows_ref
from esm_amd import _native as N
from esm_amd import score_sequences
from esm_amd.scoring import CHUNK_TOKENS, plan_packed_chunks
from test_c_abi_validation_cpu import FAKE, err, make


# ---- the chunk planner ---------------------------------------------------------------------------------------------------
def check_plan(lengths, budget):
    chunks = plan_packed_chunks(lengths, budget)
    at = 0
    for lo, hi, starts, rows in chunks:
        assert lo == at and hi > lo and len(starts) == hi - lo  # every copy exactly once, in input order
        at = hi
        assert starts[0] == 0 and rows % 64 == 0 and rows > 0
        end = 0
        for s, n in zip(starts, lengths[lo:hi]):
            assert s % 16 == 0 and s >= end and (s == 0 or s > 0 and s - end < 16)  # ascending, disjoint, back to back
            end = s + n
        used = sum((n + 15) // 16 * 16 for n in lengths[lo:hi])
        assert end <= used <= rows < used + 64
        assert used <= budget or hi - lo == 1  # within the budget unless one copy alone passes it
    assert at == len(lengths)
    # greedy: the first copy of a chunk did not fit into the chunk in front of it
    for (lo0, hi0, _, _), (lo1, _, _, _) in zip(chunks, chunks[1:]):
        assert sum((n + 15) // 16 * 16 for n in lengths[lo0:hi0 + 1]) > budget and lo1 == hi0
    return chunks


def test_plan_packed_chunks_properties():
    rng = random.Random(5)
    for trial in range(200):
        n = rng.randint(1, 60)
        top = rng.choice([5, 40, 300, 1100])
        lengths = [rng.randint(1, top) for _ in range(n)]
        check_plan(lengths, rng.choice([16, 64, 100, 256, 1000, 4096, CHUNK_TOKENS]))
    assert plan_packed_chunks([], 256) == []


def test_plan_packed_chunks_by_hand():
    assert plan_packed_chunks([3], 256) == [(0, 1, [0], 64)]
    assert plan_packed_chunks([3, 16, 17, 64, 65], 65536) == [(0, 5, [0, 16, 32, 64, 128], 256)]  # 16+16+32+64+80 = 208
    # a budget of 128 rows: 16 + 16 + 32 = 64, + 64 = 128 fits exactly, 80 starts another chunk
    assert plan_packed_chunks([3, 16, 17, 64, 65], 128) == [(0, 4, [0, 16, 32, 64], 128), (4, 5, [0], 128)]
    # a copy that alone passes the budget gets a chunk of its own, in its place
    assert plan_packed_chunks([10, 300, 10], 128) == [(0, 1, [0], 64), (1, 2, [0], 320), (2, 3, [0], 64)]
    assert plan_packed_chunks([130] * 3, 256) == [(0, 1, [0], 192), (1, 2, [0], 192), (2, 3, [0], 192)]
    assert plan_packed_chunks([3] * 5)[0][2] == [0, 16, 32, 48, 64]  # the default budget
    with pytest.raises(ValueError, match="nothing to lay out"):
        plan_packed_chunks([5, 0, 7], 256)
    with pytest.raises(ValueError, match="budget"):
        plan_packed_chunks([5], 0)


# ---- the references, on cases worked by hand --------------------------------------------------------------------------
def test_mask_rows_packed_reference_by_hand():
    tokens = [[0, 5, 6, 7, 2, PAD], [0, 8, 9, 2, PAD, PAD]]
    out = mask_rows_packed_ref(tokens, [1, 0], [0, 16], [4, 5], [0, 1, 3], [2, 1, 1], [-7] * 70, 64)
    assert out[:4] == [0, 8, MASK, 2] and out[4:16] == [PAD] * 12
    assert out[16:21] == [0, MASK, 6, 7, 2] and out[21:64] == [PAD] * 43 and out[64:] == [-7] * 6
    assert sum_target_rows_ref([[1.0, 2.0], [0.5, 0.25], [4.0, 8.0]], [1, 0, 5], [0, 2, 2, 3]) == [2.5, 0.0, 8.0]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def rows_call(h, seg, rows=128, n_sel=4, tokens=FAKE, sel=FAKE, out=FAKE, ws=FAKE, packed=FAKE, ws_bytes=16, seg_null=False):
    arr = (ctypes.c_int32 * len(seg))(*seg)
    return N.lib.esmk_forward_packed_rows(h, packed, tokens, None if seg_null else arr, len(seg) // 2, rows, sel, n_sel, out, ws,
                                          ctypes.c_size_t(ws_bytes), None)


def size_call(h, seg, rows=128, n_sel=4):
    arr = (ctypes.c_int32 * len(seg))(*seg)
    n, off = ctypes.c_size_t(), ctypes.c_size_t()
    rc = N.lib.esmk_packed_rows_workspace_bytes(h, arr, len(seg) // 2, rows, n_sel, ctypes.byref(n), ctypes.byref(off))
    return rc, n.value, off.value


def test_packed_rows_argument_checks():
    rc, h = make()
    good = [0, 20, 32, 5]
    for kw in (dict(tokens=None), dict(sel=None), dict(out=None), dict(ws=None), dict(packed=None), dict(seg_null=True)):
        assert rows_call(h, good, **kw) != 0 and err() == "esmk_forward_packed_rows: null argument", kw
    assert N.lib.esmk_forward_packed_rows(None, FAKE, FAKE, (ctypes.c_int32 * 2)(0, 20), 1, 64, FAKE, 1, FAKE, FAKE,
                                          ctypes.c_size_t(16), None) != 0 and err() == "esmk_forward_packed_rows: null argument"
    assert rows_call(h, good, rows=100) != 0 and err() == "esmk_forward_packed_rows: rows must be a multiple of 64"
    assert rows_call(h, good, rows=0) != 0 and err().startswith("esmk_forward_packed_rows: n_seg and rows must be positive")
    assert rows_call(h, good, rows=(1 << 24) + 64) != 0 and err() == "esmk_forward_packed_rows: rows exceed 2^24"
    assert rows_call(h, good, n_sel=0) != 0 and err() == "esmk_forward_packed_rows: n_sel must be positive"
    assert rows_call(h, good, n_sel=-3) != 0 and err() == "esmk_forward_packed_rows: n_sel must be positive"
    assert rows_call(h, good, n_sel=(1 << 24) + 1) != 0 and err() == "esmk_forward_packed_rows: n_sel exceeds 2^24 rows"
    for seg, msg in (([0, 0], "empty segment"), ([0, 20, 24, 5], "multiples of 16"), ([16, 20], "start at row 0"),
                     ([0, 40, 32, 5], "disjoint"), ([0, 20, 112, 30], "past the last row"), ([], "n_seg and rows must be positive")):
        assert rows_call(h, seg) != 0 and err().startswith("esmk_forward_packed_rows: ") and msg in err(), (seg, err())
        rc, _, _ = size_call(h, seg)
        assert rc != 0 and err().startswith("esmk_packed_rows_workspace_bytes: ") and msg in err(), (seg, err())
    assert rows_call(h, good) != 0 and err() == "esmk_forward_packed_rows: workspace too small"  # a valid call gets this far
    N.lib.esmk_destroy(h)


def test_packed_rows_workspace_is_the_packed_forward_plus_the_head():
    rc, h = make()
    seg = [0, 20, 32, 5, 48, 130]
    n = ctypes.c_size_t()
    assert N.lib.esmk_packed_workspace_bytes(h, 3, 192, N.OUT_LOGITS, ctypes.byref(n)) == 0
    forward = n.value
    rc, small, off_small = size_call(h, seg, rows=192, n_sel=1)
    assert rc == 0, err()
    rc, large, off_large = size_call(h, seg, rows=192, n_sel=155)
    assert rc == 0, err()
    # the selected logits are the last block: fp32 [n_sel, V = 33] behind everything else
    assert forward <= off_small < small and forward < off_large < large and small < large
    assert off_small + 1 * 33 * 4 <= small and off_large + 155 * 33 * 4 <= large
    arr = (ctypes.c_int32 * 6)(*seg)
    assert N.lib.esmk_packed_rows_workspace_bytes(h, arr, 3, 192, 1, ctypes.byref(n), None) == 0 and n.value == small
    assert N.lib.esmk_packed_rows_workspace_bytes(h, arr, 3, 192, 1, None, None) != 0 and "null argument" in err()
    # the padded entry kept its sizes: the packed planning is an argument it does not pass
    pad_n, pad_off = ctypes.c_size_t(), ctypes.c_size_t()
    assert N.lib.esmk_rows_workspace_bytes(h, 2, 64, 4, ctypes.byref(pad_n), ctypes.byref(pad_off)) == 0
    assert N.lib.esmk_workspace_bytes(h, 2, 64, N.OUT_LOGITS, ctypes.byref(n)) == 0 and n.value <= pad_off.value < pad_n.value
    N.lib.esmk_destroy(h)


def test_packed_rows_refuse_handles_without_a_packed_forward():
    good = [0, 20, 32, 5]
    cfg = N.EsmkMsaConfig(2, 128, 2, 256, 33, 1, 32, 0, 2, 1, 0, 1026, 1, N.dtype_code(torch.float16))
    hm = ctypes.c_void_p()
    assert N.lib.esmk_msa_create(ctypes.byref(cfg), ctypes.byref(hm)) == 0
    assert rows_call(hm, good) != 0 and err() == "esmk_forward_packed_rows: not an ESM-2 handle"
    assert size_call(hm, good)[0] != 0 and err() == "esmk_packed_rows_workspace_bytes: not an ESM-2 handle"
    N.lib.esmk_destroy(hm)
    rc, h1 = make(no_rope=N.ESM1)
    assert rc == 0, err()
    assert rows_call(h1, good) != 0 and err().startswith("esmk_forward_packed_rows: ESM-1 ") and "no token-packed form" in err()
    assert size_call(h1, good)[0] != 0 and err().startswith("esmk_packed_rows_workspace_bytes: ESM-1 ")
    N.lib.esmk_destroy(h1)
    rc, h3 = make(weight_split=4)
    assert rc == 0, err()
    assert rows_call(h3, good) != 0 and err().startswith("esmk_forward_packed_rows: the f16x3 precision mode")
    assert size_call(h3, good)[0] != 0 and err().startswith("esmk_packed_rows_workspace_bytes: the f16x3 precision mode")
    N.lib.esmk_destroy(h3)


def test_single_op_entries_argument_checks():
    def mask(tokens=FAKE, src=FAKE, start=FAKE, length=FAKE, off=FAKE, pos=FAKE, out=FAKE, B=2, T=16, n=3, total=3, rows=64):
        return N.lib.esmk_op_mask_rows_packed(tokens, src, start, length, off, pos, out, B, T, n, total, rows, 32, 1, None)

    for name in ("tokens", "src", "start", "length", "off", "pos", "out"):
        assert mask(**{name: None}) != 0 and err() == "esmk_op_mask_rows_packed: null argument", name
    assert mask(rows=100) != 0 and "rows % 64 == 0" in err()
    assert mask(rows=0) != 0 and "rows" in err()
    assert mask(rows=-64) != 0 and "rows" in err()
    assert mask(rows=(1 << 24) + 64) != 0 and "2^24" in err()
    assert mask(n=0) != 0 and "positive" in err()
    assert mask(B=0) != 0 and "positive" in err()
    assert mask(total=-1) != 0 and "total" in err()

    def total(lp=FAKE, target=FAKE, off=FAKE, out=FAKE, n_rows=4, n_seq=2, V=33):
        return N.lib.esmk_op_sum_target_rows(lp, target, off, out, n_rows, n_seq, V, None)

    for name in ("lp", "target", "off", "out"):
        assert total(**{name: None}) != 0 and err() == "esmk_op_sum_target_rows: null argument", name
    for kw in (dict(n_rows=0), dict(n_seq=0), dict(V=0)):
        assert total(**kw) != 0 and "positive" in err(), kw


# ---- python -m esm_amd.score_sequences: argument errors ---------------------------------------------------------------
def test_score_sequences_argument_errors(tmp_path, capsys):
    table = tmp_path / "lib.csv"
    table.write_text("name,sequence\na,MKT\n")
    fasta = tmp_path / "lib.fasta"
    fasta.write_text(">a\nMKT\n")
    out = str(tmp_path / "out.csv")
    base = ["--model-location", "nowhere.pt", "--output", out]
    for argv, msg in ((base, "one of the arguments --fasta --csv is required"),
                      (base + ["--fasta", str(fasta), "--csv", str(table)], "not allowed with"),
                      (base + ["--csv", str(table)], "--csv needs --sequence-col"),
                      (base + ["--fasta", str(fasta), "--sequence-col", "sequence"], "go with --csv"),
                      (base + ["--fasta", str(fasta), "--strategy", "masked-marginals"], "invalid choice"),
                      (["--fasta", str(fasta), "--output", out], "--model-location"),
                      (["--model-location", "nowhere.pt", "--fasta", str(fasta)], "--output")):
        with pytest.raises(SystemExit) as exit_info:
            score_sequences.main(argv)
        assert exit_info.value.code == 2 and msg in capsys.readouterr().err, argv
    with pytest.raises(SystemExit, match="no column 'seq'"):
        score_sequences.main(base + ["--csv", str(table), "--sequence-col", "seq"])
    with pytest.raises(SystemExit, match="no column 'label'"):
        score_sequences.main(base + ["--csv", str(table), "--sequence-col", "sequence", "--label-col", "label"])
    args = score_sequences.create_parser().parse_args(base + ["--csv", str(table), "--sequence-col", "sequence"])
    assert score_sequences.read_records(args, None) == [("0", "MKT")] and args.strategy == "pseudo-ppl" and not args.no_varlen
    args = score_sequences.create_parser().parse_args(base + ["--fasta", str(fasta), "--no-varlen", "--strategy", "wt-marginals"])
    assert score_sequences.read_records(args, None) == [("a", "MKT")] and args.no_varlen
