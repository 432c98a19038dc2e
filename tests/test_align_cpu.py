"""Embedding-based alignment without a GPU (esm_amd/align.py): the numpy reference against brute-force enumeration, the block
planner, the refusals that come before any GPU call, the text helpers, and the emitted code of the DP kernel."""
import io
import os
import re
import sys
import tempfile

import numpy as np
import pytest
import torch

import _align_ref as ref
import esm
import esm_amd
from esm_amd import _native as N
from esm_amd import align as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


# ---- the reference itself -----------------------------------------------------------------------------------------------
def exact_S(rng, La, Lb, integer):
    """values whose sums are exact in fp32 and fp64 alike: integers in -2 .. 2 (many ties), or multiples of 2^-6 in [-2, 2]"""
    if integer:
        return rng.integers(-2, 3, size=(La, Lb)).astype(np.float32)
    return (rng.integers(-128, 129, size=(La, Lb)) / 64.0).astype(np.float32)


@pytest.mark.parametrize("integer", [False, True], ids=["random", "integer"])
@pytest.mark.parametrize("o,e", [(1.0, 0.125), (1.0, 1.0), (0.5, 0.0), (2.0, 1.0)])
def test_reference_global_score_is_the_brute_force_optimum(integer, o, e):
    rng = np.random.default_rng(5 + int(integer))
    for La in range(1, 6):
        for Lb in range(1, 6):
            S = exact_S(rng, La, Lb, integer)
            got = ref.align(S, "global", o, e)
            assert float(got["score"]) == ref.brute_force_global(S, o, e), (La, Lb, S)
            # the returned path is a global alignment and re-scores to the score
            cols = got["cols"]
            assert [i for i in cols[:, 0] if i >= 0] == list(range(La)) and [j for j in cols[:, 1] if j >= 0] == list(range(Lb))
            assert ref.rescore(S, cols, o, e) == float(got["score"])
            assert got["start"] == (0, 0) and got["end"] == (La, Lb)
            assert got["n_match"] == int(((cols[:, 0] >= 0) & (cols[:, 1] >= 0)).sum())


@pytest.mark.parametrize("integer", [False, True], ids=["random", "integer"])
def test_reference_local_path_rescores(integer):
    rng = np.random.default_rng(9)
    for La, Lb in [(1, 1), (3, 7), (12, 9), (20, 20)]:
        S = exact_S(rng, La, Lb, integer)
        got = ref.align(S, "local", 1.0, 0.25)
        cols = got["cols"]
        assert float(got["score"]) >= 0
        assert ref.rescore(S, cols, 1.0, 0.25) == float(got["score"])
        if len(cols):  # a local alignment starts and ends with a match and covers start .. end
            assert cols[0].min() >= 0 and cols[-1].min() >= 0
            assert tuple(cols[0]) == got["start"] and tuple(cols[-1] + 1) == got["end"]
        # no cell is better, and the end cell is the first of its value in row-major order
        H = got["H"]
        assert float(got["score"]) == float(H.max())
        assert got["end"] == tuple(int(v) for v in np.argwhere(H == H.max())[0])
    none = ref.align(-np.ones((4, 6), dtype=np.float32), "local", 1.0, 0.1)
    assert float(none["score"]) == 0 and len(none["cols"]) == 0 and none["end"] == (0, 0)


def test_reference_affine_gap_beats_two_short_ones():
    # matches on the diagonal except residues 3 .. 6 of a, which have no partner: one gap of 4 costs o + 3 e = 1.75; a linear
    # reading (4 o) would rather take the poor matches
    La, Lb = 10, 6
    S = np.full((La, Lb), -0.6, dtype=np.float32)
    for k in range(3):
        S[k, k] = 1
        S[k + 7, k + 3] = 1
    got = ref.align(S, "global", 1.0, 0.25)
    assert float(got["score"]) == 6 - 1.75
    assert [tuple(c) for c in got["cols"][3:7]] == [(3, -1), (4, -1), (5, -1), (6, -1)]


# ---- the planner --------------------------------------------------------------------------------------------------------
def check_plan(len_a, len_b, pairs, E, max_bytes, **kw):
    blocks = A.plan_blocks(len_a, len_b, pairs, E, max_bytes, **kw)
    seen = np.zeros(len(pairs), dtype=np.int64)
    for a0, a1, b0, b1, idx in blocks:
        assert 0 <= a0 < a1 <= len(len_a) and 0 <= b0 < b1 <= len(len_b) and len(idx) > 0
        p = np.asarray(pairs)[idx]
        assert ((p[:, 0] >= a0) & (p[:, 0] < a1) & (p[:, 1] >= b0) & (p[:, 1] < b1)).all()
        seen[idx] += 1
        local = p - np.array([a0, b0])
        assert A.block_bytes(len_a[a0:a1], len_b[b0:b1], local, E, **kw) <= max_bytes
    assert (seen == 1).all()
    return blocks


def test_plan_blocks():
    rng = np.random.default_rng(3)
    len_a = rng.integers(20, 400, size=13).tolist()
    len_b = rng.integers(20, 700, size=29).tolist()
    every = A.check_pairs(None, 13, 29)
    assert len(check_plan(len_a, len_b, every, 320, 4 << 30)) == 1
    small = check_plan(len_a, len_b, every, 320, 6 << 20)
    assert len(small) > 4
    assert len(check_plan(len_a, len_b, every, 320, 6 << 20, paths=False)) <= len(small)
    check_plan(len_a, len_b, every, 320, 6 << 20, enhance=True)
    # a sparse list: rectangles without a listed pair give no block
    sparse = np.array([(0, 0), (12, 28), (5, 17)])
    blocks = check_plan(len_a, len_b, sparse, 320, 3 << 20)
    assert len(blocks) <= 3 and sum(len(b[4]) for b in blocks) == 3
    assert A.plan_blocks(len_a, len_b, np.zeros((0, 2), dtype=np.int64), 320, 1 << 20) == []
    # the same arguments give the same plan; a budget below one pair is refused
    again = A.plan_blocks(len_a, len_b, every, 320, 6 << 20)
    assert [b[:4] for b in again] == [b[:4] for b in small]
    one = A.block_bytes([300], [300], [(0, 0)], 320)
    assert len(A.plan_blocks([300], [300], [(0, 0)], 320, one)) == 1
    with pytest.raises(ValueError, match="does not hold the pair"):
        A.plan_blocks([300], [300], [(0, 0)], 320, one - 1)
    with pytest.raises(ValueError, match="does not hold the pair"):
        A.plan_blocks(len_a, len_b, every, 320, 100 << 10)
    # a side b beyond one panel counts the boundary-column workspace
    assert A.block_bytes([10], [600], [(0, 0)], 64, panel=512) - A.block_bytes([10], [600], [(0, 0)], 64, panel=1024) == 8 * 11


def test_pair_table():
    table, size = A.pair_table([0, 5], [5, 3], [0, 8], [7, 17])
    assert table.tolist() == [[0, 5, 0, 7, 0], [5, 3, 8, 17, 80]] and size == 80 + 3 * 32


# ---- refusals before any GPU call ---------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_gpu():
    x = [torch.zeros(5, 64)]  # CPU tensors: a call in order would be refused as such, last of all
    with pytest.raises(ValueError, match="exceeds gap_open"):
        esm_amd.align_embeddings(x, x, gap_open=0.5, gap_extend=1.0)
    for kw in (dict(gap_open=-1.0), dict(gap_extend=-0.1), dict(gap_open=float("nan")), dict(gap_open=float("inf"))):
        with pytest.raises(ValueError, match="finite and >= 0"):
            esm_amd.align_embeddings(x, x, **kw)
    with pytest.raises(ValueError, match="mode"):
        esm_amd.align_embeddings(x, x, mode="semiglobal")
    with pytest.raises(ValueError, match="similarity"):
        esm_amd.align_embeddings(x, x, similarity="euclid")
    with pytest.raises(ValueError, match="8193 residues"):
        esm_amd.align_embeddings(x, [torch.zeros(8193, 64)])
    with pytest.raises(ValueError, match="0 residues"):
        esm_amd.align_embeddings((torch.zeros(5, 64), [5, 0]), x)
    with pytest.raises(ValueError, match="sum to"):
        esm_amd.align_embeddings((torch.zeros(5, 64), [2, 2]), x)
    with pytest.raises(ValueError, match="E = 64"):
        esm_amd.align_embeddings(x, [torch.zeros(5, 128)])
    with pytest.raises(RuntimeError, match="MI355X"):
        esm_amd.align_embeddings(x, x)
    with pytest.raises(ValueError, match="listed twice"):
        A.check_pairs([(0, 1), (0, 1)], 2, 2)
    with pytest.raises(ValueError, match="pairs must index"):
        A.check_pairs([(0, 2)], 2, 2)
    assert A.check_pairs(None, 2, 3).tolist() == [[0, 0], [0, 1], [0, 2], [1, 0], [1, 1], [1, 2]]


def test_model_refusals():
    model = esm.ESM2(2, 64, 2).eval()
    toks = torch.zeros(1, 8, dtype=torch.int64)
    for layer in (-1, 3):
        with pytest.raises(ValueError, match="outside 0 .. 2"):
            model.align(toks, toks, layer=layer)
    with pytest.raises(NotImplementedError, match="window"):
        model.align(toks, toks, window=1024)
    with pytest.raises(ValueError, match="exceeds gap_open"):
        model.align(toks, toks, gap_open=0.1, gap_extend=0.2)
    long = torch.full((1, 8195), 5, dtype=torch.int64)
    with pytest.raises(ValueError, match="8193 residues"):
        model.align(toks, long)
    assert esm.ProteinBertModel.align is esm.ESM2.align


def test_msa_transformer_refuses():
    import argparse

    args = argparse.Namespace(layers=1, embed_dim=64, ffn_embed_dim=256, attention_heads=2, max_positions=64, max_tokens_per_msa=2 ** 14,
                              embed_positions_msa=True, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0)
    msa = esm.MSATransformer(args, esm.Alphabet.from_architecture("msa_transformer"))
    toks = torch.zeros(1, 2, 8, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="MSA Transformer"):
        A.align(msa, toks, toks)
    assert not hasattr(msa, "align")


def test_op_entries_refuse_before_any_hip_call():
    L, null, p = N.lib, None, 4096  # p: a non-null, aligned address that is never dereferenced
    assert L.esmk_op_align_panel() % 64 == 0
    assert L.esmk_op_align_rows(null, 64, 4, null, 4, 1, 0, p, 192, 64, null) != 0
    assert L.esmk_op_align_rows(p, 64, 4, null, 4, 1, 0, p, 191, 64, null) != 0
    assert L.esmk_op_align_rows(p, 64, 4, null, 4, 2, 0, p, 192, 64, null) != 0
    dp = lambda **k: L.esmk_op_align_dp(*[k.get(n, d) for n, d in (
        ("S", p), ("ld", 64), ("rows", 8), ("cols", 64), ("table", p), ("n", 1), ("mode", 0), ("o", 1.0), ("e", 0.1), ("la", 8),
        ("lb", 8), ("score", p), ("end", p), ("tb", p), ("tbn", 1024), ("want", 1), ("ws", null), ("wsn", 0), ("stream", null))])
    for bad in (dict(e=2.0), dict(e=-0.1), dict(o=float("inf")), dict(o=float("nan")), dict(la=8193), dict(lb=0), dict(mode=2),
                dict(cols=60), dict(ld=60), dict(S=p + 4), dict(tb=null), dict(lb=8192), dict(lb=8192, ws=p, wsn=17),
                dict(score=null), dict(n=-1)):
        assert dp(**bad) != 0, bad
        assert "esmk_op_align_dp" in L.esmk_last_error().decode()
    assert dp(n=0) == 0  # nothing to do: nothing is launched
    assert L.esmk_op_align_enhance(p, 64, 8, 64, p, 1, 8, null, 0, null) != 0
    assert L.esmk_op_align_enhance(p, 64, 8, 64, p, 1, 8193, p, 1 << 20, null) != 0
    assert L.esmk_op_align_traceback(p, 1, 0, p, null, 64, p, p, 16, p, p, p, null) != 0
    assert L.esmk_op_align_traceback(p, 1, 3, p, p, 64, p, p, 16, p, p, p, null) != 0


# ---- text ---------------------------------------------------------------------------------------------------------------
def test_alignment_strings_and_tsv():
    cols = [(0, -1), (1, 0), (2, 1), (-1, 2), (3, 3)]
    assert esm_amd.alignment_strings("MKVL", "KVAL", cols) == ("MKV-L", "-KVAL")
    assert esm_amd.alignment_strings("MKVL", "KVAL", torch.tensor(cols, dtype=torch.int32)) == ("MKV-L", "-KVAL")
    assert esm_amd.alignment_strings("MK", "KV", np.zeros((0, 2))) == ("", "")
    fh = io.StringIO()
    A.write_tsv(fh, [dict(query="q1", target="t1", score=3.25, la=4, lb=8, n_match=3, start=[1, 0], end=[4, 3]),
                     dict(query="q1", target="t2", score=0.0, la=4, lb=5, n_match=0, start=[0, 0], end=[0, 0]),
                     dict(query="q2", target="t1", score=-1.5, la=3, lb=8)])
    lines = fh.getvalue().splitlines()
    assert lines[0].split("\t") == list(A.TSV_HEADER)
    assert lines[1].split("\t") == ["q1", "t1", "3.2500", "0.8125", "3", "2-4", "1-3"]
    assert lines[2].split("\t") == ["q1", "t2", "0.0000", "0.0000", "0", "-", "-"]
    assert lines[3].split("\t") == ["q2", "t1", "-1.5000", "-0.5000", "-", "-", "-"]


def test_cli_parser_and_exports():
    a = A.parse_args(["--model-location", "m.pt", "--query", "q.fa", "--target", "t.fa", "--output", "hits.tsv", "--mode", "local",
                      "--top", "5", "--enhance", "--gap-open", "2", "--layer", "12"])
    assert (a.mode, a.top, a.enhance, a.gap_open, a.gap_extend, a.layer, a.similarity) == ("local", 5, True, 2.0, 0.1, 12, "cosine")
    assert esm_amd.align_embeddings is A.align_embeddings and esm_amd.alignment_strings is A.alignment_strings


# ---- the emitted code ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_dp_kernel_compiles_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report

    path = os.path.join(tempfile.mkdtemp(prefix="isa_align_"), "align.s")
    isa_report.compile_asm(os.path.join(ROOT, "esm_amd", "csrc"), "align.hip", path)
    meta = isa_report.meta(path)
    kernels = [k for k in meta if re.search(r"align_dp_kernel", k)]
    assert len(kernels) == 1, list(meta)
    vgpr, _, scratch = meta[kernels[0]]
    assert scratch == 0 and vgpr <= 128, (vgpr, scratch)  # 128: four wavefronts per SIMD
    assert all(meta[k][2] == 0 for k in meta if "align_" in k), meta
