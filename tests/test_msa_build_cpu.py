"""The host side of esm_amd/msa_build.py and the references of tests/_msa_build_ref.py, without a GPU: every reference against a
brute force of per-cell loops on tiny cases, the a3m text and its round trip through ``read_msa``, the first 64 records of the
reference's 1a3a example alignment (real gap patterns), the token table, the rank order, and every refusal of the Python
layer, of the parser and of the two C entries before any HIP call."""
import argparse
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

import _cluster_ref as cref
import _msa_build_ref as ref
import esm
import esm_amd
from esm_amd import _native as N
from esm_amd import msa_build as MB
from esm_amd.search import EmbeddingIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msa_build_1a3a_first64.a3m")


# ---- the references against brute force ---------------------------------------------------------------------------------------
def brute_project(cols, col_offsets, blob, seq_off, lens, query, ld):
    """Per cell (p, i): the letter of the last path column of hit p that matches query column i; per hit the six integers by
    scanning the path once per integer."""
    P, Lq, n = len(col_offsets) - 1, len(query), len(cols)
    msa = np.zeros((P, ld), dtype=np.uint8)
    stats = np.zeros((P, 6), dtype=np.int32)
    for p in range(P):
        lo = min(max(int(col_offsets[p]), 0), n)
        hi = min(max(int(col_offsets[p + 1]), lo), n)
        off = int(seq_off[p])
        length = 0 if not 0 <= off < len(blob) else min(max(int(lens[p]), 0), len(blob) - off)
        is_match = lambda c: 0 <= cols[c][0] < Lq and 0 <= cols[c][1] < length
        for i in range(ld):
            msa[p, i] = ref.GAP if i < Lq else 0
            for c in range(lo, hi):
                if is_match(c) and cols[c][0] == i:
                    msa[p, i] = blob[off + cols[c][1]]
        matches = [c for c in range(lo, hi) if is_match(c)]
        stats[p, 0] = len(matches)
        stats[p, 1] = sum(1 for c in matches if blob[off + cols[c][1]] == query[cols[c][0]])
        stats[p, 4], stats[p, 5] = (cols[matches[0]][0], cols[matches[-1]][0]) if matches else (-1, -1)
        for c in range(lo, hi):
            if matches and matches[0] < c < matches[-1] and not is_match(c):
                stats[p, 2] += cols[c][0] == -1 and 0 <= cols[c][1] < length
                stats[p, 3] += 0 <= cols[c][0] < Lq and cols[c][1] == -1
    return msa, stats


@pytest.mark.parametrize("seed", range(12))
def test_project_reference_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    Lq, P = int(rng.integers(1, 14)), int(rng.integers(5, 9))
    paths, seqs, query = ref.case(rng, Lq, P, special=True)
    cols, col_offsets, blob, seq_off, lens = ref.tables(paths, seqs)
    if seed % 3 == 1:  # lies: columns, offsets and lengths outside their buffers
        cols = cols.copy()
        for c in rng.integers(0, len(cols), 6):
            cols[c] = [(Lq, 0), (0, 99), (-2, 0), (0, -2), (-1, -1), (-7, -7)][int(rng.integers(0, 6))]
        col_offsets = col_offsets.copy()
        col_offsets[2] = col_offsets[1] - 1
        col_offsets[-1] = len(cols) + 50
        seq_off, lens = seq_off.copy(), lens.copy()
        seq_off[0], seq_off[1], lens[2], lens[3] = len(blob) + 1, -1, 10 ** 6, -5
    ld = Lq + int(rng.integers(0, 5))
    want_msa, want_stats = brute_project(cols, col_offsets, blob, seq_off, lens, query, ld)
    msa, stats = ref.project(cols, col_offsets, blob, seq_off, lens, query, ld=ld)
    assert np.array_equal(msa, want_msa) and np.array_equal(stats, want_stats)
    if seed % 3 != 1:  # the generator's paths are valid: every residue of the span once, ascending
        for p, path in enumerate(paths):
            ii = [i for i, _ in path if i >= 0]
            jj = [j for _, j in path if j >= 0]
            assert ii == list(range(ii[0], ii[0] + len(ii))) if ii else True
            assert jj == list(range(jj[0], jj[0] + len(jj))) if jj else True
            assert stats[p, 0] + stats[p, 3] == (stats[p, 5] - stats[p, 4] + 1 if stats[p, 0] else 0)


def brute_identity(m, L, gap, min_overlap):
    N_ = m.shape[0]
    S = np.zeros((N_, (N_ + 3) // 4 * 4), dtype=np.float32)
    for r in range(N_):
        for j in range(N_):
            both = same = 0
            for c in range(L):
                if m[r, c] != gap and m[j, c] != gap:
                    both += 1
                    same += int(m[r, c] == m[j, c])
            if both >= min_overlap:
                S[r, j] = np.float32(same) / np.float32(both)
    return S


@pytest.mark.parametrize("seed", range(12))
def test_pair_identity_reference_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    N_, L = int(rng.integers(1, 9)), int(rng.integers(1, 12))
    gap = [ref.GAP, 0, 0x80][seed % 3]
    m = rng.choice(np.array([65, 67, gap], dtype=np.uint8), (N_, L + 2))
    mo = int(rng.integers(1, 4))
    got = ref.pair_identity(m, L, gap, mo)
    want = brute_identity(m, L, gap, mo)
    assert not np.isnan(got).any() and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(got[:, :N_], got[:, :N_].T)


def test_reference_on_a_real_alignment():
    records = esm_amd.read_msa(GOLDEN)
    assert len(records) == 64 and len({len(s) for _, s in records}) == 1
    m = np.frombuffer("".join(s for _, s in records).encode("ascii"), dtype=np.uint8).reshape(64, -1)
    assert (m == ref.GAP).any() and not (m[0] == ref.GAP).any()
    S = ref.pair_identity(m, min_overlap=8)
    want = brute_identity(m[:12], m.shape[1], ref.GAP, 8)
    assert np.array_equal(S[:12, :12].view(np.int32), want[:12, :12].view(np.int32))
    assert (np.diag(S[:, :64]) == 1.0).all()
    # the walk at 0.9 / 0.5 on these rows: the sequential loop of _cluster_ref on the thresholded graph
    for thr in (0.9, 0.5, 0.3):
        kept = ref.redundancy_walk(S, list(range(64)), thr)
        offsets, ids, scores = cref.csr_of(S[:, :64], thr, exclude_self=True)
        _, reps, _ = cref.greedy(offsets, ids, scores, np.arange(64, dtype=np.int32))
        assert kept == reps.tolist() and kept[0] == 0
    assert 1 < len(ref.redundancy_walk(S, list(range(64)), 0.5)) < 64


# ---- rank order ---------------------------------------------------------------------------------------------------------------
def test_rank_order_and_its_ties():
    scores = [float("inf"), 3.0, 5.0, 3.0, 5.0, 1.0, 5.0]
    passed = [True, True, True, True, False, True, True]
    want = [0, 2, 6, 1, 3, 5, 4]  # by score, ties to the lower row; the failed row last
    assert ref.rank_order(scores, passed) == want
    got = MB.rank_order(torch.tensor(scores, dtype=torch.float32), torch.tensor(passed))
    assert got.tolist() == want and got.dtype == torch.int64
    rng = np.random.default_rng(3)
    for _ in range(20):
        n = int(rng.integers(1, 30))
        s = np.concatenate([[np.inf], rng.integers(0, 4, n - 1).astype(np.float32)]).astype(np.float32)
        ok = rng.random(n) < 0.7
        assert MB.rank_order(torch.from_numpy(s), torch.from_numpy(ok)).tolist() == ref.rank_order(s, ok)


def test_row_filter_and_blocks():
    stats = np.array([[10, 10, 0, 0, 0, 9], [5, 1, 0, 0, 0, 4], [4, 4, 0, 0, 0, 3], [0, 0, 0, 0, -1, -1], [7, 2, 0, 0, 1, 8]], dtype=np.int32)
    assert ref.row_filter(stats, 10, 0.5, 0.0).tolist() == [True, True, False, False, True]
    assert ref.row_filter(stats, 10, 0.0, 0.3).tolist() == [True, False, True, False, False]
    assert ref.row_filter(stats, 10, 0.0, 0.0).tolist() == [True, True, True, False, True]
    assert MB.identity_blocks(1, 1 << 30) == [(0, 1)]
    assert MB.identity_blocks(130, 1 << 30) == [(0, 130)]
    assert MB.identity_blocks(130, 65 * 132 * 4) == [(0, 64), (64, 64), (128, 2)]
    assert MB.identity_blocks(130, 1) == [(i, 1) for i in range(130)]
    for n, b in ((130, 10000), (1025, 1 << 20), (7, 100)):
        blocks = MB.identity_blocks(n, b)
        assert [i for i, _ in blocks] == list(np.cumsum([0] + [k for _, k in blocks])[:-1]) and sum(k for _, k in blocks) == n


# ---- the text -------------------------------------------------------------------------------------------------------------------
def built_on_host(insert_in="MKAVLT"):
    """A BuiltMSA held on the host: a query of 6 columns and three hits (an insertion, a deletion with unaligned ends, one
    match)."""
    query = "MKVLAT"
    seqs = ["MKGGVLAT", "WWKVATWW", "A"]
    paths = [[(0, 0), (1, 1), (-1, 2), (-1, 3), (2, 4), (3, 5), (4, 6), (5, 7)],
             [(-1, 0), (-1, 1), (1, 2), (2, 3), (3, -1), (4, 4), (5, 5), (-1, 6)],
             [(4, 0)]]
    cols, col_offsets, blob, seq_off, lens = ref.tables(paths, [np.frombuffer(s.encode(), dtype=np.uint8) for s in seqs])
    msa, stats = ref.project(cols, col_offsets, blob, seq_off, lens, query.encode(), ld=6)
    full = np.concatenate([np.frombuffer(query.encode(), dtype=np.uint8)[None], msa], 0)
    ranges = [(int(col_offsets[k]), int(col_offsets[k + 1])) for k in range(3)]
    b = esm_amd.BuiltMSA(torch.from_numpy(full.copy()), ["q", "h ins", "h del", "h one"], torch.tensor([-1, 4, 2, 9], dtype=torch.int32),
                         torch.tensor([float("inf"), 3.0, 2.0, 1.0]), torch.zeros((4, 6), dtype=torch.int32),
                         paths=(torch.from_numpy(cols), ranges, seqs))
    return b, query, seqs, paths, stats


def test_a3m_text_and_round_trip(tmp_path):
    b, query, seqs, paths, stats = built_on_host()
    assert stats.tolist() == [[6, 6, 2, 0, 0, 5], [4, 4, 0, 1, 1, 5], [1, 1, 0, 0, 4, 4]]
    assert b.records() == [("q", "MKVLAT"), ("h ins", "MKVLAT"), ("h del", "-KV-AT"), ("h one", "----A-")]
    assert b.a3m_lines() == [">q", "MKVLAT", ">h ins", "MKggVLAT", ">h del", "-KV-AT", ">h one", "----A-"]
    assert b.a3m_lines(insertions=False)[3] == "MKVLAT"
    rows = [r for _, r in b.records()]
    for ins in (True, False):
        assert "\n".join(b.a3m_lines(ins)) + "\n" == ref.a3m_text(b.labels, rows, seqs, paths, ins)
    for ins in (True, False):
        path = tmp_path / f"out{int(ins)}.a3m"
        b.write_a3m(path, insertions=ins)
        assert esm_amd.read_msa(path) == b.records()
    assert len(b) == 4
    # the module's row against the reference's on generated paths
    rng = np.random.default_rng(1)
    for _ in range(30):
        Lq, Ls = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        path = ref.random_path(rng, Lq, Ls, local=bool(rng.integers(0, 2)))
        seq = "".join(chr(c) for c in rng.choice(ref.LETTERS, Ls))
        cols, off, blob, so, ln = ref.tables([path], [np.frombuffer(seq.encode(), dtype=np.uint8)])
        row = bytes(ref.project(cols, off, blob, so, ln, b"A" * Lq, ld=Lq)[0][0]).decode()
        for ins in (True, False):
            text = MB.a3m_row(row, seq, path, ins)
            assert text == ref.a3m_row(row, seq, path, ins)
            assert "".join(ch for ch in text if not ch.islower()) == row
    with pytest.raises(ValueError, match="query column"):
        MB.a3m_row("AAAA", "CCCC", [(0, 0), (2, 1), (3, 2)])
    low, _, _, _, _ = built_on_host()
    low.msa[2, 1] = ord("k")
    with pytest.raises(ValueError, match="insertion"):
        low.a3m_lines()
    assert MB.file_name("sp|P1/x y") == "sp_P1_x_y.a3m" and MB.file_name("..") == "query.a3m"


def test_token_table_and_tokens():
    alphabet = esm.Alphabet.from_architecture("msa_transformer")
    table = MB.token_table(alphabet)
    assert table.dtype == torch.int64 and tuple(table.shape) == (256,)
    for b in range(256):
        assert int(table[b]) == alphabet.get_idx(chr(b))
    assert int(table[ord("-")]) == alphabet.get_idx("-") != alphabet.unk_idx and int(table[0]) == alphabet.unk_idx
    built, *_ = built_on_host()
    tok = built.tokens(alphabet)
    _, _, want = alphabet.get_batch_converter()(built.records())
    assert tok.dtype == torch.int64 and torch.equal(tok, want)
    with pytest.raises(ValueError, match="rows"):
        built.tokens(alphabet, max_rows=3)
    with pytest.raises(ValueError, match="columns"):
        built.tokens(alphabet, max_positions=6)
    assert MB.MAX_ROWS == 1024 and MB.MAX_POSITIONS == 1024


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def host_index(sequences=True):
    seqs = ["MKVLAT", "MKVLA"]
    return EmbeddingIndex(np.ones((2, 64), dtype=np.float32), ["a", "b"], [6, 5], seqs if sequences else None,
                          dict(layer=1, num_layers=1, embed_dim=64))


def test_python_layer_refuses_before_any_gpu_call():
    model = esm.ESM2(1, 64, 2).eval()  # on the host: a GPU call would raise RuntimeError, not ValueError
    alphabet = model.alphabet if hasattr(model, "alphabet") else esm.Alphabet.from_architecture("ESM-1b")
    q = [("q", "MKVLAT")]
    with pytest.raises(ValueError, match="no sequences"):
        esm_amd.build_msas(model, alphabet, q, host_index(False))
    index = host_index()
    for bad in (dict(depth=0), dict(depth=-3), dict(depth=2.5), dict(min_coverage=-0.1), dict(min_coverage=1.5),
                dict(min_coverage=float("nan")), dict(max_identity=1.01), dict(max_identity=float("nan")), dict(max_identity=-1),
                dict(min_query_identity=2), dict(min_query_identity=float("nan")), dict(min_overlap=0), dict(subsample="best"),
                dict(paths=False), dict(pairs=[(0, 0)]), dict(similarity="dot"), dict(return_similarity=True)):
        with pytest.raises(ValueError, match="build_msas"):
            esm_amd.build_msas(model, alphabet, q, index, **bad)
        with pytest.raises(ValueError, match="build_msas"):
            model.build_msa(alphabet, q[0], index, **bad)
    with pytest.raises(ValueError, match="gap"):  # the aligner's own checks, as search_and_align makes them
        esm_amd.build_msas(model, alphabet, q, index, gap_open=0.1, gap_extend=1.0)
    assert MB.check_args(index, max_identity=None)[2] is None
    assert MB.check_args(index)[5] == dict(mode="local", enhance=True)
    assert MB.check_args(index, align_kw=dict(mode="global", enhance=False, gap_open=2.0))[5] == dict(mode="global", enhance=False, gap_open=2.0)


def test_msa_transformer_refuses_and_exports():
    args = argparse.Namespace(layers=1, embed_dim=64, ffn_embed_dim=256, attention_heads=2, max_positions=64, max_tokens_per_msa=2 ** 14,
                              embed_positions_msa=True, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0)
    msa = esm.MSATransformer(args, esm.Alphabet.from_architecture("msa_transformer"))
    with pytest.raises(NotImplementedError, match="MSA Transformer"):
        esm_amd.build_msas(msa, None, [("q", "MKV")], host_index())
    assert not hasattr(msa, "build_msa") and not hasattr(msa, "build_msas")
    assert hasattr(esm.ESM2, "build_msa") and hasattr(esm.ProteinBertModel, "build_msas")
    assert esm_amd.build_msas is MB.build_msas and esm_amd.BuiltMSA is MB.BuiltMSA and esm_amd.msa_build is MB
    import esm_amd.build_msa as cli

    assert callable(esm_amd.build_msa) and cli.main is MB.main and callable(cli)
    with pytest.raises(NotImplementedError, match="MSA Transformer"):
        esm_amd.build_msa(msa, None, ("q", "MKV"), host_index())


def test_parser_refusals_and_defaults(capsys):
    base = ["--model-location", "m.pt", "--index", "db.npz", "--query", "q.fa", "--output-dir", "out"]
    a = MB.parse_args(base)
    assert (a.top, a.depth, a.min_coverage, a.max_identity, a.min_query_identity, a.subsample, a.mode, a.gap_open, a.gap_extend,
            a.no_enhance, a.no_insertions, a.summary) == (1024, None, 0.5, 0.9, 0.0, "first", "local", 1.0, 0.1, False, False, None)
    a = MB.parse_args(base + ["--top", "50", "--depth", "16", "--subsample", "greedy", "--mode", "global", "--no-enhance",
                              "--no-insertions", "--summary", "s.tsv", "--max-identity", "1"])
    assert (a.top, a.depth, a.subsample, a.mode, a.no_enhance, a.no_insertions, a.summary, a.max_identity) == \
        (50, 16, "greedy", "global", True, True, "s.tsv", 1.0)
    for bad in (["--top", "0"], ["--top", "1025"], ["--depth", "0"], ["--min-coverage", "1.5"], ["--max-identity", "-0.5"],
                ["--min-query-identity", "nan"], ["--subsample", "best"], ["--mode", "semiglobal"]):
        with pytest.raises(SystemExit):
            MB.parse_args(base + bad)
    with pytest.raises(SystemExit):
        MB.parse_args(base[2:])
    capsys.readouterr()


def test_op_entries_refuse_before_any_hip_call():
    L, null, p = N.lib, None, 4096  # p: a non-null, aligned address that is never dereferenced
    proj = lambda **k: L.esmk_op_msa_project(*[k.get(n, d) for n, d in (
        ("cols", p), ("n", 100), ("off", p), ("P", 4), ("seqs", p), ("nb", 100), ("so", p), ("sl", p), ("query", p), ("Lq", 65),
        ("msa", p), ("ld", 68), ("stats", p), ("stream", null))])
    for bad in (dict(off=null), dict(so=null), dict(sl=null), dict(query=null), dict(msa=null), dict(stats=null), dict(cols=null),
                dict(seqs=null), dict(n=-1), dict(nb=-1), dict(P=-1), dict(P=(1 << 24) + 1), dict(Lq=0), dict(Lq=8193, ld=8196),
                dict(ld=64), dict(ld=66), dict(ld=67), dict(P=1 << 24, ld=128), dict(cols=p + 2), dict(off=p + 4), dict(so=p + 4),
                dict(sl=p + 2), dict(msa=p + 2), dict(stats=p + 1)):
        assert proj(**bad) != 0, bad
        assert "esmk_op_msa_project" in L.esmk_last_error().decode(), bad
    assert proj(P=0) == 0                      # nothing to do: nothing is launched
    assert proj(P=0, cols=null, n=0, seqs=null, nb=0) == 0
    ident = lambda **k: L.esmk_op_msa_pair_identity(*[k.get(n, d) for n, d in (
        ("msa", p), ("N", 130), ("L", 100), ("ld", 100), ("gap", 45), ("mo", 8), ("i0", 0), ("nb", 130), ("S", p), ("ldS", 132),
        ("stream", null))])
    for bad in (dict(msa=null), dict(S=null), dict(N=0), dict(L=0), dict(ld=99), dict(L=65536, ld=65536, N=2, nb=2, ldS=4),
                dict(N=(1 << 22) + 1, nb=1, ldS=(1 << 22) + 4), dict(N=1 << 22, ld=512, L=512, nb=1, ldS=1 << 22), dict(gap=-1),
                dict(gap=256), dict(mo=0), dict(mo=-2), dict(i0=-1), dict(nb=-1), dict(i0=1), dict(i0=130, nb=1), dict(ldS=128),
                dict(ldS=131), dict(ldS=134), dict(S=p + 8), dict(S=p + 4)):
        assert ident(**bad) != 0, bad
        assert "esmk_op_msa_pair_identity" in L.esmk_last_error().decode(), bad
    assert ident(nb=0) == 0 and ident(i0=130, nb=0) == 0


# ---- the emitted code -----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_compile_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report

    path = os.path.join(tempfile.mkdtemp(prefix="isa_msa_build_"), "msa_build.s")
    isa_report.compile_asm(os.path.join(ROOT, "esm_amd", "csrc"), "msa_build.hip", path)
    meta = isa_report.meta(path)
    assert sum("msa_project_kernel" in k for k in meta) == 1 and sum("msa_pair_identity_kernel" in k for k in meta) == 2, list(meta)
    for k, (vgpr, _, scratch) in meta.items():
        assert scratch == 0 and vgpr <= 168, (k, vgpr, scratch)  # 168: three wavefronts per SIMD
