"""The host side of MSA row selection without a GPU: the numpy references of tests/_msa_select_ref.py against answers worked
out by hand, the neighbour threshold rule, the golden lists of the reference notebook's own ``greedy_select`` against the
integer rule, the argument checks of the five new C entries (refused before any HIP call, on fake pointers as in
tests/test_sampling_cpu.py), strategy "first", ``read_msa(path, None)`` and the two command lines."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _msa_select_ref as M
import esm_amd
from esm_amd import _native as N
from esm_amd import msa_select, predict_msa

FAKE = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused first
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msa_select_greedy.json")

# three rows of five columns; byte 200 and byte 0 are symbols like any other
TOY = np.array([[65, 66, 67, 0, 200],
                [65, 66, 68, 0, 72],
                [70, 66, 67, 1, 200]], dtype=np.uint8)


def err():
    return N.lib.esmk_last_error().decode()


# ---- the references ---------------------------------------------------------------------------------------------------------
def test_mismatch_and_neighbour_counts_known_answers():
    assert M.mism(TOY).tolist() == [[0, 2, 2], [2, 0, 4], [2, 4, 0]]
    assert M.mism(TOY, L=3).tolist() == [[0, 1, 1], [1, 0, 2], [1, 2, 0]]  # the columns past L never count
    assert M.mismatch_rows(TOY, [1, -4, 7]).tolist() == [[2, 0, 4], [0, 2, 2], [2, 4, 0]]  # indices clamped to [0, N)
    assert M.neighbor_counts(TOY, -1).tolist() == [0, 0, 0]
    assert M.neighbor_counts(TOY, 0).tolist() == [1, 1, 1]
    assert M.neighbor_counts(TOY, 2).tolist() == [3, 2, 2]
    assert M.neighbor_counts(TOY, 3).tolist() == [3, 2, 2]
    assert M.neighbor_counts(TOY, 5).tolist() == [3, 3, 3]
    assert M.neighbor_counts(TOY, 1, L=3).tolist() == [3, 2, 2]


def test_greedy_known_answers():
    # from row 0: sums (., 2, 2): a tie, the lower row wins; then row 2
    assert M.greedy(TOY, 3, 0, 0) == [0, 1, 2] and M.greedy(TOY, 3, 0, 1) == [0, 1, 2]
    assert M.greedy(TOY, 2, 1, 0) == [1, 2] and M.greedy(TOY, 2, 1, 1) == [1, 0]  # from row 1: sums (2, ., 4)
    assert M.greedy(TOY, 1, 2, 0) == [2]
    four = np.vstack([TOY, TOY[1:2]])  # row 3 duplicates row 1
    assert M.greedy(four, 3, 0, 0) == [0, 1, 2]  # sums after row 0: (., 2, 2, 2); after row 1: (., ., 6, 2)
    assert M.greedy(four, 3, 0, 1) == [0, 1, 3]  # the smallest: the duplicate of the row picked last


def test_ranks_and_race_keys_known_answers():
    nan, inf = float("nan"), float("inf")
    assert M.ranks([0.5, nan, 0.5, inf, -1.0, nan, inf]).tolist() == [1, 5, 2, 3, 0, 6, 4]
    assert M.ranks([nan, nan]).tolist() == [0, 1] and M.ranks([2.0]).tolist() == [0]
    assert M.ranks([0.0, -0.0]).tolist() == [0, 1]  # equal keys: the lower index
    u = M.race_u(64, 7, 3)
    assert u.dtype == np.float64 and (u >= 0).all() and (u < 1).all() and len(set(u.tolist())) == 64
    assert ((u * 2.0 ** 24) == np.round(u * 2.0 ** 24)).all()  # 24-bit fractions
    assert not np.array_equal(u, M.race_u(64, 7, 4)) and not np.array_equal(u, M.race_u(64, 8, 3))
    import _sampling_ref as R

    assert int(R.word0(7, 3, 0, 2, 5)) >> 8 == int(u[5] * 2.0 ** 24)  # counter (subsample, 0, 2, i): purpose 2
    c = np.arange(64) - 1
    key = M.race_keys(64, 7, 3, c)
    assert key[0] == inf and key[1] == inf and key[2] == -np.log(u[2]) and key[9] == -np.log(u[9]) * 8.0
    assert np.array_equal(M.race_keys(64, 7, 3), -np.log(u))
    pick = M.weighted_pick(64, 10, 7, 3)
    assert pick[0] == 0 and len(pick) == 10 and pick == sorted(set(pick))
    assert M.min_relative_gap([1.0, 1.0, 2.0, inf, 4.0]) == 0.5


def test_the_generator_is_seeded_and_holds_a_duplicate():
    a = M.family_msa(257, 65, 3)
    assert a.shape == (257, 65) and a.dtype == np.uint8 and np.array_equal(a, M.family_msa(257, 65, 3))
    assert not np.array_equal(a, M.family_msa(257, 65, 4))
    assert np.array_equal(a[256], a[128]) and set(np.unique(a).tolist()) <= set(M.ALPHABET.tolist())
    c = M.neighbor_counts(a, M.max_mismatch(0.2, 65))
    assert c.min() >= 1 and c.max() > 4 and c[256] == c[128] >= 2  # families: some rows have many neighbours
    recs = M.records(a)
    assert recs[5] == ("seq5", bytes(a[5].tolist()).decode()) and len(recs) == 257


# ---- a row is a neighbour when mism < theta * L ------------------------------------------------------------------------------
def test_max_mismatch_rule():
    """The largest integer m with float(m) < theta * L, that product in fp64.  0.2 * 65 is 13.0 exactly in fp64 (the error of
    0.2 is below half an ulp of 13), so 13 mismatches are a distance of exactly theta, not below it: 12.  At L = 64 the
    product is 12.8: 12 again; at L = 66 it is 13.2: 13."""
    assert 0.2 * 65 == 13.0
    for theta, L, want in ((0.2, 65, 12), (0.2, 64, 12), (0.2, 66, 13), (0.2, 5, 0), (0.2, 4, 0), (0.2, 6, 1), (0.5, 64, 31),
                           (0.5, 65, 32), (1.0, 64, 63), (1.5, 64, 64), (0.0, 64, -1), (-0.3, 64, -1), (0.01, 64, 0),
                           (0.25, 1021, 255), (0.3, 10, 2)):  # fp64 rounds 0.3 * 10 to 3.0: 2
        assert msa_select.max_mismatch(theta, L) == want, (theta, L)
        assert M.max_mismatch(theta, L) == want, (theta, L)
    for L in range(1, 300):
        for theta in (0.1, 0.2, 0.3, 0.62, 0.9):
            m = msa_select.max_mismatch(theta, L)
            assert m == M.max_mismatch(theta, L)
            assert (m < 0 or float(m) < theta * L) and not float(m + 1) < theta * L


# ---- the notebook's own choice ---------------------------------------------------------------------------------------------
def test_integer_greedy_reproduces_the_notebook_lists():
    """tests/golden/msa_select_greedy.json holds what the reference notebook's ``greedy_select`` returned for the generator
    alignment (tests/golden/make_golden_msa_select.py).  At L = 64 its float means are exact, so the integer rule agrees."""
    with open(GOLDEN) as fh:
        g = json.load(fh)
    gen = g["generator"]
    assert (gen["n"], gen["L"], g["num_seqs"]) == (257, 64, 32)
    a = M.family_msa(gen["n"], gen["L"], gen["seed"])
    assert sorted(M.greedy(a, g["num_seqs"], 0, 0)) == g["max"]
    assert sorted(M.greedy(a, g["num_seqs"], 0, 1)) == g["min"]
    assert g["max"] != g["min"] and g["max"][0] == g["min"][0] == 0


# ---- the C entries refuse bad arguments before any HIP call -----------------------------------------------------------------
def test_msa_select_op_argument_checks():
    lib = N.lib

    def rows(msa=FAKE, n=8, L=5, ld=5, query=FAKE, nq=2, out=FAKE):
        return lib.esmk_op_msa_mismatch_rows(msa, n, L, ld, query, nq, out, None)

    def counts(msa=FAKE, n=8, L=5, ld=5, m=1, out=FAKE):
        return lib.esmk_op_msa_neighbor_counts(msa, n, L, ld, m, out, None)

    def greedy(msa=FAKE, n=8, L=5, ld=5, first=0, num=3, mode=0, work=FAKE, sel=FAKE):
        return lib.esmk_op_msa_greedy_select(msa, n, L, ld, first, num, mode, work, sel, None)

    for call, who, nulls in ((rows, "esmk_op_msa_mismatch_rows", ("msa", "query", "out")),
                             (counts, "esmk_op_msa_neighbor_counts", ("msa", "out")),
                             (greedy, "esmk_op_msa_greedy_select", ("msa", "work", "sel"))):
        for name in nulls:
            assert call(**{name: None}) != 0 and err() == who + ": null argument", (who, name)
        for kw in (dict(n=0), dict(n=-1), dict(L=0), dict(L=-3)):
            assert call(**kw) != 0 and who + ": N and L must be positive" in err(), (who, kw)
        assert call(L=6) != 0 and who + ": ld must not be smaller than L" in err()
        for kw in (dict(n=1 << 16, L=5, ld=1 << 15), dict(n=(1 << 31) - 1, L=1, ld=2), dict(n=1 << 20, L=100, ld=1 << 11)):
            assert call(**kw) != 0 and who + ": N * ld must be below 2^31" in err(), (who, kw)
        assert call(n=2, L=65536, ld=65536) != 0 and who + ": L must not exceed 65535" in err()
    for nq in (0, -1):
        assert rows(nq=nq) != 0 and "esmk_op_msa_mismatch_rows: nq must be positive" in err()
    assert rows(n=1 << 20, nq=1 << 11) != 0 and "esmk_op_msa_mismatch_rows: nq * N must be below 2^31" in err()
    for num in (0, -1, 9):
        assert greedy(num=num) != 0 and "esmk_op_msa_greedy_select: num must be in 1 .. N" in err(), num
    for first in (-1, 8, 1 << 30):
        assert greedy(first=first) != 0 and "esmk_op_msa_greedy_select: first must be in [0, N)" in err(), first
    # (num * L >= 2^31 cannot be reached from outside: num <= N and L <= ld, and N * ld >= 2^31 is refused first)
    for mode in (-1, 2):
        assert greedy(mode=mode) != 0 and "esmk_op_msa_greedy_select: mode must be 0" in err(), mode

    def keys(count=None, n=8, seed=1, sub=0, out=FAKE):
        return lib.esmk_op_msa_race_keys(count, n, seed, sub, out, None)

    assert keys(out=None) != 0 and err() == "esmk_op_msa_race_keys: null argument"
    for n in (0, -5, (1 << 24) + 1):
        assert keys(n=n) != 0 and "esmk_op_msa_race_keys: N must be in 1 .. 2^24" in err(), n
    assert keys(sub=-1) != 0 and "esmk_op_msa_race_keys: subsample must not be negative" in err()
    for kw in (dict(key=None), dict(rank=None)):
        a = dict(key=FAKE, rank=FAKE)
        a.update(kw)
        assert lib.esmk_op_rank_keys(a["key"], a["rank"], 8, None) != 0 and err() == "esmk_op_rank_keys: null argument"
    for n in (0, -1, (1 << 24) + 1):
        assert lib.esmk_op_rank_keys(FAKE, FAKE, n, None) != 0 and "esmk_op_rank_keys: N must be in 1 .. 2^24" in err(), n


# ---- the Python layer without a GPU ---------------------------------------------------------------------------------------------
def test_strategy_first_and_small_msas_need_no_gpu():
    msa = M.records(M.family_msa(9, 12, 0))
    assert msa_select.subsample_indices(msa, 4, "first") == [0, 1, 2, 3]
    assert msa_select.subsample_msa(msa, 4, "first") == msa[:4]
    for strategy in msa_select.STRATEGIES:  # an MSA that is not deeper than num_seqs is returned whole
        assert msa_select.subsample_indices(msa, 9, strategy) == list(range(9))
        assert msa_select.subsample_msa(msa, 400, strategy) == msa
    toks = torch.arange(40).view(8, 5)
    assert torch.equal(msa_select.subsample_msa(toks, 3, "first"), toks[:3])
    assert torch.equal(msa_select.subsample_msa(toks[None], 3, "first"), toks[None, :3])
    assert esm_amd.subsample_msa(msa, 2, "first") == msa[:2] and esm_amd.subsample_indices is msa_select.subsample_indices
    with pytest.raises(ValueError, match="strategy"):
        msa_select.subsample_indices(msa, 4, "random")
    for bad in (0, -2, 2.5):
        with pytest.raises(ValueError, match="num_seqs"):
            msa_select.subsample_indices(msa, bad, "first")
    assert esm_amd.encode_msa is msa_select.encode_msa and esm_amd.msa_neff is msa_select.msa_neff


def test_encode_msa_on_the_host():
    msa = [("q", "MK-AY"), ("h", "MKTAY"), ("g", "-KTAW")]
    enc = msa_select.encode_msa(msa, device="cpu")
    assert enc.dtype == torch.uint8 and enc.tolist() == [list(s.encode()) for _, s in msa]
    with pytest.raises(ValueError, match="one length"):
        msa_select.encode_msa(msa + [("x", "MKTA")], device="cpu")
    with pytest.raises(ValueError, match="empty"):
        msa_select.encode_msa([], device="cpu")
    alphabet = esm_amd.Alphabet.from_architecture("msa_transformer")
    _, _, toks = alphabet.get_batch_converter()(msa)
    t = msa_select.encode_msa(toks, device="cpu")  # [1, R, C]: the <cls> column dropped
    assert t.dtype == torch.uint8 and tuple(t.shape) == (3, 5) and torch.equal(t.long(), toks[0, :, 1:])
    assert torch.equal(msa_select.encode_msa(toks[0], device="cpu"), t)
    # the same pairs of cells differ in both encodings
    assert torch.equal(enc[:, None, :] != enc[None, :, :], t[:, None, :] != t[None, :, :])
    raw = torch.randint(0, 256, (4, 7), dtype=torch.uint8)
    assert torch.equal(msa_select.encode_msa(raw, device="cpu"), raw)


def test_read_msa_reads_every_record_with_none(tmp_path):
    a3m = tmp_path / "p.a3m"
    a3m.write_text("#comment\n>q d\nMKTAY\n>h1\nMK-AYabc\n>h2\n-KTaAY\n>h3\nMKTAW\n")
    full = esm_amd.read_msa(a3m, None)
    assert full == [("q d", "MKTAY"), ("h1", "MK-AY"), ("h2", "-KTAY"), ("h3", "MKTAW")]
    assert esm_amd.read_msa(a3m) == full and esm_amd.read_msa(a3m, 2) == full[:2] and esm_amd.read_msa(a3m, 0) == []
    assert predict_msa.load_msa(a3m, None) == full


# ---- the command lines -----------------------------------------------------------------------------------------------------------
BASE = ["--model-location", "m", "--msa-path", "p.a3m", "--dms-input", "i", "--dms-output", "o"]


def test_predict_msa_subsample_flags():
    d = predict_msa.parse_args(BASE)
    assert (d.msa_subsample, d.msa_theta, d.msa_seed, d.msa_ensemble, d.msa_samples) == ("first", 0.2, 0, 1, 400)
    a = predict_msa.parse_args(BASE + ["--msa-subsample", "weighted", "--msa-theta", "0.3", "--msa-seed", "9", "--msa-ensemble", "5",
                                       "--msa-samples", "64"])
    assert (a.msa_subsample, a.msa_theta, a.msa_seed, a.msa_ensemble, a.msa_samples) == ("weighted", 0.3, 9, 5, 64)
    assert predict_msa.parse_args(BASE + ["--msa-subsample", "uniform", "--msa-ensemble", "2"]).msa_ensemble == 2
    assert predict_msa.parse_args(BASE + ["--msa-subsample", "greedy"]).msa_ensemble == 1
    for bad in (["--msa-ensemble", "2"], ["--msa-subsample", "first", "--msa-ensemble", "3"],
                ["--msa-subsample", "greedy", "--msa-ensemble", "2"], ["--msa-subsample", "weighted", "--msa-ensemble", "0"],
                ["--msa-subsample", "greedy-min"], ["--msa-subsample", "random"]):
        with pytest.raises(SystemExit):
            predict_msa.parse_args(BASE + bad)


def test_predict_msa_main_refuses_an_ensemble_of_first_rows_before_reading_anything(tmp_path):
    with pytest.raises(SystemExit):  # neither the a3m file nor the table exists: the refusal comes first
        predict_msa.main(["--model-location", "m", "--msa-path", str(tmp_path / "none.a3m"), "--dms-input",
                          str(tmp_path / "none.csv"), "--dms-output", str(tmp_path / "o.csv"), "--msa-ensemble", "2"])


def test_subsample_msa_parser():
    import importlib

    cli = importlib.import_module("esm_amd.subsample_msa")
    a = cli.parse_args(["--msa-path", "in.a3m", "--num-seqs", "128", "--output", "out.a3m"])
    assert (a.strategy, a.theta, a.seed, a.subsample, a.num_seqs, a.weights_out) == ("greedy", 0.2, 0, 0, 128, None)
    assert str(a.msa_path) == "in.a3m" and str(a.output) == "out.a3m"
    a = cli.parse_args(["--msa-path", "in.a3m", "--num-seqs", "8", "--output", "o", "--strategy", "weighted", "--theta", "0.1",
                        "--seed", "4", "--weights-out", "w.npy"])
    assert (a.strategy, a.theta, a.seed, str(a.weights_out)) == ("weighted", 0.1, 4, "w.npy")
    for bad in (["--num-seqs", "0"], ["--num-seqs", "8", "--strategy", "best"], ["--num-seqs", "8", "--seed", "-1"], []):
        with pytest.raises(SystemExit):
            cli.parse_args(["--msa-path", "in.a3m", "--output", "o"] + bad)
    # the package attribute names the function and the command-line module at once: both answer a call
    msa = M.records(M.family_msa(6, 8, 1))
    assert esm_amd.subsample_msa(msa, 2, "first") == msa[:2] and cli(msa, 3, "first") == msa[:3]


# ---- the emitted code of the hot kernel ---------------------------------------------------------------------------------------
def test_neighbour_count_kernel_needs_no_scratch(tmp_path):
    """Both instantiations of neighbor_counts_kernel (dword rows, byte rows) keep their 16 pair counts and their operands in
    registers: no scratch, and few enough VGPRs for four waves per SIMD (hipcc cross-compiles gfx950 without a GPU)."""
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import isa_report

    path = str(tmp_path / "msa_select.s")
    isa_report.compile_asm(os.path.join(root, "esm_amd", "csrc"), "msa_select.hip", path)
    meta = isa_report.meta(path)
    hot = [k for k in meta if "neighbor_counts_kernel" in k]
    assert len(hot) == 2, hot
    for k in hot:
        vgpr, _, scratch = meta[k]
        assert scratch == 0 and vgpr <= 128, (k, vgpr, scratch)
    assert all(scratch == 0 for _, _, scratch in meta.values()), meta  # nor does any other kernel of the file
