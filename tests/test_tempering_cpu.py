"""The host side of the n-gram term and of replica exchange without a GPU: the numpy references of tests/_tempering_ref.py on
hand-worked cases, ``esm_amd.ngram.Background`` against the Counter restatement (floor, unseen keys, the npz round trip, the
command line that writes one), the argument errors of ``design`` and of ``python -m esm_amd.design``, the argument checks of the
three C entries (refused before any HIP call, on fake pointers as in tests/test_design_cpu.py), and the seeds of the GPU tests:
none of their decisions is undecided in the reference alone."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _design_ref as R
import _tempering_ref as TR
import esm
from esm_amd import _native as N
from esm_amd import ngram_table
from esm_amd.ngram import Background

D = __import__("importlib").import_module("esm_amd.design")
FAKE = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused first
A = 20


def err():
    return N.lib.esmk_last_error().decode()


# ---- the references on hand-worked cases --------------------------------------------------------------------------------------
def test_reference_ngram_on_worked_sequences():
    uniform = TR.uniform_tables(A, (1, 2, 3, 4))
    # "AAAA": one distinct n-gram per order, p = 1: KL_n = log(20^n)
    for n in (1, 2, 3, 4):
        e, bound = TR.ngram_energy(TR.encode("AAAA"), {n: uniform[n]}, A)
        assert abs(e - n * math.log(20.0)) < 1e-14 and 0 < bound < 1e-14
    e, _ = TR.ngram_energy(TR.encode("AAAA"), uniform, A)
    assert abs(e - 10 * math.log(20.0)) < 1e-13
    assert TR.ngram_energy(TR.encode("AAA"), {4: uniform[4]}, A) == (0.0, 0.0)  # S < n: no window
    # all windows distinct: "ACDE" has 4 monograms of p = 1/4, 3 bigrams of p = 1/3
    e, _ = TR.ngram_energy(TR.encode("ACDE"), {1: uniform[1]}, A)
    assert abs(e - math.log(20.0 / 4.0)) < 1e-15
    e, _ = TR.ngram_energy(TR.encode("ACDE"), {2: uniform[2]}, A)
    assert abs(e - math.log(400.0 / 3.0)) < 1e-15
    # p == q: "AC" against a background of A and C at one half each is 0 exactly
    half = np.full(A, 1e-5)
    half[[0, 1]] = 0.5
    assert TR.ngram_energy(TR.encode("AC"), {1: half}, A) == (0.0, 0.0)
    # a window holding X is left out: "AXC" has the monograms A and C, and no bigram at all
    assert TR.encode("AXC") == [0, -1, 1]
    assert TR.ngram_energy(TR.encode("AXC"), {1: half}, A) == (0.0, 0.0)
    assert TR.ngram_energy(TR.encode("AXC"), {2: uniform[2]}, A) == (0.0, 0.0)
    assert TR.ngram_counts(TR.encode("AXCC"), 2) == {(1, 1): 1}
    e, _ = TR.ngram_energy(TR.encode("XAAX"), {1: uniform[1], 2: uniform[2], 3: uniform[3]}, A)
    assert abs(e - 3 * math.log(20.0)) < 1e-14  # A twice, AA once, no trigram
    # the key: the first residue is most significant
    assert TR.key_of((1, 2, 3), 20) == 1 * 400 + 2 * 20 + 3
    q2 = uniform[2].copy()
    q2[TR.key_of((0, 1), A)] = 0.25  # "AC"
    e, _ = TR.ngram_energy(TR.encode("AC"), {2: q2}, A)
    assert e == math.log(4.0)
    e, _ = TR.ngram_energy(TR.encode("CA"), {2: q2}, A)
    assert abs(e - math.log(400.0)) < 1e-15


def test_reference_acceptance_with_rungs_and_a_third_term():
    assert TR.combine_ex(1.0, 2.0, 1.0, -30.0, 10) == R.combine(1.0, 2.0, 1.0, -30.0, 10)[0] == 5.0
    assert TR.combine_ex(1.0, 2.0, 1.0, -30.0, 10, 0.5, 3.0) == 6.5 and TR.combine_ex(1.0, 2.0, 1.0, -30.0, 10, 0.0, 3.0) == 5.0
    case = TR.accept_ex_case(n=12)
    one = dict(case, rung=np.zeros(12, dtype=np.int32), e_extra=np.zeros(12))
    plain = R.accept_reference(dict(case, e_cur=case["e_cur"]), 1.0, 1.0, 0.5, 0)
    ex = TR.accept_ex(one, 1.0, 1.0, 0.0, [2.0], 0)
    assert all(np.array_equal(a, b) for a, b in zip(plain, ex))
    # a chain at a hot rung accepts what the same chain at a cold rung rejects
    up = dict(R.accept_case(n=3), rung=np.array([0, 1, 1], dtype=np.int32), e_extra=np.zeros(3))
    up["e_cur"] = up["e_cur"] - 50.0  # every proposal climbs by about 50
    up["tok"][:] = 5
    _, _, acc, _ = TR.accept_ex(up, 1.0, 1.0, 0.0, [1.0, 1e-9], 0)
    assert acc.tolist() == [False, True, True]


def test_reference_swap_round():
    # two chains, rungs (0, 1): the cold rung holds the higher energy, so a = (1 - 0.5) * (3 - 1) > 0: always swapped
    rung, acc, u, und = TR.swap_round([0, 1], [3.0, 1.0], [1.0, 0.5], [7], 1, 0)
    assert rung.tolist() == [1, 0] and acc.tolist() == [1, 1] and u[0] == u[1] == TR.swap_uniform(1, 7, 0, 0) and not und.any()
    # the other way round: a = 0.5 * (1 - 3) = -1: swapped iff u < exp(-1)
    rung, acc, u, _ = TR.swap_round([0, 1], [1.0, 3.0], [1.0, 0.5], [7], 1, 0)
    assert acc.tolist() == [int(u[0] < math.exp(-1.0))] * 2 and rung.tolist() == ([1, 0] if acc[0] else [0, 1])
    # an odd round pairs rungs (1, 2): with K = 2 there is none, with K = 3 rung 0 is left alone; an even round leaves rung 2 alone
    rung, acc, u, _ = TR.swap_round([0, 1], [3.0, 1.0], [1.0, 0.5], [7], 1, 1)
    assert rung.tolist() == [0, 1] and acc.tolist() == [0, 0] and u.tolist() == [-1.0, -1.0]
    rung, acc, u, _ = TR.swap_round([2, 0, 1], [1.0, 9.0, 5.0], [1.0, 0.5, 0.25], [4], 1, 1)
    assert rung.tolist() == [1, 0, 2] and u[1] == -1.0 and u[0] == u[2] == TR.swap_uniform(1, 4, 1, 1)
    rung, acc, u, _ = TR.swap_round([2, 0, 1], [1.0, 9.0, 5.0], [1.0, 0.5, 0.25], [4], 1, 0)
    assert rung.tolist() == [2, 1, 0] and u[0] == -1.0 and acc.tolist() == [0, 1, 1]
    assert TR.swap_round([0], [1.0], [1.0], [4], 1, 0)[0].tolist() == [0]
    # a NaN rejects; the uniform is a 24-bit fraction and depends on every counter word
    assert TR.swap_round([0, 1], [float("nan"), 1.0], [1.0, 0.5], [7], 1, 0)[1].tolist() == [0, 0]
    us = {TR.swap_uniform(1, 7, 0, 0), TR.swap_uniform(2, 7, 0, 0), TR.swap_uniform(1, 8, 0, 0), TR.swap_uniform(1, 7, 1, 0),
          TR.swap_uniform(1, 7, 0, 1), R.accept_uniform(1, 7, 0)}
    assert len(us) == 6 and all(0 <= x < 1 and x * 2 ** 24 == int(x * 2 ** 24) for x in us)


def test_the_seeds_of_the_gpu_tests_leave_nothing_undecided():
    case = TR.accept_ex_case()
    inv_t = [1.0 / t for t in TR.EX_TEMPERATURES]
    e_prop, u, acc, und = TR.accept_ex(case, 1.0, 1.0, TR.EX_W_EXTRA, inv_t, 0)
    assert und.sum() == 0 and 0 < acc.sum() < acc.size and not acc[case["tok"] < 0].any()
    for k in range(3):
        assert 0 < acc[case["rung"] == k].sum()
    for K in TR.SWAP_KS:
        c = TR.swap_case(K)
        for rnd in (0, 1):
            rung, acc, u, und = TR.swap_round(c["rung"], c["e_cur"], c["inv_t"], c["ladder_ids"], TR.SWAP_SEED, rnd)
            assert und.sum() == 0
            if K >= 3 or (K == 2 and rnd == 0):
                attempted = u >= 0
                assert 0 < acc.sum() < attempted.sum(), (K, rnd)


# ---- Background ---------------------------------------------------------------------------------------------------------------
SEQS = ["MKTAYIAKQRQISFVKSHFSRQLEERLGLIEVQ", "ACDEFGHIKLMNPQRSTVWYAACC", "MKXTAYBZ", "AAAAAAAA", "", "K"]


def test_background_against_the_counter_restatement():
    bg = Background.from_sequences(SEQS, orders=(1, 2, 3, 4), floor=0.02)
    assert bg.orders == (1, 2, 3, 4) and bg.alphabet == TR.STANDARD
    for n in bg.orders:
        counts = sum((TR.ngram_counts(TR.encode(s), n) for s in SEQS), TR.Counter())
        total = sum(counts.values())
        want = np.full((A ** n,), 0.02)  # an unseen key reads as the floor
        for window, c in counts.items():
            want[TR.key_of(window, A)] = max(c / total, 0.02)  # ... and so does a rare one
        assert bg.tables[n].dtype == np.float64 and np.array_equal(bg.tables[n], want), n
        assert (bg.tables[n] == 0.02).any() and (bg.tables[n] > 0.02).any()
    # windows over X, B, Z are not counted: "MKXTAYBZ" gives the bigrams MK, TA, AY only
    only = Background.from_sequences(["MKXTAYBZ"], orders=(2,), floor=1e-5)
    seen = np.nonzero(only.tables[2] > 1e-5)[0].tolist()
    assert seen == sorted(TR.key_of(tuple(TR.encode(w)), A) for w in ("MK", "TA", "AY")) and only.tables[2][seen[0]] == 1.0 / 3.0
    assert Background.from_sequences(SEQS).orders == (1, 2, 3)
    empty = Background.from_sequences(["XX"], orders=(1,))
    assert (empty.tables[1] == 1e-5).all()
    model = esm.ESM2(1, 128, 2)
    code = bg.token_codes(model.alphabet)
    assert code.dtype == np.int32 and code.shape == (model.alphabet_size,)
    for i, tok in enumerate(model.alphabet.all_toks):
        assert code[i] == (TR.STANDARD.index(tok) if tok in TR.STANDARD and len(tok) == 1 else -1)
    for bad in (dict(orders=()), dict(orders=(5,)), dict(orders=(0, 1)), dict(floor=0.0), dict(floor=float("nan")), dict(alphabet="AA")):
        with pytest.raises(ValueError):
            Background.from_sequences(SEQS, **bad)
    with pytest.raises(ValueError, match="finite and positive"):
        Background("AC", {1: np.array([1.0, 0.0])})
    with pytest.raises(ValueError, match="entries"):
        Background("AC", {2: np.ones(3)})


def test_background_npz_round_trip_and_the_table_command(tmp_path):
    bg = Background.from_sequences(SEQS, orders=(1, 3), alphabet="ACDEKLM", floor=1e-4)
    path = tmp_path / "bg.npz"
    bg.save(path)
    with np.load(path, allow_pickle=False) as z:  # plain arrays: nothing in the file needs pickle
        assert sorted(z.files) == ["alphabet", "orders", "q1", "q3"]
    back = Background.load(path)
    assert back.alphabet == "ACDEKLM" and back.orders == (1, 3)
    assert all(np.array_equal(back.tables[n].view(np.uint64), bg.tables[n].view(np.uint64)) for n in (1, 3))
    fasta = tmp_path / "s.fasta"
    fasta.write_text("".join(f">s{i} some text\n{s[:10].lower()}\n{s[10:]}\n" for i, s in enumerate(SEQS) if s))
    assert ngram_table.read_fasta(fasta) == [s for s in SEQS if s]
    out = tmp_path / "cli.npz"
    ngram_table.main(["--fasta", str(fasta), "--orders", "1", "2", "--floor", "1e-4", "--output", str(out)])
    cli, want = Background.load(out), Background.from_sequences(SEQS, orders=(1, 2), floor=1e-4)
    assert cli.orders == (1, 2) and all(np.array_equal(cli.tables[n], want.tables[n]) for n in (1, 2))
    for bad in (["--fasta", str(fasta)], ["--fasta", str(fasta), "--output", "o", "--orders", "5"],
                ["--fasta", str(fasta), "--output", "o", "--floor", "0"]):
        with pytest.raises(SystemExit):
            ngram_table.parse_args(bad)


# ---- argument errors of design and of the command line ------------------------------------------------------------------------
def test_design_refusals_before_a_device_is_asked_for():
    model = esm.ESM2(1, 128, 2)
    toks = torch.tensor([[0, 5, 6, 7, 8, 2], [0, 9, 10, 11, 12, 2], [0, 9, 10, 11, 12, 2], [0, 5, 5, 5, 5, 2]])
    target = np.zeros((4, 4), dtype=np.uint8)
    bg = Background.from_sequences(SEQS)
    with pytest.raises(ValueError, match="no multiple of replicas = 3"):
        model.design(toks, target, 3, replicas=3, temperature=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="positive and finite"):
        model.design(toks, target, 3, replicas=2, temperature=[1.0, 0.0])
    for t in ([1.0, float("inf")], [1.0, float("nan")], [1.0, -2.0], 1.0, [1.0, 2.0, 3.0], [[1.0, 2.0]] * 2):
        with pytest.raises(ValueError):
            model.design(toks, target, 3, replicas=2, temperature=t)
    for kw in (dict(replicas=1), dict(replicas=65), dict(replicas=2, temperature=[1.0, 2.0], swap_every=-1)):
        with pytest.raises(ValueError):
            model.design(toks, target, 3, **kw)
    with pytest.raises(ValueError, match="w_ngram != 0 needs ngram"):
        model.design(toks, target, 3, w_ngram=1.0)
    with pytest.raises(ValueError, match="w_ngram != 0 needs ngram"):
        model.design_energy(toks, target, w_ngram=0.5)
    with pytest.raises(ValueError, match="w_ngram must be finite"):
        model.design(toks, target, 3, w_ngram=float("inf"), ngram=bg)
    # what passes every host check reaches the device question
    for call in (lambda: model.design(toks, target, 3, replicas=2, temperature=[1.0, 2.0]),
                 lambda: model.design(toks, target, 3, replicas=4, temperature=[[1.0, 2.0, 3.0, 4.0]] * 3, swap_every=0),
                 lambda: model.design(toks, target, 3, w_ngram=1.0, ngram=bg), lambda: model.design_energy(toks, target, w_ngram=1.0, ngram=bg),
                 lambda: D.design(model, toks, None, 3, w_contact=0, w_ngram=2.0, ngram=bg, replicas=2, temperature=[1.0, 2.0])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    lad = D.ladder_inverse_temperatures([1.0, 4.0], 3, 2)
    assert lad.shape == (3, 2) and lad.dtype == np.float64 and lad.tolist() == [[1.0, 0.25]] * 3
    assert D.ladder_inverse_temperatures([[1.0, 4.0], [2.0, 8.0]], 2, 2).tolist() == [[1.0, 0.25], [0.5, 0.125]]


def test_cli_parsing_of_the_new_switches(tmp_path):
    base = ["--model-location", "m.pt", "--output", "o.fasta", "--no-target", "--length", "9"]
    a = D.parse_args(base)
    assert (a.replicas, a.ladder, a.swap_every, a.w_ngram, a.ngram_table) == (None, None, 1, 0.0, None)
    a = D.parse_args(base + ["--replicas", "4", "--ladder", "1:8", "--num-chains", "8", "--swap-every", "5", "--w-ngram", "0.5",
                             "--ngram-table", "bg.npz"])
    assert (a.replicas, a.ladder, a.swap_every, a.w_ngram, a.ngram_table) == (4, (1.0, 8.0), 5, 0.5, "bg.npz")
    ladder = D.anneal_ladder(*a.ladder, a.replicas)
    assert ladder[0] == 1.0 and abs(ladder[-1] - 8.0) < 1e-14 and abs(ladder[1] - 2.0) < 1e-14
    for bad in (["--replicas", "2", "--ladder", "1:4", "--num-chains", "3"], ["--replicas", "2", "--num-chains", "2"],
                ["--ladder", "1:4"], ["--replicas", "2", "--ladder", "1:4", "--temperature", "1", "--num-chains", "2"],
                ["--replicas", "2", "--ladder", "1:4", "--anneal", "1:2", "--num-chains", "2"],
                ["--replicas", "2", "--ladder", "1:0", "--num-chains", "2"], ["--replicas", "1", "--ladder", "1:4"],
                ["--w-ngram", "1"], ["--swap-every", "-1"]):
        with pytest.raises(SystemExit):
            D.parse_args(base + bad)
    # the files: without replicas the bytes of before; with them |rung=<r> and the new columns
    out = tmp_path / "o.fasta"
    D.write_fasta(out, "design", [0, 1], ["MA", "MC"], [1.25, 0.5], seed=5)
    assert out.read_text() == ">design|chain=0|seed=5|energy=1.250000\nMA\n>design|chain=1|seed=5|energy=0.500000\nMC\n"
    D.write_fasta(out, "design", [0, 1], ["MA", "MC"], [1.25, 0.5], seed=5, rungs=[1, 0])
    assert out.read_text() == ">design|chain=0|seed=5|energy=1.250000|rung=1\nMA\n>design|chain=1|seed=5|energy=0.500000|rung=0\nMC\n"
    assert D.TRAJECTORY_FIELDS == ("site", "old", "new", "e_cur", "e_prop", "e_contact", "e_lm", "hastings", "u", "accepted")
    fields = D.TRAJECTORY_FIELDS + D.NGRAM_FIELDS + D.REPLICA_FIELDS
    traj = {k: torch.zeros((2, 2), dtype=torch.float64) for k in reversed(fields)}
    D.write_log(tmp_path / "l.csv", traj, [4, 5])
    rows = (tmp_path / "l.csv").read_text().splitlines()
    assert rows[0] == "step,chain," + ",".join(fields) and rows[0].endswith("accepted,e_ngram,rung,swapped,swap_u") and len(rows) == 5


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_tempering_op_argument_checks():
    lib = N.lib

    def g(tokens=FAKE, code=FAKE, q1=FAKE, q2=None, q3=None, q4=None, mask=1, out=FAKE, B=2, T=70, first=1, S=68, V=33, A=20):
        return lib.esmk_op_ngram_energy(tokens, code, q1, q2, q3, q4, mask, out, B, T, first, S, V, A, None)

    for kw in (dict(tokens=None), dict(code=None), dict(out=None)):
        assert g(**kw) != 0 and err() == "esmk_op_ngram_energy: null argument", kw
    for kw in (dict(B=0), dict(T=0)):
        assert g(**kw) != 0 and "B and T must be positive" in err(), kw
    assert g(B=1 << 12, T=1 << 13, S=5) != 0 and "2^24" in err()
    assert g(S=0) != 0 and "S must be positive" in err()
    assert g(T=40000, S=32769) != 0 and "S above 32768" in err()
    for kw in (dict(first=-1), dict(first=3), dict(first=0, S=71)):
        assert g(**kw) != 0 and "must lie in [0, T)" in err(), kw
    for kw in (dict(V=0), dict(V=65)):
        assert g(**kw) != 0 and "V must be in 1 .. 64" in err(), kw
    for kw in (dict(A=0), dict(A=33)):
        assert g(**kw) != 0 and "A must be in 1 .. 32" in err(), kw
    for mask in (0, 16, 17, -1):
        assert g(mask=mask) != 0 and "order_mask must choose" in err(), mask
    assert g(q1=None) != 0 and "order 1 is chosen but its table is null" in err()
    assert g(mask=0b1001) != 0 and "order 4 is chosen but its table is null" in err()
    assert g(mask=0b0110, q2=FAKE) != 0 and "order 3 is chosen but its table is null" in err()

    def a(tokens=FAKE, slot=None, site=FAKE, tok=FAKE, cid=FAKE, ec=FAKE, lp=FAKE, n_res=FAKE, h=None, ex=None, wc=1.0, wl=1.0, wx=0.0,
          inv_t=FAKE, rung=None, n_rung=1, seed=1, step=0, e_cur=FAKE, ecc=None, elc=None, exc=None, acc=FAKE, u=None, ep=None, n=4,
          B=4, T=70):
        return lib.esmk_op_mh_accept_ex(tokens, slot, site, tok, cid, ec, lp, n_res, h, ex, wc, wl, wx, inv_t, rung, n_rung, seed,
                                        step, e_cur, ecc, elc, exc, acc, u, ep, n, B, T, None)

    for kw in (dict(tokens=None), dict(site=None), dict(tok=None), dict(cid=None), dict(e_cur=None), dict(acc=None), dict(inv_t=None)):
        assert a(**kw) != 0 and err() == "esmk_op_mh_accept_ex: null argument", kw
    assert a(n_res=None) != 0 and "lp_sum without n_res" in err()
    for kw in (dict(n=0), dict(B=0), dict(T=-1)):
        assert a(**kw) != 0 and "n_chain, B and T must be positive" in err(), kw
    assert a(B=1 << 12, T=1 << 13) != 0 and "2^24" in err()
    assert a(n_rung=0) != 0 and "n_rung must be in 1 .. 2^24" in err()
    for kw in (dict(wc=float("inf")), dict(wl=float("nan")), dict(wx=float("-inf"))):
        assert a(**kw) != 0 and "weights must be finite" in err(), kw
    assert a(step=-1) != 0 and "step must not be negative" in err()

    def s(rung=FAKE, e_cur=FAKE, inv_t=FAKE, host=(1.0, 0.5), lid=FAKE, seed=1, rnd=0, acc=FAKE, u=FAKE, n_ladder=3, K=2):
        h = None if host is None else (ctypes.c_double * len(host))(*host)
        return lib.esmk_op_replica_swap(rung, e_cur, inv_t, h, lid, seed, rnd, acc, u, n_ladder, K, None)

    for kw in (dict(rung=None), dict(e_cur=None), dict(inv_t=None), dict(host=None), dict(lid=None), dict(acc=None), dict(u=None)):
        assert s(**kw) != 0 and err() == "esmk_op_replica_swap: null argument", kw
    for K in (0, -1, 65):
        assert s(K=K, host=(1.0,) * 65) != 0 and "K must be in 1 .. 64" in err(), K
    for n_ladder in (0, 1 << 24):
        assert s(n_ladder=n_ladder) != 0 and "n_ladder * K must be in 1 .. 2^24" in err()
    assert s(rnd=-1) != 0 and "round must not be negative" in err()
    for bad in (-1.0, float("nan"), float("inf")):
        assert s(host=(1.0, bad)) != 0 and "every inv_t must be finite and not negative" in err(), bad
