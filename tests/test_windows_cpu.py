"""The host side of windowed scoring and embedding (esm_amd/windows.py) without a GPU: the planning functions against the
brute-force restatement of the definitions (tests/_windows_ref.py) and as properties of their own, ``resolve_window``, the
argument parsing of the three command lines, and the argument checks of the three new C entries (fake pointers: every check
fails before the library touches the HIP runtime)."""
import argparse
import ctypes

import pytest

import _windows_ref as ref
import esm
from esm_amd import _native as N
from esm_amd import windows as W

FAKE = ctypes.c_void_p(0x1000)
WINDOWS = (5, 8, 33)
ENDS = ((1, 1), (1, 0), (0, 0))  # ESM-1b / ESM-2 alphabets, the ESM-1 alphabet, no special tokens


def lengths(window):
    return (window + 1, window + 2, 2 * window - 1, 3 * window + 5)


def cases():
    for window in WINDOWS:
        for n in lengths(window):
            yield n, window, False, 0, 0  # a raw slice has no special tokens of its own
            for h, t in ENDS:
                yield n, window, True, h, t


def strides(R):
    return sorted({1, max(1, R // 2), R})


def err():
    return N.lib.esmk_last_error().decode()


def test_geometry_and_starts():
    for n, window, wrap, h, t in cases():
        R, lo, hi = W.geometry(n, window, wrap, h, t)
        assert (R, lo, hi) == ref.geometry(n, window, wrap, h, t)
        assert R >= 1 and hi - lo > R  # n > window: every copy is exactly `window` columns wide
        for p in range(lo, hi):
            s = W.optimal_start(p, R, lo, hi)
            assert s == ref.start_of(p, R, lo, hi)
            assert lo <= s <= hi - R and s <= p < s + R


def test_grid_covers_the_body_range_and_owners_follow_the_rule():
    for n, window, wrap, h, t in cases():
        R, lo, hi = W.geometry(n, window, wrap, h, t)
        for stride in strides(R) + [None]:
            starts = W.grid_starts(R, lo, hi, stride)
            assert starts == ref.grid(R, lo, hi, stride)
            assert starts == sorted(set(starts)) and starts[0] == lo and starts[-1] == hi - R
            assert all(lo <= s <= hi - R for s in starts)
            assert all(b - a <= R for a, b in zip(starts, starts[1:]))  # no gap between neighbouring windows
            own = W.owners(starts, R, lo, hi)
            assert own == [ref.owner_of(p, starts, R) for p in range(lo, hi)]
            lists = W.blend_lists(starts, R, lo, hi)
            for p, w, lst in zip(range(lo, hi), own, lists):
                assert starts[w] <= p < starts[w] + R
                assert [k for k, _, _ in lst] == [k for k, s in enumerate(starts) if s <= p < s + R]
                assert all(j == p - starts[k] and wt == ref.weight(j, R) and wt >= 1 for k, j, wt in lst)
                assert w in [k for k, _, _ in lst]
    for bad in (0, -1, 9):
        with pytest.raises(ValueError, match="stride"):
            W.grid_starts(8, 0, 40, bad)


def test_owner_ties_go_to_the_lower_start():
    # R = 4, stride 1: position p is equally central in the windows at p - 2 (column 2) and p - 1 (column 1): |2 c - 3| = 1
    R, lo, hi = 4, 0, 12
    starts = W.grid_starts(R, lo, hi, 1)
    own = W.owners(starts, R, lo, hi)
    for p in range(2, hi - 2):
        keys = sorted((abs(2 * (p - s) - (R - 1)), s) for s in starts if s <= p < s + R)
        assert keys[0][0] == keys[1][0] == 1 and keys[0][1] == p - 2  # an exact tie
        assert starts[own[p]] == p - 2
    # pairs: i + j = 2 s + R - 1 +- 1 for two neighbouring starts
    assert W.pair_owner(starts, R, 4, 5) == starts.index(3)  # keys: s = 3 -> 0
    assert W.pair_owner(starts, R, 4, 4) == starts.index(2)  # s = 2 and s = 3 both give 1: the lower start
    assert W.pair_owner(starts, R, 0, 4) is None


def test_pair_owner_is_symmetric_and_follows_the_rule():
    for n, window, wrap, h, t in cases():
        R, lo, hi = W.geometry(n, window, wrap, h, t)
        for stride in strides(R):
            starts = W.grid_starts(R, lo, hi, stride)
            for i in range(lo, hi):
                for j in range(i, hi):
                    w = W.pair_owner(starts, R, i, j)
                    assert w == W.pair_owner(starts, R, j, i) == ref.pair_owner_of(i, j, starts, R)
                    assert (w is None) == (not any(s <= i and j < s + R for s in starts))


def test_set_rule_raises_exactly_when_the_set_spans_a_window():
    for n, window, wrap, h, t in cases():
        R, lo, hi = W.geometry(n, window, wrap, h, t)
        for a in range(lo, hi):
            for span in (0, 1, R - 2, R - 1, R, R + 3):
                b = a + span
                if span < 0 or b >= hi:
                    continue
                if span >= R:
                    with pytest.raises(ValueError, match="does not fit"):
                        W.set_start([a, b], R, lo, hi)
                    with pytest.raises(ValueError):
                        ref.start_of_set([a, b], R, lo, hi)
                    continue
                s = W.set_start([b, a], R, lo, hi)
                assert s == ref.start_of_set([a, b], R, lo, hi)
                assert lo <= s <= hi - R and s <= a and b < s + R
                if span == 0:
                    assert s == W.optimal_start(a, R, lo, hi)
    with pytest.raises(ValueError, match=r"set 7 \[3, 30\]"):
        W.set_start([3, 30], 8, 1, 60, name="7 [3, 30]")


def test_a_sequence_that_fits_plans_nothing():
    for window in WINDOWS:
        for n in (1, window - 1, window):
            for wrap in (True, False):
                assert W.plan_sequence(n, window, wrap, 1, 1) is None
        R, lo, hi, starts = W.plan_sequence(window + 1, window, False, 1, 1)
        assert (R, lo, hi, starts) == (window, 0, window + 1, [0, 1])


def esm1b(max_positions=40):
    args = argparse.Namespace(arch="roberta_large", layers=1, embed_dim=64, ffn_embed_dim=128, attention_heads=1,
                              max_positions=max_positions, token_dropout=True, emb_layer_norm_before=True)
    return esm.ProteinBertModel(args, esm.Alphabet.from_architecture("roberta_large"))


def test_resolve_window():
    esm2 = esm.ESM2(1, 64, 1)
    assert W.resolve_window(esm2, None) is None
    assert W.resolve_window(esm2, 32) == 32 and W.resolve_window(esm2, 3) == 3 and W.resolve_window(esm2, 5000) == 5000
    with pytest.raises(ValueError, match="int"):
        W.resolve_window(esm2, "max")
    for bad in (2, 0, -4):
        with pytest.raises(ValueError, match="below 3"):
            W.resolve_window(esm2, bad)
    for bad in ("32", "all", 7.5, True):
        with pytest.raises(ValueError, match="'max'"):
            W.resolve_window(esm2, bad)
    b = esm1b()
    assert W.resolve_window(b, "max") == 40 and W.resolve_window(b, 40) == 40 and W.resolve_window(b, 17) == 17
    with pytest.raises(ValueError, match="above maximum"):
        W.resolve_window(b, 41)
    from esm_amd.synth import esm1_args

    esm1 = esm.ProteinBertModel(esm1_args(1, 64, 1), esm.Alphabet.from_architecture("protein_bert_base"))
    assert W.resolve_window(esm1, 2) == 2  # <cls> and one residue: this alphabet appends no <eos>
    with pytest.raises(ValueError, match="int"):
        W.resolve_window(esm1, "max")  # sinusoidal positions: no table to take the size of
    msa_args = argparse.Namespace(layers=1, embed_dim=64, ffn_embed_dim=128, attention_heads=1, dropout=0.1, attention_dropout=0.1,
                                  activation_dropout=0.1, max_positions=1024, embed_positions_msa=True, embed_positions_msa_dim=64,
                                  max_tokens_per_msa=2 ** 14)
    msa = esm.MSATransformer(msa_args, esm.Alphabet.from_architecture("msa_transformer"))
    with pytest.raises(NotImplementedError):
        W.resolve_window(msa, 32)
    with pytest.raises(NotImplementedError):
        msa.forward_windows(None, window=32)
    with pytest.raises(NotImplementedError):
        msa.masked_marginals(None, window=32)


def test_command_line_parsing():
    from esm_amd import extract, predict, score_sequences

    base = ["--model-location", "m", "--sequence", "MKT", "--dms-input", "in.csv", "--dms-output", "out.csv"]
    a = predict.create_parser().parse_args(base)
    assert a.window is None and a.no_wrap is False
    a = predict.create_parser().parse_args(base + ["--window", "max", "--no-wrap"])
    assert a.window == "max" and a.no_wrap is True
    assert predict.create_parser().parse_args(base + ["--window", "1024"]).window == 1024
    base = ["--model-location", "m", "--fasta", "f.fasta", "--output", "o.csv"]
    a = score_sequences.create_parser().parse_args(base)
    assert a.window is None and a.no_wrap is False
    a = score_sequences.create_parser().parse_args(base + ["--window", "32", "--no-wrap"])
    assert a.window == 32 and a.no_wrap is True
    assert score_sequences.create_parser().parse_args(base + ["--window", "max"]).window == "max"
    base = ["m.pt", "f.fasta", "out", "--include", "mean"]
    a = extract.create_parser().parse_args(base)
    assert (a.window, a.window_stride, a.window_stitch, a.truncation_seq_length) == (None, None, "owner", None)
    a = extract.create_parser().parse_args(base + ["--window", "max", "--window-stride", "100", "--window-stitch", "blend"])
    assert (a.window, a.window_stride, a.window_stitch, a.truncation_seq_length) == ("max", 100, "blend", None)
    a = extract.create_parser().parse_args(base + ["--window", "512", "--truncation_seq_length", "2000"])
    assert (a.window, a.truncation_seq_length) == (512, 2000)
    for parser, head in ((predict.create_parser(), ["--model-location", "m", "--sequence", "M", "--dms-input", "i", "--dms-output", "o"]),
                         (extract.create_parser(), base)):
        for bad in ("0", "-3", "most", "1.5"):
            with pytest.raises(SystemExit):
                parser.parse_args(head + ["--window", bad])
    with pytest.raises(SystemExit):
        extract.create_parser().parse_args(base + ["--window", "32", "--window-stitch", "mean"])


def test_window_rows_argument_checks():
    def call(tok=FAKE, src=FAKE, start=FAKE, off=FAKE, pos=FAKE, out=FAKE, B=2, T=97, n=5, Tw=32, total=5):
        return N.lib.esmk_op_window_rows(tok, src, start, off, pos, out, B, T, n, Tw, total, 0, 2, 32, None)

    who = "esmk_op_window_rows"
    for kw in (dict(tok=None), dict(src=None), dict(start=None), dict(off=None), dict(pos=None), dict(out=None)):
        assert call(**kw) != 0 and who + ": null argument" in err(), kw
    for kw in (dict(B=0), dict(T=0), dict(n=0), dict(Tw=0), dict(n=-1), dict(Tw=-8)):
        assert call(**kw) != 0 and who in err() and "positive" in err(), kw
    assert call(total=-1) != 0 and who + ": total" in err()
    assert call(B=1 << 14, T=1 << 11) != 0 and who in err() and "2^24" in err()
    assert call(n=1 << 14, Tw=1 << 11) != 0 and who in err() and "2^24" in err()


def test_blend_rows_argument_checks():
    def call(x=FAKE, off=FAKE, src=FAKE, w=FAKE, out=FAKE, dt=N.F32, Nr=64, E=128, n_out=9, total=20):
        return N.lib.esmk_op_blend_rows(x, dt, off, src, w, out, Nr, E, n_out, total, None)

    who = "esmk_op_blend_rows"
    for kw in (dict(x=None), dict(off=None), dict(src=None), dict(w=None), dict(out=None)):
        assert call(**kw) != 0 and who + ": null argument" in err(), kw
    for kw in (dict(Nr=0), dict(n_out=0), dict(Nr=-2)):
        assert call(**kw) != 0 and who in err() and "positive" in err(), kw
    for E in (0, -4, 2, 130):
        assert call(E=E) != 0 and who + ": E must be a positive multiple of 4" in err(), E
    assert call(total=-1) != 0 and who + ": total" in err()
    assert call(dt=9) != 0 and who + ": x_dtype" in err()


def test_stitch_contacts_argument_checks():
    def call(maps=FAKE, start=FAKE, out=FAKE, n_w=3, R=6, Lb=20, body_lo=1):
        return N.lib.esmk_op_stitch_contacts(maps, start, out, n_w, R, Lb, body_lo, None)

    who = "esmk_op_stitch_contacts"
    for kw in (dict(maps=None), dict(start=None), dict(out=None)):
        assert call(**kw) != 0 and who + ": null argument" in err(), kw
    for kw in (dict(n_w=0), dict(R=0), dict(Lb=0), dict(Lb=-5)):
        assert call(**kw) != 0 and who in err() and "positive" in err(), kw
