"""Multi-mutant variant scoring through the model (esm_amd/scoring.py: ``masked_joint``, ``score_variants``; the command line's
``--mutation-sep``): the joint-mask rows against this model's own ``forward`` at B = 1 on the masked sequence (bit for bit),
the scores against the fp64 sum of the fp32 terms read from those rows (exact), single mutants against ``score_mutations``
(exact).  The models and the B = 2, T = 70 batch (lengths 70 and 41) are those of tests/test_scoring_gpu.py: L = 2, E = 128,
ESM-2, ESM-1b and ESM-1, all with token dropout (whose divisor depends on each built sequence's own mask count)."""
import csv
import functools

import pytest
import torch

import esm
from _scoring_ref import check_rows
from esm_amd import ops, predict, scoring
from test_scoring_gpu import MODELS, PAD, L, batch

pytestmark = pytest.mark.gpu
ALPHABETS = {"esm2": "ESM-1b", "esm1b": "roberta_large", "esm1": "protein_bert_base"}


@functools.lru_cache(maxsize=None)
def case(kind):
    """(model, tokens [2, 70], alphabet, sequence): the sequence is the residues of row 0 of the batch as a string."""
    make, tok_kw = MODELS[kind]
    model = make()
    toks = batch(**tok_kw)
    alphabet = esm.Alphabet.from_architecture(ALPHABETS[kind])
    residues = toks[0, 1:-1] if alphabet.append_eos else toks[0, 1:]
    seq = "".join(alphabet.get_tok(int(t)) for t in residues)
    _, _, again = alphabet.get_batch_converter()([("protein1", seq)])
    assert torch.equal(again, toks[:1])  # the converter gives row 0 back
    assert bool(model.token_dropout)
    return model, toks.cuda(), alphabet, seq


def sub(seq, idx, mt):
    """The substitution of residue ``idx`` (0-based) by ``mt`` in 1-based numbering: 'K2G'."""
    assert seq[idx] != mt
    return f"{seq[idx]}{idx + 1}{mt}"


def other(seq, idx, k=0):
    """A residue letter that differs from seq[idx]."""
    return [c for c in "ACDEFGHIKLMNPQRSTVWY" if c != seq[idx]][k]


def same_pll(got, want, n_terms):
    """Two pseudo-log-likelihoods of the same fp32 terms: ``pseudo_log_likelihood`` adds them in fp64 through
    ``index_add_``, whose order on the device is not fixed.  Every term is a log-probability (<= 0), so a sum of n terms in
    any order is within (n - 1) 2^-53 |sum| of the exact one, and two orders within twice that of each other."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert abs(g - w) <= 2 * n_terms * 2.0 ** -53 * abs(w), (g, w)


SETS = [[5], [5, 6], [40, 1, 17], list(range(1, 40))]  # the last one: all 39 residues of sequence 1
SRC = [0, 0, 0, 1]


@pytest.mark.parametrize("kind", list(MODELS))
def test_masked_joint_rows_equal_forward_of_the_masked_sequence(kind):
    model, toks, _, _ = case(kind)
    offsets, pos, lp, logits = model.masked_joint(toks, SETS, src=SRC, chunk=3, return_logits=True)  # copies: 3 + 1
    V = model.alphabet_size
    assert offsets.tolist() == [0, 1, 3, 6, 45] and offsets.dtype == torch.int64 and not offsets.is_cuda
    assert pos.tolist() == [5, 5, 6, 1, 17, 40] + list(range(1, 40)) and pos.dtype == torch.int64 and pos.is_cuda
    assert lp.shape == (45, V) and lp.dtype == torch.float32 and logits.shape == (45, V) and logits.dtype == torch.float32
    with torch.no_grad():
        for s, (ps, b) in enumerate(zip(SETS, SRC)):
            masked = toks[b:b + 1].clone()
            masked[0, ps] = model.mask_idx
            want = model(masked)["logits"][0, sorted(ps)].float()
            assert torch.equal(logits[offsets[s]:offsets[s + 1]], want), f"{kind} set {s}: logits differ from forward's at B = 1"
    assert torch.equal(lp, ops.log_softmax_rows(logits.contiguous()))
    check_rows(lp, logits, f"masked_joint {kind}")
    # the joint mask is not the single mask: position 5 with 6 masked as well gives another row
    assert not torch.equal(logits[0], logits[1])
    # without the logits, with the default chunk (one call) and tokens from the host: the same log-probabilities
    off2, pos2, lp2 = model.masked_joint(toks.cpu(), SETS, src=SRC)
    assert torch.equal(off2, offsets) and torch.equal(pos2, pos) and torch.equal(lp2, lp)
    # a single-position set is the masked-marginal row
    one = model.masked_marginals(toks, positions=[[5], []])
    assert torch.equal(one[0, 5], lp[0])
    # src defaults to sequence 0 of a batch of one
    off1, _, lp1 = model.masked_joint(toks[:1], SETS[:3])
    assert off1.tolist() == [0, 1, 3, 6] and torch.equal(lp1, lp[:6])


def test_masked_joint_refusals():
    model, toks, _, _ = case("esm2")
    with pytest.raises(ValueError, match="empty"):
        model.masked_joint(toks, [[5], []], src=[0, 0])
    with pytest.raises(ValueError, match="outside"):
        model.masked_joint(toks, [[5, 70]], src=[0])
    with pytest.raises(ValueError, match="outside"):
        model.masked_joint(toks, [[-1]], src=[0])
    with pytest.raises(ValueError, match="<pad>"):
        model.masked_joint(toks, [[5, 50]], src=[1])  # position 50 of sequence 1 is padding
    with pytest.raises(ValueError, match="src"):
        model.masked_joint(toks, [[5]])  # two sequences: which one?
    with pytest.raises(ValueError, match="outside"):
        model.masked_joint(toks, [[5]], src=[2])
    assert toks[1, 50].item() == PAD


@pytest.mark.parametrize("kind", list(MODELS))
def test_score_variants_masked_marginals(kind, monkeypatch):
    model, toks, alphabet, seq = case(kind)
    a = alphabet.get_idx
    singles = [sub(seq, 4, other(seq, 4)), sub(seq, 0, other(seq, 0)), sub(seq, len(seq) - 1, other(seq, len(seq) - 1))]
    table = model.masked_marginals(toks[:1])
    want_single = scoring.score_mutations(table.cpu(), seq, singles, alphabet, offset_idx=1)
    got_single = model.score_variants(alphabet, seq, singles, offset_idx=1)
    assert all(isinstance(s, float) for s in got_single) and got_single == want_single  # exactly: the same fp32 difference

    # a double mutant: residues 4 and 5 sit at token positions 5 and 6; its rows come from the forward with BOTH masked
    m0, m1 = other(seq, 4), other(seq, 5, 3)
    double = sub(seq, 4, m0) + ":" + sub(seq, 5, m1)
    _, pos, lp = model.masked_joint(toks[:1], [[5, 6]])
    assert pos.tolist() == [5, 6]
    lp = lp.cpu()
    t0, t1 = lp[0, a(m0)] - lp[0, a(seq[4])], lp[1, a(m1)] - lp[1, a(seq[5])]
    assert t0.dtype == torch.float32
    want_double = (t0.double() + t1.double()).item()
    # a triple, written in descending order: the terms are added in ascending order of position
    triple_parts = [sub(seq, 39, other(seq, 39)), sub(seq, 16, other(seq, 16, 5)), sub(seq, 0, other(seq, 0, 7))]
    _, _, lp3 = model.masked_joint(toks[:1], [[40, 17, 1]])
    lp3 = lp3.cpu()
    want_triple = 0.0
    for row, part in zip(lp3, reversed(triple_parts)):  # rows ascend: residues 0, 16, 39
        want_triple += float((row[a(part[-1])] - row[a(part[0])]).item())
    # the same double with other mutants, the double written the other way round, and a single at one of its positions
    double2 = sub(seq, 4, other(seq, 4, 9)) + ":" + sub(seq, 5, other(seq, 5, 11))
    flipped = ":".join(reversed(double.split(":")))
    variants = [double, singles[0], ":".join(triple_parts), double2, flipped, ":".join(reversed(triple_parts))]

    calls = []
    real_forward_rows = scoring.forward_rows

    def counting(model_, tokens, sel_rows, return_logits=False):
        calls.append((tokens.shape[0], sel_rows.numel()))
        return real_forward_rows(model_, tokens, sel_rows, return_logits=return_logits)

    monkeypatch.setattr(scoring, "forward_rows", counting)
    got = model.score_variants(alphabet, seq, variants, offset_idx=1)
    # three distinct position sets ({5,6}, {5}, {1,17,40}) in ONE forward of three masked copies and 2 + 1 + 3 selected rows
    assert calls == [(3, 6)]
    assert got[0] == want_double and got[4] == want_double
    assert got[1] == want_single[0]
    assert got[2] == want_triple and got[5] == want_triple
    assert got[3] != got[0]
    # the sum of two single-mask scores is another number: the joint mask is in use
    assert got[0] != model.score_variants(alphabet, seq, [sub(seq, 4, m0)], offset_idx=1)[0] + \
        model.score_variants(alphabet, seq, [sub(seq, 5, m1)], offset_idx=1)[0]
    del calls[:]
    assert model.score_variants(alphabet, seq, variants, offset_idx=1, chunk=2) == got  # two calls: 2 copies + 1 copy
    assert calls == [(2, 3), (1, 3)]
    # a custom separator and 0-based numbering
    zero_based = f"{seq[4]}4{m0}+{seq[5]}5{m1}"
    assert model.score_variants(alphabet, seq, [zero_based], offset_idx=0, sep="+") == [want_double]
    assert model.score_variants(alphabet, seq, []) == []
    with pytest.raises(ValueError, match="wild type"):
        model.score_variants(alphabet, seq, [sub(seq, 4, m0) + ":" + other(seq, 5) + "6" + seq[5]], offset_idx=1)


@pytest.mark.parametrize("kind", list(MODELS))
def test_score_variants_wt_marginals_and_pseudo_ppl(kind):
    model, toks, alphabet, seq = case(kind)
    a = alphabet.get_idx
    m0, m1 = other(seq, 4), other(seq, 5, 3)
    single, double = sub(seq, 10, other(seq, 10)), sub(seq, 4, m0) + ":" + sub(seq, 5, m1)
    table = model.wt_marginals(toks[:1]).cpu()
    got = model.score_variants(alphabet, seq, [single, double], strategy="wt-marginals", offset_idx=1)
    assert got[0] == scoring.score_mutations(table, seq, single, alphabet, offset_idx=1)
    t0, t1 = table[0, 5, a(m0)] - table[0, 5, a(seq[4])], table[0, 6, a(m1)] - table[0, 6, a(seq[5])]
    assert got[1] == (t0.double() + t1.double()).item()
    # pseudo-ppl: the pseudo-log-likelihood of the mutated sequences over the reference's positions
    mutated = [("s", seq[:10] + single[-1] + seq[11:]), ("d", seq[:4] + m0 + m1 + seq[6:])]
    _, _, mtoks = alphabet.get_batch_converter()(mutated)
    want = model.pseudo_log_likelihood(mtoks, positions=range(1, len(seq) - 1)).tolist()
    assert all(w < 0 for w in want)
    same_pll(model.score_variants(alphabet, seq, [single, double], strategy="pseudo-ppl", offset_idx=1), want, len(seq) - 2)


def test_predict_cli_with_multi_mutant_rows(tmp_path, monkeypatch):
    """``python -m esm_amd.predict`` (called in process) on a table with ':'-joined rows: every strategy's column is what
    ``score_variants`` gives; a table of single substitutions is written exactly as it was before variants were scored."""
    from esm_amd.synth import write_esm2_checkpoint

    path = write_esm2_checkpoint(str(tmp_path), "esm2_t2_synth", L, 128, 2, seed=3)
    seq = "MKTAYIAKQRQISFVKSHFSRQLEERLGLI"
    muts = ["K26G", "T27C:I54A", "I54A", "M25W:K26G:Y29F"]  # offset 25
    src = tmp_path / "scan.csv"
    src.write_text("mutant,fitness\n" + "".join(f"{m},0\n" for m in muts))
    model, alphabet = esm.pretrained.load_model_and_alphabet(path)
    model = model.eval().cuda()
    for strategy in predict.STRATEGIES:
        want = model.score_variants(alphabet, seq, muts, strategy=strategy, offset_idx=25)
        out = tmp_path / f"{strategy}.csv"
        assert predict.main(["--model-location", path, "--sequence", seq, "--dms-input", str(src), "--dms-output", str(out),
                             "--offset-idx", "25", "--scoring-strategy", strategy]) == 0
        rows = list(csv.DictReader(open(out, newline="")))
        assert [r["mutant"] for r in rows] == muts
        if strategy == "pseudo-ppl":
            same_pll([float(r[path]) for r in rows], want, len(seq) - 2)
        else:
            assert [float(r[path]) for r in rows] == want, strategy
    # another separator: ':' is then no separator, and the rows above are refused as malformed
    other_sep = tmp_path / "semicolon.csv"
    other_sep.write_text("mutant\nT27C;I54A\n")
    out = tmp_path / "semicolon_scored.csv"
    assert predict.main(["--model-location", path, "--sequence", seq, "--dms-input", str(other_sep), "--dms-output", str(out),
                         "--offset-idx", "25", "--scoring-strategy", "masked-marginals", "--mutation-sep", ";"]) == 0
    assert float(list(csv.DictReader(open(out, newline="")))[0][path]) == \
        model.score_variants(alphabet, seq, ["T27C:I54A"], offset_idx=25)[0]
    with pytest.raises(ValueError, match="form"):
        predict.score_table(model, alphabet, seq, muts, "masked-marginals", 25, sep=";")

    # single substitutions only: the path of before (score_variants is not entered), the file of before, byte for byte
    singles = ["K26G", "T27C", "I54A"]
    src1 = tmp_path / "singles.csv"
    src1.write_text("mutant,fitness\n" + "".join(f"{m},0.5\n" for m in singles))
    _, _, toks = alphabet.get_batch_converter()([("protein1", seq)])
    want = {"wt-marginals": scoring.score_mutations(model.wt_marginals(toks).cpu(), seq, singles, alphabet, 25),
            "masked-marginals": scoring.score_mutations(model.masked_marginals(toks).cpu(), seq, singles, alphabet, 25)}
    mutated = [(m, seq[:i] + m[-1] + seq[i + 1:]) for m, i in zip(singles, (1, 2, 29))]
    _, _, mtoks = alphabet.get_batch_converter()(mutated)
    want["pseudo-ppl"] = model.pseudo_log_likelihood(mtoks, positions=range(1, len(seq) - 1)).tolist()

    def not_entered(*args, **kwargs):
        raise AssertionError("a table of single substitutions went through score_variants")

    monkeypatch.setattr(scoring, "score_variants", not_entered)
    pll_calls = []
    real_pll = scoring.pseudo_log_likelihood

    def recording(model_, tokens, positions=None, chunk=None):
        pll_calls.append((tokens.clone(), list(positions), chunk))
        return real_pll(model_, tokens, positions=positions, chunk=chunk)

    monkeypatch.setattr(scoring, "pseudo_log_likelihood", recording)
    for strategy, scores in want.items():
        out = tmp_path / f"singles_{strategy}.csv"
        assert predict.main(["--model-location", path, "--sequence", seq, "--dms-input", str(src1), "--dms-output", str(out),
                             "--offset-idx", "25", "--scoring-strategy", strategy]) == 0
        if strategy == "pseudo-ppl":
            # its sum has no fixed order (same_pll), so the bytes of two runs may differ in the last digit; what is pinned is
            # the path of before: ONE pseudo_log_likelihood call on the batch of the mutated sequences, the reference's positions
            same_pll([float(r[path]) for r in csv.DictReader(open(out, newline=""))], scores, len(seq) - 2)
            assert len(pll_calls) == 1 and torch.equal(pll_calls[0][0].cpu(), mtoks)
            assert pll_calls[0][1] == list(range(1, len(seq) - 1)) and pll_calls[0][2] is None
            text = out.read_text().splitlines()
            assert text[0] == f",mutant,fitness,{path}" and [t.rsplit(",", 1)[0] for t in text[1:]] == \
                [f"{i},{m},0.5" for i, m in enumerate(singles)]
            continue
        assert not pll_calls
        lines = [f",mutant,fitness,{path}"] + [f"{i},{m},0.5,{float(s)!r}" for i, (m, s) in enumerate(zip(singles, scores))]
        assert out.read_bytes() == ("\r\n".join(lines) + "\r\n").encode(), strategy


def test_forward_is_unchanged_after_variant_scoring():
    """Scoring shares the engine's workspace: the next forward gives the bits it gave before."""
    model, toks, alphabet, seq = case("esm2")
    with torch.no_grad():
        before = model(toks, repr_layers=[0, L], return_contacts=True)
    model.masked_joint(toks, SETS, src=SRC, chunk=3)
    for strategy in predict.STRATEGIES:
        model.score_variants(alphabet, seq, [sub(seq, 4, other(seq, 4)) + ":" + sub(seq, 9, other(seq, 9))], strategy=strategy,
                             offset_idx=1)
    with torch.no_grad():
        after = model(toks, repr_layers=[0, L], return_contacts=True)
    for key in ("logits", "contacts", "attentions"):
        assert torch.equal(before[key], after[key]), key
    for layer in (0, L):
        assert torch.equal(before["representations"][layer], after["representations"][layer])
    assert model._engine.workspace2 is None and model._engine.stream2 is None
