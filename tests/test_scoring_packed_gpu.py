"""Mixed-length libraries scored token-packed (esm_amd/scoring.py: ``forward_rows_packed`` over esmk_forward_packed_rows, the
``varlen=True`` form of the strategies, ``python -m esm_amd.score_sequences``).  Every kernel on the path computes a row from
that row's own sequence alone, so everything here is bit-equality with the padded path of the same model (``torch.equal``), or
equality with a sequential fp64 sum on the host; no tolerance.  Toy models of tests/test_scoring_gpu.py (L = 2, E = 128, H = 2;
one with head_dim 128; ESM-1b with token dropout and emb_layer_norm_before; ESM-1 for the refusals); sequences of 3, 15, 16, 17,
63, 64, 65, 129 and 130 tokens, one with an interior <pad> (tests/_scoring_packed_ref.py)."""
import csv
import ctypes
import functools

import pytest
import torch

import esm
from _scoring_packed_ref import INTERIOR_PAD, LENGTHS, MASK, PAD, aligned_starts, library
from esm_amd import _native as N
from esm_amd import score_sequences, scoring
from test_scoring_gpu import CONFIGS, L, esm1_model, esm1b_model, esm2_model

pytestmark = pytest.mark.gpu
T = max(LENGTHS)


def hand_packed(toks, rows=640):
    """The library laid out by hand: (flat int64 [rows], segments int32 [9, 2], padded flat rows, packed flat rows) of every
    non-pad token.  576 rows hold the segments; the row space ends in a gap of 64 rows."""
    starts, used = aligned_starts(LENGTHS)
    assert used == 576 and rows % 64 == 0
    flat = torch.full((rows,), PAD, dtype=torch.int64)
    sel_pad, sel_pk = [], []
    for b, (s, n) in enumerate(zip(starts, LENGTHS)):
        flat[s:s + n] = toks[b, :n]
        for t in range(n):
            if toks[b, t] != PAD:
                sel_pad.append(b * T + t)
                sel_pk.append(s + t)
    seg = torch.tensor([[s, n] for s, n in zip(starts, LENGTHS)], dtype=torch.int32)
    as_dev = lambda v: torch.tensor(v, dtype=torch.int32).cuda()
    return flat.cuda(), seg, as_dev(sel_pad), as_dev(sel_pk)


PACKED_CONFIGS = dict(CONFIGS)
PACKED_CONFIGS.update({"half-model": dict(), "bf16-model": dict(), "esm1b": dict(), "esm1b-fold": dict(ESM_AMD_LN_FOLD="1")})


@pytest.mark.parametrize("name", list(PACKED_CONFIGS))
def test_packed_rows_equal_padded_rows(name, monkeypatch):
    for key in ("ESM_AMD_LN_FOLD", "ESM_AMD_OPERAND"):
        monkeypatch.delenv(key, raising=False)
    for key, value in PACKED_CONFIGS[name].items():
        monkeypatch.setenv(key, value)
    if name.startswith("esm1b"):
        model = esm1b_model()
    else:
        model = esm2_model(E=256, H=2) if name == "head_dim128" else esm2_model()
    if name == "half-model":
        model = model.half()
    if name == "bf16-model":
        model = model.bfloat16()
    toks = library()
    toks[3, 5] = MASK  # the token-dropout divisor is per sequence
    toks[7, 100] = MASK
    flat, seg, sel_pad, sel_pk = hand_packed(toks)
    assert sel_pad.numel() == sum(LENGTHS) - 1
    lp_pad, logits_pad = scoring.forward_rows(model, toks.cuda(), sel_pad, return_logits=True)
    lp_pk, logits_pk = scoring.forward_rows_packed(model, flat, seg, sel_pk, return_logits=True)
    if "LN_FOLD" in "".join(PACKED_CONFIGS[name]):
        assert model.ln_fold_active() is (PACKED_CONFIGS[name]["ESM_AMD_LN_FOLD"] == "1")
    assert logits_pk.dtype == torch.float32 and logits_pk.shape == (sel_pk.numel(), model.alphabet_size)
    assert torch.isfinite(lp_pk).all()
    assert torch.equal(logits_pk, logits_pad), f"{name}: packed logits differ from the padded batch's"
    assert torch.equal(lp_pk, lp_pad), f"{name}: packed log-probabilities differ from the padded batch's"
    # without the logits, a subset in another order, indices outside the row space clamped to its ends
    some = torch.tensor([sel_pk[-1].item(), 0, 17, -4, 10 ** 6], dtype=torch.int32).cuda()
    lp = scoring.forward_rows_packed(model, flat, seg, some)
    assert lp.shape == (5, model.alphabet_size)  # (row 4 is the last gap row, whose values are undefined)
    assert torch.equal(lp[0], lp_pk[-1]) and torch.equal(lp[1], lp_pk[0]) and torch.equal(lp[3], lp_pk[0])
    assert torch.equal(lp[2], lp_pk[sel_pk.tolist().index(17)])


@functools.lru_cache(maxsize=None)
def case(kind="esm2"):
    """(model, tokens [9, 130] on the device)."""
    model = {"esm2": esm2_model, "esm1b": esm1b_model}[kind]()
    assert bool(model.token_dropout)
    return model, library().cuda()


@pytest.mark.parametrize("kind", ["esm2", "esm1b"])
def test_masked_marginals_varlen_equal_padded(kind):
    model, toks = case(kind)
    padded = model.masked_marginals(toks)
    packed = model.masked_marginals(toks, varlen=True)
    assert packed.shape == (len(LENGTHS), T, model.alphabet_size) and packed.dtype == torch.float32
    assert torch.equal(packed, padded)
    real = toks.ne(PAD)
    assert (packed[~real] == 0).all() and (packed[real] != 0).any(-1).all() and not real[INTERIOR_PAD]
    assert torch.equal(scoring.masked_marginals(model, toks.cpu(), varlen=True), padded)  # tokens from the host
    # a positions mask; packed row spaces of 256 rows (one 129- or 130-token copy each) against the default budget
    g = torch.Generator().manual_seed(2)
    want = (real.cpu() & (torch.rand(real.shape, generator=g) < 0.12))
    want[0, 1] = want[8, 129] = want[7, 0] = True
    some = model.masked_marginals(toks, positions=want, varlen=True)
    assert torch.equal(some, model.masked_marginals(toks, positions=want))
    assert torch.equal(some[want], padded[want]) and (some[~want] == 0).all()
    assert torch.equal(model.masked_marginals(toks, positions=want, varlen=True, chunk_rows=256), some)
    # per-sequence lists: a sequence with nothing to score contributes no segment
    lists = [[1], [], [0, 14], [], [], [63, 31], [], [], [129]]
    assert torch.equal(model.masked_marginals(toks, positions=lists, varlen=True), model.masked_marginals(toks, positions=lists))
    with pytest.raises(ValueError, match="<pad>"):
        model.masked_marginals(toks, positions=[[1], [20]] + [[]] * 7, varlen=True)  # position 20 of the 15-token sequence
    # chunk_rows sizes packed row spaces only: without varlen=True it is refused, not dropped
    with pytest.raises(ValueError, match="chunk_rows"):
        model.masked_marginals(toks, chunk_rows=256)
    with pytest.raises(ValueError, match="chunk_rows"):
        scoring.pseudo_log_likelihood(model, toks, chunk_rows=256)


def test_packed_chunks_are_what_the_planner_says(monkeypatch):
    model, toks = case("esm2")
    calls = []
    real_call = scoring.forward_rows_packed

    def recording(model_, tokens_flat, segments, sel_rows, return_logits=False):
        calls.append((tokens_flat.numel(), segments.tolist(), sel_rows.tolist()))
        assert bool((tokens_flat[int(segments[-1].sum()):] == PAD).all())  # the gap behind the last copy
        return real_call(model_, tokens_flat, segments, sel_rows, return_logits=return_logits)

    monkeypatch.setattr(scoring, "forward_rows_packed", recording)
    lists = [[1], [], [0, 14], [], [], [63, 31], [], [], [129, 5]]
    model.masked_marginals(toks, positions=lists, varlen=True, chunk_rows=256)
    # copies in (sequence, position) order: 3, 16, 16, 64 and 64 tokens fill 176 rows; a 130-token copy (144 rows) would pass
    # 256, so each of the two gets a row space of its own
    assert calls == [(192, [[0, 3], [16, 16], [32, 16], [48, 64], [112, 64]], [1, 16, 46, 79, 175]),
                     (192, [[0, 130]], [5]), (192, [[0, 130]], [129])]


@pytest.mark.parametrize("kind", ["esm2", "esm1b"])
def test_masked_joint_and_wt_marginals_varlen_equal_padded(kind):
    model, toks = case(kind)
    sets = [[1], [0, 14], [5, 6, 16], [62], [1, 63, 31], [64, 0], [128, 2], [129, 1, 64], [2, 1]]
    src = [0, 1, 3, 4, 5, 6, 7, 8, 2]  # sets of different sequences, not in sequence order
    want = model.masked_joint(toks, sets, src=src, return_logits=True)
    for kw in (dict(), dict(chunk_rows=256)):
        got = model.masked_joint(toks, sets, src=src, return_logits=True, varlen=True, **kw)
        assert len(got) == 4 and all(torch.equal(g, w) for g, w in zip(got, want)), kw
    got3 = model.masked_joint(toks, sets, src=src, varlen=True)
    assert len(got3) == 3 and torch.equal(got3[2], want[2])
    assert not torch.equal(want[2][1], model.masked_marginals(toks[1:2], positions=[0])[0, 0])  # the joint mask is in use
    wt = model.wt_marginals(toks)
    assert torch.equal(model.wt_marginals(toks, varlen=True), wt)
    assert torch.equal(model.wt_marginals(toks.cpu(), varlen=True, chunk_rows=256), wt)
    assert (wt[toks.eq(PAD)] == 0).all()


@pytest.mark.parametrize("kind", ["esm2", "esm1b"])
def test_pseudo_log_likelihood_varlen_is_the_sequential_sum(kind):
    model, toks = case(kind)
    table = model.masked_marginals(toks).cpu()
    tok = toks.cpu()
    got = model.pseudo_log_likelihood(toks, varlen=True)
    assert got.shape == (len(LENGTHS),) and got.dtype == torch.float64
    want = []
    for b, n in enumerate(LENGTHS):
        acc = 0.0
        for t in range(1, n - 1):  # the residues: no <cls>, no <eos>
            if tok[b, t] != PAD:
                acc += table[b, t, tok[b, t]].item()  # an fp32 value as a Python float, added in fp64
        want.append(acc)
    assert got.tolist() == want and all(w < 0 for w in want)
    assert want[0] == table[0, 1, tok[0, 1]].item()  # one residue
    assert model.pseudo_log_likelihood(toks, varlen=True, chunk_rows=1024).tolist() == want
    # the reference's positions on one sequence, and per-sequence lists with empty ones
    one = model.pseudo_log_likelihood(toks[8:9], positions=range(1, 128), varlen=True)
    acc = 0.0
    for t in range(1, 128):
        acc += table[8, t, tok[8, t]].item()
    assert one.tolist() == [acc]
    lists = [[1], [], [3, 2], [], [], [], [], [], []]
    some = model.pseudo_log_likelihood(toks, positions=lists, varlen=True).tolist()
    assert some == [want[0], 0.0, table[2, 2, tok[2, 2]].item() + table[2, 3, tok[2, 3]].item()] + [0.0] * 6
    # the padded path adds the same terms through atomics: the same number up to the rounding of an fp64 sum
    for p, w in zip(model.pseudo_log_likelihood(toks).tolist(), want):
        assert abs(p - w) <= 2 * 130 * 2.0 ** -53 * abs(w)


# ---- refusals and fall-back -----------------------------------------------------------------------------------------
def test_esm1_is_refused_by_the_entry_and_falls_back_in_the_strategies():
    model = esm1_model()
    toks = library(cls=32, eos=9)
    flat, seg, _, sel_pk = hand_packed(toks)
    before = model.masked_marginals(toks.cuda(), positions=[1, 2])
    with pytest.raises(N.EsmkError, match=r"esmk_packed_rows_workspace_bytes: ESM-1 .*no token-packed form"):
        scoring.forward_rows_packed(model, flat, seg, sel_pk)
    eng = model._engine
    out = torch.empty((4, model.alphabet_size), dtype=torch.float32, device="cuda")
    seg_ptr = ctypes.cast(seg.data_ptr(), ctypes.POINTER(ctypes.c_int32))
    rc = N.lib.esmk_forward_packed_rows(eng.handle, N.ptr(eng.packed), N.ptr(flat), seg_ptr, len(LENGTHS), 640, N.ptr(sel_pk), 4,
                                        N.ptr(out), N.ptr(eng.workspace), eng.workspace.numel(), N.cur_stream())
    assert rc != 0 and N.lib.esmk_last_error().decode().startswith("esmk_forward_packed_rows: ESM-1")
    # varlen=True on a model without a packed forward: the padded result, and the model still runs
    assert torch.equal(model.masked_marginals(toks.cuda(), positions=[1, 2], varlen=True), before)
    assert torch.equal(model.wt_marginals(toks, varlen=True), model.wt_marginals(toks))
    pll = model.pseudo_log_likelihood(toks[:4], varlen=True)
    assert pll.shape == (4,) and bool((pll < 0).all())
    got = model.masked_joint(toks, [[1, 2]], src=[3], varlen=True)
    assert torch.equal(got[2], model.masked_joint(toks, [[1, 2]], src=[3])[2])


def test_f16x3_is_refused_by_the_entry_and_falls_back_in_the_strategies(monkeypatch):
    monkeypatch.delenv("ESM_AMD_LN_FOLD", raising=False)
    monkeypatch.setenv("ESM_AMD_OPERAND", "f16x3")
    model = esm2_model()
    toks = library()
    flat, seg, _, sel_pk = hand_packed(toks)
    before = model.masked_marginals(toks, positions=[1, 2])
    with pytest.raises(N.EsmkError, match=r"esmk_packed_rows_workspace_bytes: the f16x3 precision mode"):
        scoring.forward_rows_packed(model, flat, seg, sel_pk)
    eng = model._engine
    out = torch.empty((4, model.alphabet_size), dtype=torch.float32, device="cuda")
    seg_ptr = ctypes.cast(seg.data_ptr(), ctypes.POINTER(ctypes.c_int32))
    rc = N.lib.esmk_forward_packed_rows(eng.handle, N.ptr(eng.packed), N.ptr(flat), seg_ptr, len(LENGTHS), 640, N.ptr(sel_pk), 4,
                                        N.ptr(out), N.ptr(eng.workspace), eng.workspace.numel(), N.cur_stream())
    assert rc != 0 and N.lib.esmk_last_error().decode().startswith("esmk_forward_packed_rows: the f16x3 precision mode")
    assert torch.equal(model.masked_marginals(toks, positions=[1, 2], varlen=True), before)
    assert torch.equal(model.masked_marginals(toks, positions=[1, 2]), before)  # the model still runs


def test_msa_handle_is_refused_at_the_c_entry():
    cfg = N.EsmkMsaConfig(2, 128, 2, 256, 33, 1, 32, 0, 2, 1, 0, 1026, 1, N.dtype_code(torch.float16))
    hm = ctypes.c_void_p()
    assert N.lib.esmk_msa_create(ctypes.byref(cfg), ctypes.byref(hm)) == 0
    toks = library()
    flat, seg, _, sel_pk = hand_packed(toks)
    seg_ptr = ctypes.cast(seg.data_ptr(), ctypes.POINTER(ctypes.c_int32))
    need = ctypes.c_size_t()
    assert N.lib.esmk_packed_rows_workspace_bytes(hm, seg_ptr, len(LENGTHS), 640, 4, ctypes.byref(need), None) != 0
    assert N.lib.esmk_last_error().decode() == "esmk_packed_rows_workspace_bytes: not an ESM-2 handle"
    out = torch.empty((4, 33), dtype=torch.float32, device="cuda")
    ws = torch.empty((1 << 20,), dtype=torch.uint8, device="cuda")
    rc = N.lib.esmk_forward_packed_rows(hm, N.ptr(ws), N.ptr(flat), seg_ptr, len(LENGTHS), 640, N.ptr(sel_pk), 4, N.ptr(out),
                                        N.ptr(ws), ws.numel(), N.cur_stream())
    assert rc != 0 and N.lib.esmk_last_error().decode() == "esmk_forward_packed_rows: not an ESM-2 handle"
    N.lib.esmk_destroy(hm)
    with pytest.raises(NotImplementedError, match="MSA Transformer"):
        from esm_amd.msa_transformer import MSATransformer

        scoring.forward_rows_packed(MSATransformer.__new__(MSATransformer), flat, seg, sel_pk)


def test_errors_past_the_entry_checks_name_the_entry(monkeypatch):
    """A refusal from the shared forward code is reported under esmk_forward_packed_rows: the LayerNorm fold's check that
    the packed image is the one the handle packed."""
    monkeypatch.setenv("ESM_AMD_LN_FOLD", "1")
    monkeypatch.delenv("ESM_AMD_OPERAND", raising=False)
    model = esm2_model()
    flat, seg, _, sel_pk = hand_packed(library())
    scoring.forward_rows_packed(model, flat, seg, sel_pk)
    eng = model._engine
    other = eng.packed.clone()
    out = torch.empty((4, model.alphabet_size), dtype=torch.float32, device="cuda")
    seg_ptr = ctypes.cast(seg.data_ptr(), ctypes.POINTER(ctypes.c_int32))
    rc = N.lib.esmk_forward_packed_rows(eng.handle, N.ptr(other), N.ptr(flat), seg_ptr, len(LENGTHS), 640, N.ptr(sel_pk), 4,
                                        N.ptr(out), N.ptr(eng.workspace), eng.workspace.numel(), N.cur_stream())
    assert rc != 0 and N.lib.esmk_last_error().decode().startswith("esmk_forward_packed_rows: LayerNorm fold")


def test_forward_is_unchanged_after_packed_scoring():
    """Packed scoring shares the engine's workspace: the next forward, padded or packed, gives the bits it gave before."""
    model = esm2_model(seed=9)
    toks = library().cuda()
    with torch.no_grad():
        before = model(toks, repr_layers=[0, L], return_contacts=True)
        before_pk = model.forward_varlen(toks, repr_layers=[L], min_saving=None)
    model.masked_marginals(toks, positions=[1, 2], varlen=True)
    model.wt_marginals(toks, varlen=True)
    model.pseudo_log_likelihood(toks[:4], varlen=True)
    with torch.no_grad():
        after = model(toks, repr_layers=[0, L], return_contacts=True)
        after_pk = model.forward_varlen(toks, repr_layers=[L], min_saving=None)
    for key in ("logits", "contacts", "attentions"):
        assert torch.equal(before[key], after[key]), key
    assert torch.equal(before["representations"][L], after["representations"][L])
    assert torch.equal(before_pk["logits"], after_pk["logits"])
    assert model._engine.workspace2 is None and model._engine.stream2 is None


# ---- python -m esm_amd.score_sequences --------------------------------------------------------------------------------
SEQS = [("one", "M"), ("short", "MKTAYIAKQRQISF"), ("edge", "MKTAYIAKQRQISFV"), ("mid", "ACDEFGHIKLMNPQRSTVWY" * 3 + "AC"),
        ("tile", "ACDEFGHIKLMNPQRSTVWY" * 3 + "ACDE"), ("long", "MKTAYIAKQRQISFVKSHFSRQLEERLGLIEVQ" * 4)]


def test_score_sequences_cli(tmp_path):
    from esm_amd.synth import write_esm2_checkpoint

    path = write_esm2_checkpoint(str(tmp_path), "esm2_t2_synth", L, 128, 2, seed=3)
    fasta = tmp_path / "lib.fasta"
    fasta.write_text("".join(f">{label}\n{seq[:40]}\n{seq[40:]}\n" for label, seq in SEQS))
    table = tmp_path / "lib.csv"
    table.write_text("name,sequence,note\n" + "".join(f"{label},{seq},x\n" for label, seq in SEQS))
    model, alphabet = esm.pretrained.load_model_and_alphabet(path)
    model = model.eval().cuda()
    _, _, toks = alphabet.get_batch_converter()(SEQS)
    assert toks.shape == (6, 134) and [len(s) + 2 for _, s in SEQS] == [3, 16, 17, 64, 66, 134]
    want = model.pseudo_log_likelihood(toks, varlen=True).tolist()

    def run(*extra):
        out = tmp_path / ("out_" + "_".join(e.strip("-") for e in extra if e.startswith("--")) + ".csv")
        assert score_sequences.main(["--model-location", path, "--output", str(out)] + list(extra)) == 0
        return out, list(csv.DictReader(open(out, newline="")))

    out, rows = run("--fasta", str(fasta))
    assert [r["label"] for r in rows] == [label for label, _ in SEQS]
    assert [int(r["length"]) for r in rows] == [len(seq) for _, seq in SEQS]
    assert [float(r["pll"]) for r in rows] == want  # the API's floats
    import math

    assert [float(r["pseudo_perplexity"]) for r in rows] == [math.exp(-w / len(seq)) for w, (_, seq) in zip(want, SEQS)]
    assert out.read_text().splitlines()[0] == "label,length,pll,pseudo_perplexity"
    out_csv, rows_csv = run("--csv", str(table), "--sequence-col", "sequence", "--label-col", "name")
    assert out_csv.read_bytes() == out.read_bytes()
    _, rows_num = run("--csv", str(table), "--sequence-col", "sequence", "--strategy", "pseudo-ppl")
    assert [r["label"] for r in rows_num] == [str(i) for i in range(6)] and [r["pll"] for r in rows_num] == [r["pll"] for r in rows]
    # the padded path: the same terms through an atomic fp64 sum; the packed column is the exact one
    _, rows_pad = run("--fasta", str(fasta), "--no-varlen")
    for p, w in zip(rows_pad, rows):
        assert abs(float(p["pll"]) - float(w["pll"])) <= 1e-12 * abs(float(w["pll"]))
        assert abs(float(p["pseudo_perplexity"]) - float(w["pseudo_perplexity"])) <= 1e-12 * float(w["pseudo_perplexity"])
    # wt-marginals: one table, one ordered sum on both paths: the same file byte for byte
    out_wt, rows_wt = run("--fasta", str(fasta), "--strategy", "wt-marginals")
    out_wt_pad, _ = run("--fasta", str(fasta), "--strategy", "wt-marginals", "--no-varlen")
    assert out_wt.read_bytes() == out_wt_pad.read_bytes()
    wt = model.wt_marginals(toks).cpu()
    for b, (r, (_, seq)) in enumerate(zip(rows_wt, SEQS)):
        acc = 0.0
        for t in range(1, len(seq) + 1):
            acc += wt[b, t, toks[b, t]].item()
        assert float(r["pll"]) == acc
    assert [float(r["pll"]) for r in rows_wt] != want


def test_score_sequences_refuses_sequences_past_the_positional_limit():
    model = esm1b_model()  # max_positions 1024
    alphabet = esm.Alphabet.from_architecture("roberta_large")
    with pytest.raises(ValueError, match="Sequence length 1102 above maximum"):
        score_sequences.score_records(model, alphabet, [("ok", "MKT"), ("long", "A" * 1100)])
