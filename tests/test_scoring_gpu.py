"""Variant scoring through the model (esm_amd/scoring.py over esmk_forward_rows): the selected rows against ``forward``, the
three strategies against the reference's masked-position loop (examples/variant-prediction/predict.py:205-215, :138-143)
run on this model's own ``forward`` at B = 1.  Synthetic models of esm_amd/synth.py, L = 2, E = 128, H = 2 (one with
head_dim 128: E = 256, H = 2).  Log-probabilities are compared with ``torch.log_softmax`` of the fp32 logits taken in fp64,
bound 4 fp32 ulp at the row's largest |reference value| (tests/_scoring_ref.py); logits and the batched-against-B = 1
comparison are bit for bit."""
import argparse
import functools

import pytest
import torch

import esm
from _scoring_ref import check_rows, masked_loop_logits, row_bound
from esm_amd import ops, scoring
from esm_amd.synth import esm1_args, synth_esm1_state_dict, synth_esm1b_state_dict, synth_esm2_state_dict, synth_tokens

pytestmark = pytest.mark.gpu
PAD = 1
L = 2


def batch(cls=0, last=2):
    """B = 2, lengths 70 and 41, T = 70: the second sequence padded."""
    toks = synth_tokens(2, 68, seed=11)
    toks[:, 0] = cls
    toks[0, -1] = last if last is not None else 9
    toks[1, 40] = last if last is not None else 9
    toks[1, 41:] = PAD
    return toks


def esm2_model(E=128, H=2, seed=3):
    model = esm.ESM2(L, E, H).eval()
    model.load_state_dict(synth_esm2_state_dict(L, E, H, seed=seed))
    return model.cuda()


def esm1b_model():
    args = argparse.Namespace(arch="roberta_large", layers=L, embed_dim=128, ffn_embed_dim=512, attention_heads=2,
                              max_positions=1024, token_dropout=True, emb_layer_norm_before=True)
    model = esm.ProteinBertModel(args, esm.Alphabet.from_architecture("roberta_large")).eval()
    model.load_state_dict(synth_esm1b_state_dict(L, 128, 2, seed=5), strict=True)
    return model.cuda()


def esm1_model():
    model = esm.ProteinBertModel(esm1_args(L, 128, 2, final_bias=True, token_dropout=True),
                                 esm.Alphabet.from_architecture("protein_bert_base")).eval()
    model.load_state_dict(synth_esm1_state_dict(L, 128, 2, seed=7, final_bias=True), strict=True)
    return model.cuda()


# ---- row selection against forward ------------------------------------------------------------------------------------
CONFIGS = {
    "f16-nofold": dict(ESM_AMD_LN_FOLD="0"),
    "f16-fold": dict(ESM_AMD_LN_FOLD="1"),
    "bf16-nofold": dict(ESM_AMD_LN_FOLD="0", ESM_AMD_OPERAND="bf16"),
    "bf16-fold": dict(ESM_AMD_LN_FOLD="1", ESM_AMD_OPERAND="bf16"),
    "head_dim128": dict(),
    "f16x2a": dict(ESM_AMD_OPERAND="f16x2a"),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_selected_rows_equal_forward(name, monkeypatch):
    for key in ("ESM_AMD_LN_FOLD", "ESM_AMD_OPERAND"):
        monkeypatch.delenv(key, raising=False)
    for key, value in CONFIGS[name].items():
        monkeypatch.setenv(key, value)
    model = esm2_model(E=256, H=2) if name == "head_dim128" else esm2_model()
    toks = batch().cuda()
    with torch.no_grad():
        full = model(toks)["logits"].float().view(-1, model.alphabet_size)
    if "LN_FOLD" in "".join(CONFIGS[name]):
        assert model.ln_fold_active() is (CONFIGS[name]["ESM_AMD_LN_FOLD"] == "1")
    real = toks.ne(PAD).view(-1).nonzero().view(-1)
    assert real.numel() == 111
    g = torch.Generator().manual_seed(1)
    for n_sel in (1, 64, 65, real.numel()):
        sel = real[torch.randperm(real.numel(), generator=g)[:n_sel].cuda()] if n_sel < real.numel() else real
        if n_sel == 1:
            sel = real[-1:]  # the last real row of the padded sequence
        lp, logits = scoring.forward_rows(model, toks, sel.to(torch.int32).contiguous(), return_logits=True)
        assert torch.equal(logits, full[sel]), f"{name} n_sel={n_sel}: selected logits differ from forward's"
        check_rows(lp, full[sel], f"forward_rows {name} n_sel={n_sel}")


def test_out_of_range_rows_are_clamped():
    """Row indices are device data: an index outside [0, B*T) reads the first / last row and does not fault."""
    model = esm2_model()
    toks = batch().cuda()
    N = toks.numel()
    sel = torch.tensor([-5, 0, N - 1, N + 1000, 2 ** 31 - 1], dtype=torch.int32).cuda()
    lp = scoring.forward_rows(model, toks, sel)
    assert torch.equal(lp[0], lp[1]) and torch.equal(lp[3], lp[2]) and torch.equal(lp[4], lp[2])


# ---- the strategies against the reference's loop -------------------------------------------------------------------------
MODELS = {"esm2": (esm2_model, dict()), "esm1b": (esm1b_model, dict()), "esm1": (esm1_model, dict(cls=32, last=None))}


@functools.lru_cache(maxsize=None)
def loop_case(kind):
    """(model, tokens, reference): the loop's fp32 logits [B, T, V], computed once per model kind and left unchanged."""
    make, tok_kw = MODELS[kind]
    model = make()
    toks = batch(**tok_kw).cuda()
    return model, toks, masked_loop_logits(model, toks)


@pytest.mark.parametrize("kind", list(MODELS))
def test_masked_marginals_against_the_loop(kind):
    model, toks, loop = loop_case(kind)
    assert bool(model.token_dropout)  # the divisor of the token dropout depends on each built sequence's mask count
    real = toks.ne(PAD)
    got = model.masked_marginals(toks, chunk=48)  # 111 rows: 48 + 48 + 15, the first boundary inside sequence 0
    assert got.shape == (2, 70, model.alphabet_size) and got.dtype == torch.float32
    check_rows(got[real], loop[real], f"masked_marginals {kind}")
    # the batched forward and the B = 1 forward agree bit for bit: the same kernel on the loop's logits gives the same bits
    assert torch.equal(got[real], ops.log_softmax_rows(loop[real].contiguous()))
    assert (got[~real] == 0).all() and torch.isfinite(got).all()
    assert torch.equal(model.masked_marginals(toks.cpu()), got)  # the default chunk, tokens from the host
    # a subset of positions: the same rows, zeros elsewhere
    some = model.masked_marginals(toks, positions=[0, 17, 40], chunk=4)
    assert torch.equal(some[:, [0, 17, 40]], got[:, [0, 17, 40]]) and int((some != 0).any(-1).sum()) == 6


@pytest.mark.parametrize("kind", list(MODELS))
def test_wt_marginals_and_pseudo_log_likelihood(kind):
    model, toks, loop = loop_case(kind)
    real = toks.ne(PAD)
    with torch.no_grad():
        full = model(toks)["logits"].float()
    wt = model.wt_marginals(toks)
    check_rows(wt[real], full[real], f"wt_marginals {kind}")
    assert (wt[~real] == 0).all() and torch.isfinite(wt).all()
    # compute_pppl's POSITIONS on one sequence of 68 residues (69 for ESM-1: no <eos>), token positions 1 .. len - 2, with the
    # log-probability of the token that was masked there — not compute_pppl itself, which reads sequence[i], the next residue
    ref = torch.log_softmax(loop.double().cpu(), -1)
    n_res = 68 if model.append_eos else 69
    positions = list(range(1, n_res - 1))
    true = toks[0, positions].cpu()
    want = ref[0, positions].gather(1, true.unsqueeze(1)).sum().item()
    bound = row_bound(ref[0, positions]).sum().item()
    got = model.pseudo_log_likelihood(toks[:1], positions=positions, chunk=32)
    assert got.shape == (1,) and got.dtype == torch.float64
    print(f"\npseudo_log_likelihood {kind}: {got.item():.9f} against {want:.9f}, err {abs(got.item() - want):.2e}, bound {bound:.2e}")
    assert abs(got.item() - want) <= bound
    # default: all residues of every sequence (no <cls>, no <eos>, no <pad>)
    res = real.clone()
    res[:, 0] = False
    if model.append_eos:
        res &= toks.ne(model.eos_idx)
    both = model.pseudo_log_likelihood(toks)
    for b in range(2):
        rows = res[b].nonzero().view(-1).cpu()
        want_b = ref[b, rows].gather(1, toks[b, rows].cpu().unsqueeze(1)).sum().item()
        assert abs(both[b].item() - want_b) <= row_bound(ref[b, rows]).sum().item()


def test_positions_on_padding_are_refused():
    model, toks, _ = loop_case("esm2")
    with pytest.raises(ValueError, match="<pad>"):
        model.masked_marginals(toks, positions=[0, 50])  # position 50 of sequence 1 is padding
    with pytest.raises(ValueError, match="outside"):
        model.masked_marginals(toks, positions=[70])
    with pytest.raises(ValueError, match="<pad>"):
        model.pseudo_log_likelihood(toks, positions=[[1, 2], [45]])
    per_seq = model.masked_marginals(toks, positions=[[0, 69], [40]])
    assert (per_seq != 0).any(-1).nonzero().tolist() == [[0, 0], [0, 69], [1, 40]]


def test_forward_is_unchanged_after_scoring():
    """Scoring shares the engine's workspace: the next forward gives the bits it gave before."""
    model = esm2_model(seed=9)
    toks = batch().cuda()
    with torch.no_grad():
        before = model(toks, repr_layers=[0, L], return_contacts=True)
    ws_before = model._engine.workspace.numel()
    model.masked_marginals(toks, chunk=40)
    model.wt_marginals(toks)
    model.pseudo_log_likelihood(toks)
    with torch.no_grad():
        after = model(toks, repr_layers=[0, L], return_contacts=True)
    for key in ("logits", "contacts", "attentions"):
        assert torch.equal(before[key], after[key]), key
    for layer in (0, L):
        assert torch.equal(before["representations"][layer], after["representations"][layer])
    # one workspace, grown at most to the largest call; no second buffer or stream was made
    assert model._engine.workspace.numel() >= ws_before and model._engine.workspace2 is None and model._engine.stream2 is None


def test_predict_cli_end_to_end(tmp_path):
    """``python -m esm_amd.predict`` (called in process) on a synthetic checkpoint: every strategy's column is what the
    methods give for the same sequence and mutations."""
    import csv

    from esm_amd import predict
    from esm_amd.synth import write_esm2_checkpoint

    path = write_esm2_checkpoint(str(tmp_path), "esm2_t2_synth", L, 128, 2, seed=3)
    seq = "MKTAYIAKQRQISFVKSHFSRQLEERLGLI"
    muts = ["K26G", "T27C", "I54A"]  # offset 25: residues 1, 2, 29
    src = tmp_path / "scan.csv"
    src.write_text("mutant,fitness\n" + "".join(f"{m},0\n" for m in muts))
    model, alphabet = esm.pretrained.load_model_and_alphabet(path)
    model = model.eval().cuda()
    _, _, toks = alphabet.get_batch_converter()([("protein1", seq)])
    want = {"wt-marginals": scoring.score_mutations(model.wt_marginals(toks).cpu(), seq, muts, alphabet, 25),
            "masked-marginals": scoring.score_mutations(model.masked_marginals(toks).cpu(), seq, muts, alphabet, 25)}
    mutated = [(m, seq[:i] + m[-1] + seq[i + 1:]) for m, i in zip(muts, (1, 2, 29))]
    _, _, mtoks = alphabet.get_batch_converter()(mutated)
    want["pseudo-ppl"] = model.pseudo_log_likelihood(mtoks, positions=range(1, len(seq) - 1)).tolist()
    for strategy, scores in want.items():
        out = tmp_path / f"{strategy}.csv"
        assert predict.main(["--model-location", path, "--sequence", seq, "--dms-input", str(src), "--dms-output", str(out),
                             "--offset-idx", "25", "--scoring-strategy", strategy]) == 0
        rows = list(csv.DictReader(open(out, newline="")))
        assert [r["mutant"] for r in rows] == muts and [float(r[path]) for r in rows] == [float(s) for s in scores], strategy
    with pytest.raises(ValueError, match="wild type"):
        predict.score_table(model, alphabet, seq, ["A26G"], "pseudo-ppl", 25)


def test_errors_past_the_entry_checks_name_the_entry(monkeypatch):
    """A refusal that comes from the shared forward code is reported under esmk_forward_rows, not esmk_forward: here the
    LayerNorm fold's check that the packed image is the one the handle packed."""
    import ctypes

    from esm_amd import _native as N

    monkeypatch.setenv("ESM_AMD_LN_FOLD", "1")
    monkeypatch.delenv("ESM_AMD_OPERAND", raising=False)
    model = esm2_model()
    toks = batch().cuda()
    sel = torch.arange(4, dtype=torch.int32).cuda()
    scoring.forward_rows(model, toks, sel)
    eng = model._engine
    other = eng.packed.clone()
    out = torch.empty((4, model.alphabet_size), dtype=torch.float32, device="cuda")
    rc = N.lib.esmk_forward_rows(eng.handle, N.ptr(other), N.ptr(toks), 2, 70, N.ptr(sel), 4, N.ptr(out), N.ptr(eng.workspace),
                                 eng.workspace.numel(), N.cur_stream())
    assert rc != 0 and N.lib.esmk_last_error().decode().startswith("esmk_forward_rows: LayerNorm fold")
    rc = N.lib.esmk_forward(eng.handle, N.ptr(other), N.ptr(toks), 2, 70, None, 0, None, 0, None, None, None,
                            N.ptr(eng.workspace), eng.workspace.numel(), N.cur_stream())
    assert rc != 0 and N.lib.esmk_last_error().decode().startswith("esmk_forward: LayerNorm fold")
