"""Edits of the residual stream through the model (esm_amd/interventions.py over esmk_set_stream_edits): ``forward_edited`` and
``model.stream_edits`` on synthetic models of esm_amd/synth.py — ESM-2 with L = 3, E = 128, H = 2, one ESM-2 with E = 96,
H = 6 (head_dim 16: operand rows of stride Kp = 128 != E) and one ESM-1b — at B = 3, T = 41 with one row padded, in both
LayerNorm-fold settings.

The ``contract ...`` lines test_contract prints are the record (profiles/stream_edit_contract_lines.txt): the engine against
the fp32 forward with the same edits (tests/_stream_edit_ref.py) next to the floor in the engine's own form."""
import argparse
import functools

import numpy as np
import pytest
import torch

import _contract as C
import _stream_edit_ref as R
import esm
from esm_amd import StreamEdit, ops, scoring
from esm_amd.interventions import plan_edits
from esm_amd.synth import synth_esm1b_state_dict, synth_esm2_state_dict, synth_tokens

pytestmark = pytest.mark.gpu
L, B, T = 3, 3, 41
DIMS = {"esm2": (128, 2), "esm2_96": (96, 6), "esm1b": (128, 2)}
FOLD = pytest.mark.parametrize("fold", [True, False], ids=["fold", "plain"])


@functools.lru_cache(maxsize=None)
def state(kind):
    E, H = DIMS[kind]
    return synth_esm1b_state_dict(L, E, H, seed=5) if kind == "esm1b" else synth_esm2_state_dict(L, E, H, seed=11)


@functools.lru_cache(maxsize=None)
def model_of(kind):
    E, H = DIMS[kind]
    if kind == "esm1b":
        args = argparse.Namespace(arch="roberta_large", layers=L, embed_dim=E, ffn_embed_dim=4 * E, attention_heads=H,
                                  max_positions=1024, token_dropout=True, emb_layer_norm_before=True)
        model = esm.ProteinBertModel(args, esm.Alphabet.from_architecture("roberta_large")).eval()
    else:
        model = esm.ESM2(L, E, H).eval()
    model.load_state_dict(state(kind), strict=True)
    return model.cuda()


def in_mode(kind, fold, monkeypatch):
    """The shared model of ``kind`` with its engine in the asked LayerNorm-fold setting."""
    monkeypatch.setenv("ESM_AMD_LN_FOLD", "1" if fold else "0")
    model = model_of(kind)
    model(batch().cuda())
    assert model.ln_fold_active() is fold
    return model


def batch(pads=True, seed=12):
    toks = synth_tokens(B, T - 2, seed=seed)
    if pads:
        toks[1, 30] = 2
        toks[1, 31:] = 1
    return toks


def same(a, b, what=""):
    assert a.keys() == b.keys(), what
    for key in a:
        if key == "representations":
            assert a[key].keys() == b[key].keys()
            for k in a[key]:
                assert torch.equal(a[key][k], b[key][k]), (what, "representation", k)
        else:
            assert torch.equal(a[key], b[key]), (what, key)


# ---- 1. nothing set, nothing changes --------------------------------------------------------------------------------------------
@FOLD
@pytest.mark.parametrize("kind", list(DIMS))
def test_no_edits_is_forward(kind, fold, monkeypatch):
    model, toks = in_mode(kind, fold, monkeypatch), batch().cuda()
    kw = dict(repr_layers=list(range(L + 1)), return_contacts=True)
    base = model(toks, **kw)
    assert set(base) == {"logits", "representations", "attentions", "contacts"}
    same(model.forward_edited(toks, [], **kw), base, "forward_edited with no edits")
    with model.stream_edits([]):
        same(model(toks, **kw), base, "an empty context")
    assert model._engine.edits is None
    same(model.forward_edited(toks, [StreamEdit(1, "zero", positions=torch.zeros(B, T, dtype=torch.bool))], **kw), base,
         "an edit of no row")
    assert model._engine.edits is None  # cleared when the call ends


# ---- 2. the identity edit ----------------------------------------------------------------------------------------------------
@FOLD
@pytest.mark.parametrize("kind", list(DIMS))
def test_identity_edit(kind, fold, monkeypatch):
    model, toks = in_mode(kind, fold, monkeypatch), batch().cuda()
    kw = dict(repr_layers=list(range(L + 1)))
    base = model(toks, **kw)
    for k in range(L + 1):
        out = model.forward_edited(toks, [StreamEdit(k, "scale", gain=1.0, positions="all")], **kw)
        if not fold or k in (0, L):
            same(out, base, f"identity at layer {k}")
        else:
            # the rows re-enter the fold's chain through rowstats' arithmetic: their fp16 operand rows are rounded around another
            # mean, once — a change of the size of the fp16-operand floor (1e-3), not of a row that lost its statistics (order 1)
            l2, mx = C.errors(out["logits"], base["logits"], toks.ne(1))
            print(f"\nidentity edit {kind} layer {k}: logits rel L2 {l2:.2e}, max {mx:.2e} against forward")
            assert mx < 1e-2, (k, l2, mx)
            for j in range(k + 1):  # the stream up to the edit is untouched, and x' = 1 * x is x
                assert torch.equal(out["representations"][j], base["representations"][j]), (k, j)


# ---- 3. patching closes the loop ---------------------------------------------------------------------------------------------
@FOLD
def test_patching_run_a_into_run_b(fold, monkeypatch):
    model = in_mode("esm2", fold, monkeypatch)
    toks_a, toks_b = batch(pads=False, seed=12).cuda(), batch(pads=False, seed=31).cuda()
    layers = list(range(L + 1))
    a = model(toks_a, repr_layers=layers)
    b = model(toks_b, repr_layers=layers)
    assert not torch.equal(a["logits"], b["logits"])
    for k in ([0] if fold else range(L)):
        out = model.forward_edited(toks_b, [StreamEdit(k, "set", a["representations"][k], positions="all")], repr_layers=layers)
        assert torch.equal(out["logits"], a["logits"]), k
        for j in layers:
            want = a if j >= k else b
            assert torch.equal(out["representations"][j], want["representations"][j]), (k, j)


# ---- 4. the contract ------------------------------------------------------------------------------------------------------------
def contract_case(kind):
    """The batch and the three edits: an ``add`` of a random direction of about the stream's row norm on the residues at layer 1,
    a ``set`` of five listed rows at layer 2, a ``project`` of every token at layer L."""
    from oracle.esm2_oracle import esm2_forward

    E, H = DIMS[kind]
    toks = batch()
    g = torch.Generator().manual_seed(13)
    ref1 = esm2_forward(state(kind), toks, L, H, repr_layers=[1, 2])["representations"]
    direction = torch.randn(E, generator=g)
    direction = direction / direction.norm() * ref1[1][toks.ne(1)].norm(dim=-1).mean()
    patch = torch.randn(5, E, generator=g) * ref1[2][toks.ne(1)].std()
    listed = torch.tensor([[0, 0], [0, 7], [1, 30], [2, 40], [2, 13]])
    return toks, [StreamEdit(1, "add", direction, positions="residues"), StreamEdit(2, "set", patch, positions=listed),
                  StreamEdit(L, "project", torch.randn(E, generator=g), positions="all")]


@FOLD
@pytest.mark.parametrize("kind", ["esm2", "esm2_96"])
def test_contract(kind, fold, monkeypatch):
    model = in_mode(kind, fold, monkeypatch)
    E, H = DIMS[kind]
    toks, edits = contract_case(kind)
    layers = list(range(L + 1))
    plans = plan_edits(model, edits, B, T)
    ref = R.forward_edited_ref(state(kind), toks, L, H, edits=plans, repr_layers=layers)
    floor = C.floor_forward(state(kind), toks, L, H, model=model, forward=R.forward_edited_ref, edits=plans, repr_layers=layers)
    plain = R.forward_edited_ref(state(kind), toks, L, H, repr_layers=layers)
    # the edits are no small thing: every output from layer 1 on moves by far more than the contract's 1e-3
    assert C.errors(ref["logits"], plain["logits"], toks.ne(1))[1] > 0.05
    out = model.forward_edited(toks.cuda(), edits, repr_layers=layers)
    mode = "fold" if fold else "plain"
    nonpad = toks.ne(1)
    C.check_tensors(f"stream_edit {kind} {mode} logits", out["logits"], ref["logits"], floor["logits"], nonpad, deep=False)
    for k in layers:
        C.check_tensors(f"stream_edit {kind} {mode} repr {k}", out["representations"][k], ref["representations"][k],
                        floor["representations"][k], nonpad, deep=False)


# ---- 5. locality -----------------------------------------------------------------------------------------------------------------
@FOLD
@pytest.mark.parametrize("kind", ["esm2", "esm1b"])
def test_an_edit_at_the_last_layer_moves_its_rows_only(kind, fold, monkeypatch):
    model, toks = in_mode(kind, fold, monkeypatch), batch().cuda()
    E = DIMS[kind][0]
    vec = torch.randn(E, generator=torch.Generator().manual_seed(3))
    base = model(toks)["logits"]

    def moved(edit):
        out = model.forward_edited(toks, [edit])["logits"]
        return (out != base).any(-1).cpu()

    listed = torch.tensor([[0, 3], [1, 30], [1, 35], [2, 0], [2, 40]])  # a residue, an <eos>, a <pad>, a <cls>, the last row
    want = torch.zeros(B, T, dtype=torch.bool)
    want[listed[:, 0], listed[:, 1]] = True
    assert torch.equal(moved(StreamEdit(L, "add", vec, positions=listed)), want)
    cpu = toks.cpu()
    assert torch.equal(moved(StreamEdit(L, "add", vec, positions="all")), cpu.ne(1))  # <pad> rows keep forward's bits
    assert torch.equal(moved(StreamEdit(L, "add", vec, positions="residues")), cpu.ne(1) & cpu.ne(0) & cpu.ne(2))


# ---- 6. applications ---------------------------------------------------------------------------------------------------------
def steer(E, layer=1, gain=4.0):
    vec = torch.randn(E, generator=torch.Generator().manual_seed(17))
    return [StreamEdit(layer, "add", vec, gain=gain, positions="residues")]


@FOLD
def test_scoring_runs_steered(fold, monkeypatch):
    model, toks = in_mode("esm2", fold, monkeypatch), batch().cuda()
    edits = steer(128)
    logits = model.forward_edited(toks, edits)["logits"]
    real = toks.ne(1)
    with model.stream_edits(edits):
        wt = model.wt_marginals(toks)
    assert torch.equal(wt[real], ops.log_softmax_rows(logits[real].contiguous()))
    assert not torch.equal(wt, model.wt_marginals(toks))  # outside the context: the unsteered model


def test_sampling_runs_steered():
    import test_sampling_gpu as S

    model, toks = model_of("esm2"), S.batch()
    edits = steer(128)
    with model.stream_edits(edits):
        final, traj = model.gibbs_sample(toks, 2, per_step=3, seed=S.SEED, return_trajectory=True)
        lists = S.residue_lists(toks, model)
        S.replay(model, toks, final, traj, lists, 3, epochs=2)  # every recorded row is masked_joint's under the same context
    plain, traj0 = model.gibbs_sample(toks, 2, per_step=3, seed=S.SEED, return_trajectory=True)
    assert not np.array_equal(S.host(traj)["logprobs"], S.host(traj0)["logprobs"])
    with model.stream_edits(edits):  # and the run is a function of (tokens, seed, edits)
        assert torch.equal(model.gibbs_sample(toks, 2, per_step=3, seed=S.SEED), final)


# ---- 7. the two-stream window ------------------------------------------------------------------------------------------------
def test_an_edited_call_runs_on_one_stream(monkeypatch):
    model = esm.ESM2(2, 128, 2).eval()
    model.load_state_dict(synth_esm2_state_dict(2, 128, 2, seed=3))
    model = model.cuda()
    toks = synth_tokens(4, 1020, seed=5).cuda()  # 4 x 1022 = 4088 rows: inside the first window of the dual-stream forward
    edits = [StreamEdit(1, "add", torch.ones(128), gain=0.5, positions="residues"),
             StreamEdit(2, "zero", positions=torch.tensor([[3, 1021], [0, 5]]))]  # a row of the second half-batch among them
    monkeypatch.delenv("ESM_AMD_DUAL_STREAM", raising=False)
    model(toks)                 # the first call of a length runs on one stream
    base = model(toks)["logits"]
    eng = model._engine
    assert eng.dual_calls == 1  # the plain forward splits this batch over two streams
    one = model.forward_edited(toks, edits)["logits"]
    assert eng.dual_calls == 1
    monkeypatch.setenv("ESM_AMD_DUAL_STREAM", "0")
    assert torch.equal(model.forward_edited(toks, edits)["logits"], one)
    assert torch.equal(model(toks)["logits"], base) and not torch.equal(one, base)
    assert not torch.equal(one[3, 1021], base[3, 1021])  # the listed row of the second half-batch was edited


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    model, toks = model_of("esm2"), batch().cuda()
    edits = steer(128)
    with model.stream_edits(edits):
        for call in (lambda: model.wt_marginals(toks, varlen=True), lambda: model.masked_marginals(toks, varlen=True),
                     lambda: model.forward_varlen(toks), lambda: model.masked_marginals(toks, window=32),
                     lambda: model.forward_windows(toks, window=32),
                     lambda: scoring.wt_marginals(model, toks, varlen=True)):  # past the methods: the engine's own refusal
            with pytest.raises(ValueError, match="not built"):
                call()
        same(model(toks), model.forward_edited(toks, edits), "the padded path inside and forward_edited")
    model.forward_varlen(toks)  # outside the context these run again
    with pytest.raises(ValueError, match="token-set edits only"):
        with model.stream_edits([StreamEdit(1, "zero", positions=torch.tensor([[0, 1]]))]):
            pass
    for k in (-1, L + 1):
        with pytest.raises(ValueError, match="outside 0 .. 3"):
            model.forward_edited(toks, [StreamEdit(k, "zero")])
    with pytest.raises(NotImplementedError):
        args = argparse.Namespace(layers=1, embed_dim=128, ffn_embed_dim=512, attention_heads=2, max_positions=64,
                                  max_tokens_per_msa=2 ** 14, embed_positions_msa=True, dropout=0.0, attention_dropout=0.0,
                                  activation_dropout=0.0)
        esm.MSATransformer(args, esm.Alphabet.from_architecture("msa_transformer")).stream_edits(edits)
    assert model._engine.edits is None


def test_mean_difference_is_the_difference_of_the_masked_means():
    import esm_amd

    model = model_of("esm2")
    a, b = batch(seed=12), batch(seed=31)
    got = esm_amd.mean_difference(model, a.cuda(), b.cuda(), 2)
    assert got.dtype == torch.float32 and tuple(got.shape) == (128,)

    def mean_of(toks):
        rep = model(toks.cuda(), repr_layers=[2])["representations"][2].double().cpu()
        keep = toks.ne(1) & toks.ne(0) & toks.ne(2)
        return rep[keep].mean(0)

    want = mean_of(a) - mean_of(b)
    assert (got.double().cpu() - want).abs().max() <= 1e-5 * max(mean_of(a).abs().max(), mean_of(b).abs().max())
