"""Edits of the residual stream without a GPU: the numpy reference of the kernel against rows computed by hand, the decided
rule on the committed inputs (no projected row of the GPU tests' inputs is undecided), the normalisation of ``StreamEdit`` and
its errors, and every host-side refusal of ``esmk_set_stream_edits`` / ``esmk_op_stream_edit`` / the token-packed entries on
fake pointers (as tests/test_c_abi_validation_cpu.py does: none of these calls reaches the HIP runtime)."""
import ctypes

import numpy as np
import pytest
import torch

import _stream_edit_ref as R
import esm
from esm_amd import StreamEdit, _native as N
from esm_amd.interventions import plan_edits, token_set
from esm_amd.synth import synth_esm2_state_dict, synth_tokens

FAKE = ctypes.c_void_p(0x1000)
f32 = np.float32


def err():
    return N.lib.esmk_last_error().decode()


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_axpby_by_hand():
    x = np.array([[1.0, 2.0, 3.0, 4.0], [0.1, 0.2, 0.3, 0.4]], dtype=f32)
    s = np.array([[0.5, -1.0, 0.25, 8.0], [1.0, 1.0, 1.0, 1.0]], dtype=f32)
    got = R.axpby_rows(x, s, 0.5, 2.0)
    assert np.array_equal(got[0], np.array([1.5, -1.0, 2.0, 18.0], dtype=f32))
    # every operation rounded on its own: 0.1f * 0.5 and 2 are exact scalings, so the sum is float32(0.05f + 2)
    assert got[1, 0] == f32(f32(f32(0.1) * f32(0.5)) + f32(2.0))
    # a fused multiply-add would give another last bit here: keep * x is inexact, then added
    a, k, g, b = f32(1 + 2.0 ** -12), f32(1 + 2.0 ** -12), f32(1.0), f32(-1.0)  # k a = 1 + 2^-11 + 2^-24: a tie, rounded away
    unfused = f32(f32(k * a) + f32(g * b))
    fused = f32(np.float64(k) * np.float64(a) + np.float64(g) * np.float64(b))
    assert unfused == f32(2.0 ** -11) and fused == f32(2.0 ** -11 + 2.0 ** -24)
    assert R.axpby_rows(np.array([[a]], dtype=f32), np.array([[b]], dtype=f32), k, g)[0, 0] == unfused
    assert np.array_equal(R.axpby_rows(x, None, 0.0, 0.0), np.zeros_like(x))          # zero
    assert np.array_equal(R.axpby_rows(x, s, 0.0, 1.0), s)                             # set
    assert np.array_equal(R.axpby_rows(x, None, 1.0, 0.0), x)                          # the identity edit


def test_project_by_hand():
    x = np.array([[3.0, 4.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0], [5.0, 6.0, 7.0, 8.0]], dtype=f32)
    s = np.array([[1.0, 0.0, 0.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, 0.0, 0.0, 0.0]], dtype=f32)
    out, c, changed = R.project_rows(x, s, 1.0)
    assert c.tolist() == [3.0, 0.5, 0.0] and changed.tolist() == [True, True, False]
    assert np.array_equal(out, np.array([[0, 4, 0, 0], [0, 0, 0, 0], [5, 6, 7, 8]], dtype=f32))  # <s, s> = 0: the row stays
    out2, c2, _ = R.project_rows(x[:1], s[:1], 0.5)
    assert c2[0] == 1.5 and out2[0, 0] == 1.5


def test_decided_rule():
    one = np.float64(1.0)
    edge = one + np.float64(2.0 ** -24)  # half way between 1 and the next float32
    assert R.decided(one) and R.decided(one + 0.3 * 2.0 ** -23)
    assert not R.decided(edge) and not R.decided(edge * (1 + 5e-10)) and not R.decided(edge * (1 - 5e-10))
    assert R.decided(edge * (1 + 2e-9)) and R.decided(edge * (1 - 2e-9))
    assert not R.decided(one - 2.0 ** -25)  # below a power of two the spacing halves: this IS the boundary under 1
    # 1e-9 of c against a spacing of 6e-8 .. 1.2e-7 of c: 1.7 - 3.3 % of random coefficients are undecided, so the inputs of
    # the bit-for-bit tests are chosen (R.OPS_SEEDS) and the tests below hold that none of their rows is


def test_selection_and_sources():
    x, src, vec, index = R.ops_inputs(96)
    rows = np.array(R.OPS_ROW_LISTS[2])
    edit = dict(op=R.AXPBY, keep=0.0, gain=1.0, rows=rows, token_set=0, src=src, src_index=index)
    out, edited, _ = R.apply_edit(x, R.OPS_TOKENS, edit)
    assert edited.tolist() == [0, 8, 3, 5, 2]                      # -1 and N are skipped
    assert np.array_equal(out[[0, 8, 3, 5, 2]], src[[3, 0, 8, 6, 6]])  # their source rows: the index entries of the kept slots
    assert np.array_equal(out[[1, 4, 6, 7]], x[[1, 4, 6, 7]])
    out, edited, _ = R.apply_edit(x, R.OPS_TOKENS, dict(op=R.AXPBY, keep=1.0, gain=2.0, rows=None, token_set=R.OPS_TOKEN_SET, src=vec,
                                                        src_index=None))
    assert edited.tolist() == [1, 2, 6]                            # residues: not <cls>, <pad>, <mask>, <eos>
    assert np.array_equal(out[1], (x[1] + (f32(2.0) * vec).astype(f32)).astype(f32))


@pytest.mark.parametrize("E,ldy", R.OPS_SIZES)
def test_no_projected_row_of_the_op_inputs_is_undecided(E, ldy):
    x, src, vec, index = R.ops_inputs(E)
    assert R.undecided_op_rows(E) == 0


def contract_case(E=128, H=2, L=3):
    """The model, batch and edits of the contract test (tests/test_stream_edit_gpu.py), on the host."""
    sd = synth_esm2_state_dict(L, E, H, seed=11)
    toks = synth_tokens(3, 39, seed=12)
    toks[1, 30] = 2
    toks[1, 31:] = 1
    g = torch.Generator().manual_seed(13)
    direction = torch.randn(E, generator=g)
    direction = direction / direction.norm() * (E ** 0.5) * 0.1  # about the row norm of the synthetic models' early stream
    patch = torch.randn(5, E, generator=g) * 0.1
    listed = torch.tensor([[0, 0], [0, 7], [1, 30], [2, 40], [2, 13]])
    edits = [StreamEdit(1, "add", direction, positions="residues"), StreamEdit(2, "set", patch, positions=listed),
             StreamEdit(L, "project", torch.randn(E, generator=g), positions="all")]
    return sd, toks, edits


def test_reference_forward_with_the_contract_edits():
    for E, H in ((128, 2), (96, 6)):
        sd, toks, edits = contract_case(E, H)
        model = esm.ESM2(3, E, H)
        und = []
        out = R.forward_edited_ref(sd, toks, 3, H, edits=plan_edits(model, edits, *toks.shape), repr_layers=[0, 1, 2, 3], undecided=und)
        assert len(und) == 3 and und[:2] == [0, 0] and torch.isfinite(out["logits"]).all()
        plain = R.forward_edited_ref(sd, toks, 3, H, repr_layers=[1])
        assert not torch.equal(plain["representations"][1], out["representations"][1])  # representation k shows the edit


def test_reference_forward_without_edits_is_the_oracle():
    from oracle.esm2_oracle import ALL_OPERANDS, esm2_forward

    sd, toks, _ = contract_case()
    for inject in (None, (frozenset(ALL_OPERANDS), torch.float16), (frozenset(ALL_OPERANDS + ("FOLD",)), torch.float16)):
        a = R.forward_edited_ref(sd, toks, 3, 2, repr_layers=[0, 2, 3], inject=inject)
        b = esm2_forward(sd, toks, 3, 2, repr_layers=[0, 2, 3], inject=inject)
        assert torch.equal(a["logits"], b["logits"])
        assert all(torch.equal(a["representations"][k], b["representations"][k]) for k in (0, 2, 3))


# ---- StreamEdit -------------------------------------------------------------------------------------------------------------
def test_token_sets_and_coefficients():
    model = esm.ESM2(2, 64, 2)
    assert token_set(model, "all") == (1 << 33) - 1 - (1 << 1)
    assert token_set(model, "residues") == R.OPS_TOKEN_SET
    vec = torch.ones(64)
    want = {"add": (N.EDIT_AXPBY, 1.0, 2.5), "set": (N.EDIT_AXPBY, 0.0, 2.5), "scale": (N.EDIT_AXPBY, 2.5, 0.0),
            "zero": (N.EDIT_AXPBY, 0.0, 0.0), "project": (N.EDIT_PROJECT, 1.0, 2.5)}
    for op, (code, keep, gain) in want.items():
        p = StreamEdit(1, op, vec if op in ("add", "set", "project") else None, gain=2.5).plan(model)
        assert (p["op"], p["keep"], p["gain"]) == (code, keep, gain) and p["rows"] is None and p["token_set"] == token_set(model, "all")


def test_row_lists_and_values():
    model = esm.ESM2(2, 64, 2)
    mask = torch.zeros(2, 5, dtype=torch.bool)
    mask[0, 1] = mask[1, 4] = mask[1, 0] = True
    p = StreamEdit(0, "zero", positions=mask).plan(model, 2, 5)
    assert p["rows"].tolist() == [1, 5, 9] and p["rows"].dtype == torch.int32 and p["src"] is None
    idx = torch.tensor([[1, 4], [0, 0]])
    p = StreamEdit(2, "set", torch.zeros(2, 64), positions=idx).plan(model, 2, 5)
    assert p["rows"].tolist() == [9, 0] and tuple(p["src"].shape) == (2, 64) and p["src_index"] is None
    p = StreamEdit(2, "set", torch.zeros(2, 5, 64), positions=idx).plan(model, 2, 5)
    assert tuple(p["src"].shape) == (10, 64) and p["src_index"].tolist() == [9, 0]
    p = StreamEdit(1, "set", torch.zeros(2, 5, 64), positions="all").plan(model, 2, 5)
    assert p["rows"] is None and p["src_index"] is None and tuple(p["src"].shape) == (10, 64)


def test_normalisation_errors():
    model = esm.ESM2(2, 64, 2)
    vec = torch.zeros(64)
    bad = [
        (lambda: StreamEdit(1, "nudge", vec), "op must be"),
        (lambda: StreamEdit(1, "add"), "needs a value"),
        (lambda: StreamEdit(1, "zero", vec), "takes no value"),
        (lambda: StreamEdit(1, "add", torch.zeros(1, 1, 1, 64)), "shape [E], [n, E] or [B, T, E]"),
        (lambda: StreamEdit(1, "add", vec, positions="everything"), "positions must be"),
        (lambda: StreamEdit(1, "add", vec, positions=torch.zeros(3, 3, dtype=torch.int64)), "positions must be"),
        (lambda: StreamEdit(3, "zero").plan(model), "outside 0 .. 2"),
        (lambda: StreamEdit(-1, "zero").plan(model), "outside 0 .. 2"),
        (lambda: StreamEdit(1, "add", torch.zeros(32)).plan(model), "embed_dim is 64"),
        (lambda: StreamEdit(1, "zero", positions=torch.tensor([[0, 1], [1, 2], [0, 1]])).plan(model, 2, 5), "listed twice"),
        (lambda: StreamEdit(1, "zero", positions=torch.tensor([[2, 1]])).plan(model, 2, 5), "outside the batch"),
        (lambda: StreamEdit(1, "zero", positions=torch.zeros(2, 4, dtype=torch.bool)).plan(model, 2, 5), "positions mask"),
        (lambda: StreamEdit(1, "add", torch.zeros(3, 64), positions=torch.tensor([[0, 1]])).plan(model, 2, 5), "positions select 1"),
        (lambda: StreamEdit(1, "add", torch.zeros(3, 64)).plan(model, 2, 5), "goes with a row list"),
        (lambda: StreamEdit(1, "add", torch.zeros(2, 4, 64)).plan(model, 2, 5), "the batch is (2, 5)"),
        # inside model.stream_edits (no batch shape): token sets with one vector only
        (lambda: model.stream_edits([StreamEdit(1, "zero", positions=torch.tensor([[0, 1]]))]), "token-set edits only"),
        (lambda: model.stream_edits([StreamEdit(1, "add", torch.zeros(2, 5, 64))]), "shape [E] only"),
        (lambda: model.stream_edits([StreamEdit(1, "zero")] * 65), "at most 64"),
    ]
    for fn, msg in bad:
        with pytest.raises(ValueError) as e:
            cm = fn()
            if hasattr(cm, "__enter__"):  # the context checks its list when it is entered
                with cm:
                    pass
        assert msg in str(e.value), (msg, str(e.value))
    with pytest.raises(TypeError):
        plan_edits(model, ["add"])


def test_msa_transformer_refuses():
    import argparse

    args = argparse.Namespace(layers=1, embed_dim=64, ffn_embed_dim=256, attention_heads=2, max_positions=64, max_tokens_per_msa=2 ** 14,
                              embed_positions_msa=True, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0)
    msa = esm.MSATransformer(args, esm.Alphabet.from_architecture("msa_transformer"))
    for call in (lambda: msa.stream_edits([StreamEdit(1, "zero")]), lambda: msa.forward_edited(None, [StreamEdit(1, "zero")])):
        with pytest.raises(NotImplementedError):
            call()


# ---- the C ABI, host side only ------------------------------------------------------------------------------------------------
def make(L=2, E=128, H=2):
    cfg = N.EsmkConfig(L, E, H, 4 * E, 33, 1, 32, 0, 2, 1, 1, 1, N.dtype_code(torch.float16), 0, 0, 0)
    h = ctypes.c_void_p()
    assert N.lib.esmk_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    return h


def edit(layer=1, op=N.EDIT_AXPBY, rows=None, n_rows=0, token_set=2, src=None, src_ld=0, n_src=0):
    return N.EsmkStreamEdit(layer, op, 1.0, 1.0, rows, n_rows, token_set, src, src_ld, n_src, None)


def test_set_stream_edits_validation():
    h = make()
    one = lambda **kw: (N.EsmkStreamEdit * 1)(edit(**kw))
    assert N.lib.esmk_set_stream_edits(None, one(), 1) != 0 and "null model" in err()
    assert N.lib.esmk_set_stream_edits(h, None, 1) != 0 and "null edit list" in err()
    assert N.lib.esmk_set_stream_edits(h, one(), -1) != 0 and "0 (clear) .. 64" in err()
    many = (N.EsmkStreamEdit * 65)(*[edit() for _ in range(65)])
    assert N.lib.esmk_set_stream_edits(h, many, 65) != 0 and "0 (clear) .. 64" in err()
    assert N.lib.esmk_set_stream_edits(h, one(layer=3), 1) != 0 and "layer 3 is outside 0 .. 2" in err()
    assert N.lib.esmk_set_stream_edits(h, one(layer=-1), 1) != 0 and "outside 0 .. 2" in err()
    assert N.lib.esmk_set_stream_edits(h, one(op=2), 1) != 0 and "ESMK_EDIT_AXPBY or ESMK_EDIT_PROJECT" in err()
    assert N.lib.esmk_set_stream_edits(h, one(op=N.EDIT_PROJECT), 1) != 0 and "needs src_dev" in err()
    assert N.lib.esmk_set_stream_edits(h, one(src=FAKE, src_ld=64, n_src=4), 1) != 0 and "src_ld must be 0" in err()
    assert N.lib.esmk_set_stream_edits(h, one(src=FAKE, src_ld=130, n_src=4), 1) != 0 and "src_ld must be 0" in err()
    assert N.lib.esmk_set_stream_edits(h, one(src=FAKE, src_ld=128, n_src=0), 1) != 0 and "n_src must be positive" in err()
    assert N.lib.esmk_set_stream_edits(h, one(rows=FAKE, n_rows=-2), 1) != 0 and "n_rows must not be negative" in err()
    bad_second = (N.EsmkStreamEdit * 2)(edit(), edit(layer=9))
    assert N.lib.esmk_set_stream_edits(h, bad_second, 2) != 0 and "edit 1" in err()
    # accepted lists: every layer 0 .. L, both selectors, both source forms; then cleared
    good = (N.EsmkStreamEdit * 4)(edit(layer=0), edit(layer=2, rows=FAKE, n_rows=3), edit(op=N.EDIT_PROJECT, src=FAKE),
                                  edit(src=FAKE, src_ld=128, n_src=7))
    assert N.lib.esmk_set_stream_edits(h, good, 4) == 0, err()
    assert N.lib.esmk_set_stream_edits(h, None, 0) == 0, err()
    N.lib.esmk_destroy(h)
    mcfg = N.EsmkMsaConfig(1, 128, 2, 512, 33, 1, 32, 0, 2, 1, 0, 64, 1, N.dtype_code(torch.float16), 0)
    m = ctypes.c_void_p()
    assert N.lib.esmk_msa_create(ctypes.byref(mcfg), ctypes.byref(m)) == 0, err()
    assert N.lib.esmk_set_stream_edits(m, one(), 1) != 0 and "MSA handle" in err()
    N.lib.esmk_destroy(m)


def test_token_packed_entries_refuse_while_edits_are_set():
    h = make()
    layers = (ctypes.c_int32 * 1)(2)
    outs = (ctypes.c_void_p * 1)(0x2000)
    seg = (ctypes.c_int32 * 4)(0, 20, 32, 5)
    big = ctypes.c_size_t(1 << 40)

    def calls():
        yield "esmk_forward_packed", N.lib.esmk_forward_packed(h, FAKE, FAKE, seg, 2, 128, layers, 1, outs, N.OUT_LOGITS, FAKE, FAKE,
                                                               ctypes.c_size_t(16), None)
        yield "esmk_forward_packed", N.lib.esmk_forward_packed_ex(h, FAKE, FAKE, seg, 2, 128, layers, 1, outs, N.OUT_LOGITS, FAKE, None,
                                                                  FAKE, ctypes.c_size_t(16), None)
        yield "esmk_forward_packed", N.lib.esmk_forward_packed_maps(h, FAKE, FAKE, seg, 2, 128, layers, 1, outs, N.OUT_LOGITS, FAKE,
                                                                    None, 0, None, FAKE, ctypes.c_size_t(16), None)
        yield "esmk_forward_packed_rows", N.lib.esmk_forward_packed_rows(h, FAKE, FAKE, seg, 2, 128, FAKE, 3, FAKE, FAKE, big, None)

    for who, rc in calls():  # no edits: each call gets as far as its workspace / RoPE check
        assert rc != 0 and "stream edits" not in err(), (who, err())
    assert N.lib.esmk_set_stream_edits(h, (N.EsmkStreamEdit * 1)(edit()), 1) == 0, err()
    for who, rc in calls():
        assert rc != 0 and "stream edits are set" in err() and "padded batches only" in err(), (who, err())
    # the padded entries still take the call: it gets as far as the workspace check
    assert N.lib.esmk_forward(h, FAKE, FAKE, 2, 16, layers, 1, outs, N.OUT_LOGITS, FAKE, None, None, FAKE, ctypes.c_size_t(16), None) != 0
    assert "workspace too small" in err()
    assert N.lib.esmk_set_stream_edits(h, None, 0) == 0
    for who, rc in calls():
        assert rc != 0 and "stream edits" not in err(), (who, err())
    N.lib.esmk_destroy(h)


def test_op_stream_edit_validation():
    e = edit()
    call = lambda x=FAKE, tok=FAKE, n=9, E=128, ed=e, y=None, ldy=0, mean=None, rstd=None, dt=N.F16: N.lib.esmk_op_stream_edit(
        x, tok, n, E, ctypes.byref(ed) if ed is not None else None, y, ldy, mean, rstd, dt, None)
    assert call(x=None) != 0 and "null argument" in err()
    assert call(ed=None) != 0 and "null argument" in err()
    assert call(n=0) != 0 and "0 < N" in err()
    assert call(E=130) != 0 and "embed_dim % 4 == 0" in err()
    assert call(E=5124) != 0 and "embed_dim <= 5120" in err()
    assert call(tok=None) != 0 and "needs tokens_dev" in err()
    assert call(ed=edit(op=N.EDIT_PROJECT)) != 0 and "needs src_dev" in err()
    assert call(y=FAKE, ldy=128) != 0 and "together" in err()
    assert call(y=FAKE, ldy=96, mean=FAKE, rstd=FAKE) != 0 and "ldy must be" in err()
    assert call(y=FAKE, ldy=128, mean=FAKE, rstd=FAKE, dt=N.F32) != 0 and "operand_dtype" in err()


# ---- python -m esm_amd.sample --steer ------------------------------------------------------------------------------------------
def test_sample_cli_steer_flags(tmp_path):
    import contextlib

    from esm_amd import sample

    base = ["--model-location", "m", "--sequence", "MKT", "--output", "o.fasta"]
    args = sample.parse_args(base)
    assert args.steer is None and args.steer_layer is None
    assert isinstance(sample.steering(None, args), contextlib.nullcontext)  # without the flags: the calls of before, nothing around them
    for bad in (["--steer", "v.npy"], ["--steer-layer", "1"], ["--steer-gain", "2"]):
        with pytest.raises(SystemExit):
            sample.parse_args(base + bad)
    np.save(tmp_path / "v.npy", np.arange(64, dtype=np.float64))
    args = sample.parse_args(base + ["--steer", str(tmp_path / "v.npy"), "--steer-layer", "1", "--steer-gain", "2.5"])
    seen = []

    class Model:
        def stream_edits(self, edits):
            seen.extend(edits)
            return contextlib.nullcontext()

    sample.steering(Model(), args)
    (e,) = seen
    assert (e.layer, e.op, e.gain, e.positions) == (1, "add", 2.5, "residues")
    assert e.value.dtype == torch.float32 and e.value.tolist() == list(range(64))
