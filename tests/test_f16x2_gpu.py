"""The split-weight precision mode (ESM_AMD_OPERAND=f16x2, esmk_config.weight_split): every matrix of the layer stack
is kept as W = W_hi + W_lo (two fp16 images) and each layer GEMM runs over both — the weight rounding, two thirds of
the fp16-operand error of a deep stack, disappears at 2x the GEMM time.

    * the split GEMM as a single op against fp64 (error ~1e-6 relative instead of ~2e-4);
    * the 650M-dimension model against the fp32 oracle: representations, logits and raw token argmax inside 1e-3
      (reference tolerance: tests/test_readme.py:116 atol=1e-3; north star: "token argmax bit-exact").
"""
import math

import pytest
import torch

import esm
from esm_amd import _native as nat
from esm_amd import ops
from esm_amd.synth import skip_param_init, synth_esm2_state_dict, synth_tokens
from oracle.esm2_oracle import esm2_forward

pytestmark = pytest.mark.gpu

SPLIT_STORE_T_TOL = 6e-4  # linear_split, operand-dtype store: the fp16 output rounding itself, relative to the largest value
SPLIT_GELU_TOL = 1e-3     # linear_split, GELU epilogue, relative to the largest value


@pytest.mark.parametrize("M,N,K", [(512, 256, 64), (1000, 1288, 320), (4096, 1280, 1280)])
def test_linear_split_matches_fp64(M, N, K):
    g = torch.Generator(device="cuda").manual_seed(3)
    a = torch.randn(M, K, device="cuda", generator=g).half()
    w = torch.randn(N, K, device="cuda", generator=g) / math.sqrt(K)
    bias = torch.randn(N, device="cuda", generator=g)
    w2 = ops.split_weight(w)
    # the image itself: hi + lo reproduces w to ~2^-19 of the weight scale
    hi = w2.view(N, K // 64, 2, 64)[:, :, 0].reshape(N, K).float()
    lo = w2.view(N, K // 64, 2, 64)[:, :, 1].reshape(N, K).float()
    assert torch.equal(hi, w.half().float())
    assert ((hi + lo) - w).abs().max().item() < 2.0 ** -18 * w.abs().max().item()
    ref = a.double() @ w.double().t() + bias.double()
    scale = ref.abs().max().item()
    for epi in (nat.EPI_STORE_F32, nat.EPI_STORE_T, nat.EPI_RESID_F32):
        x0 = torch.zeros(M, N, device="cuda") if epi == nat.EPI_RESID_F32 else None
        got = ops.linear_split(a, w2, bias, epi, out=x0).double()
        plain = ops.linear(a, w.half(), bias, epi, out=torch.zeros(M, N, device="cuda") if x0 is not None else None).double()
        e_split, e_plain = (got - ref).abs().max().item() / scale, (plain - ref).abs().max().item() / scale
        print(f"\n({M},{N},{K}) epi {epi}: split {e_split:.2e}, plain fp16 weights {e_plain:.2e}")
        if epi == nat.EPI_STORE_T:
            assert e_split < SPLIT_STORE_T_TOL
        else:
            assert e_split < 1e-5 and e_plain > 8 * e_split, (e_split, e_plain)
    # GELU epilogue against the same function in fp64
    got = ops.linear_split(a, w2, bias, nat.EPI_GELU_T).double()
    want = torch.nn.functional.gelu(ref)
    assert (got - want).abs().max().item() < SPLIT_GELU_TOL * want.abs().max().item()


def test_650m_dims_split_weights_meet_the_contract(monkeypatch):
    L, E, H = 33, 1280, 20
    sd = synth_esm2_state_dict(L, E, H, seed=0)
    toks = synth_tokens(2, 128, seed=100)
    ref = esm2_forward({k: v.float() for k, v in sd.items()}, toks, L, H, repr_layers=[L])
    with skip_param_init():
        model = esm.ESM2(L, E, H).eval()
    model.load_state_dict(sd)
    model = model.cuda()
    out = {}
    for mode in ("f16", "f16x2"):
        monkeypatch.setenv("ESM_AMD_OPERAND", mode)
        with torch.no_grad():
            o = model(toks.cuda(), repr_layers=[L])
        r, rr = o["representations"][L].double().cpu(), ref["representations"][L].double()
        lg, lgr = o["logits"].double().cpu(), ref["logits"].double()
        out[mode] = dict(repr_max=((r - rr).abs().max() / rr.abs().max()).item(), repr_l2=((r - rr).norm() / rr.norm()).item(),
                         logits=((lg - lgr).abs().max() / lgr.abs().max()).item(),
                         argmax=(lg.argmax(-1) == lgr.argmax(-1)).float().mean().item())
        print(f"\n650M dims {mode}: {out[mode]}")
    monkeypatch.delenv("ESM_AMD_OPERAND")
    s = out["f16x2"]
    # emulated floor of the mode on these inputs (oracle, weights exact): 6.2e-4 max / 4.9e-4 L2, logits 8.5e-4
    assert s["repr_max"] < 8e-4 and s["repr_l2"] < 6.5e-4, s
    assert s["logits"] < 1e-3, s
    assert s["argmax"] == 1.0, s
    assert s["repr_l2"] < 0.7 * out["f16"]["repr_l2"], out


@pytest.mark.parametrize("mode,sites,b_l2,b_mx", [("f16x2a", ("W!qk", "W!v", "W!o"), 7.2e-4, 8.5e-4), ("f16x2v", ("W!v", "W!o"), 7.6e-4, 9.0e-4)])
def test_650m_dims_attention_split_mode(monkeypatch, mode, sites, b_l2, b_mx):
    """ESM_AMD_OPERAND=f16x2a (esmk_config.weight_split = 2, round 6): split weights on the ATTENTION projections only (q, k,
    v, out — a third of the GEMM work; the feed-forward matrices stay plain fp16, the LM head runs in fp32 as in f16x2);
    f16x2v (weight_split = 3): the value path only (v, out — a sixth of the GEMM work).
    Against the fp32 oracle and against the floor of exactly this form (weights exact at those sites): the engine is on
    its floor (the ONE contract, L2 slack 1.10), the representation is inside 1e-3 with 25 - 30 % margin in both norms (plain
    mode: 3 - 5 %), the logits inside 1e-3 in L2."""
    import _contract as C
    from oracle.esm2_oracle import ALL_OPERANDS

    L, E, H = 33, 1280, 20
    sd = synth_esm2_state_dict(L, E, H, seed=0)
    sd32 = {k: v.float() for k, v in sd.items()}
    toks = synth_tokens(2, 128, seed=100)
    ref = esm2_forward(sd32, toks, L, H, repr_layers=[L])
    floor = esm2_forward(sd32, toks, L, H, repr_layers=[L], inject=(frozenset(ALL_OPERANDS + sites), torch.float16),
                         inject_head=None)
    with skip_param_init():
        model = esm.ESM2(L, E, H).eval()
    model.load_state_dict(sd)
    model = model.cuda()
    monkeypatch.setenv("ESM_AMD_OPERAND", mode)
    with torch.no_grad():
        o = model(toks.cuda(), repr_layers=[L])
        pk = model.forward_varlen(toks.cuda(), repr_layers=[L], min_saving=None)
    monkeypatch.delenv("ESM_AMD_OPERAND")
    assert model.ln_fold_active() is False  # split weights run the plain LayerNorm path
    l2, mx = C.check_tensors(f"650M-dims {mode} repr", o["representations"][L].cpu(), ref["representations"][L], floor["representations"][L],
                             hard_l2=True)
    assert l2 < b_l2 and mx < b_mx, (l2, mx)   # f16x2a measured 6.39e-4 / 6.98e-4 (floor of the form 6.40e-4 / 7.41e-4; plain mode 8.7e-4 / 9.7e-4)
    l2, mx = C.check_tensors(f"650M-dims {mode} logits", o["logits"].cpu(), ref["logits"], floor["logits"], deep=True)
    assert l2 < 1e-3, (l2, mx)                 # f16x2a measured 8.26e-4 / 9.60e-4 (plain mode: 1.19e-3 / 1.28e-3)
    C.check_raw_argmax(f"650M-dims {mode} token argmax", C.raw_argmax_agreement(o["logits"], ref["logits"]),
                       C.raw_argmax_agreement(floor["logits"], ref["logits"]))
    # the token-packed forward runs the same kernels: same bits
    assert torch.equal(pk["representations"][L], o["representations"][L]) and torch.equal(pk["logits"], o["logits"])


def test_650m_dims_f16x3_weights_and_activations_split(monkeypatch):
    """ESM_AMD_OPERAND=f16x3 (esmk_config.weight_split = 4, round 6): every layer GEMM as a plain launch over K' = 3 K — weight
    images hi | lo | hi per K tile against operand rows hi | hi | lo (LayerNorm output and fc1's GELU output in fp32 ->
    split3_rows_kernel; the attention kernel's X3 output) = A_hi W_hi + A_hi W_lo + A_lo W_hi; fp32 LM head.  What is still
    rounded to fp16: q / k, v and P inside the attention.  The engine sits on the floor of exactly that form and every output is
    inside 1e-3 with >= 2 x margin on representations and logits (contact logits: the full-size 3B test)."""
    import _contract as C

    L, E, H = 33, 1280, 20
    sd = synth_esm2_state_dict(L, E, H, seed=0)
    sd32 = {k: v.float() for k, v in sd.items()}
    toks = synth_tokens(2, 128, seed=100)
    toks[1, 90] = 2
    toks[1, 91:] = 1
    nonpad = toks.ne(1)
    ref = esm2_forward(sd32, toks, L, H, repr_layers=[L], return_contacts=True)
    floor = esm2_forward(sd32, toks, L, H, repr_layers=[L], return_contacts=True, inject=(frozenset({"QK", "V", "P"}), torch.float16),
                         inject_head=None)
    with skip_param_init():
        model = esm.ESM2(L, E, H).eval()
    model.load_state_dict(sd)
    model = model.cuda()
    monkeypatch.setenv("ESM_AMD_OPERAND", "f16x3")
    with torch.no_grad():
        o = model(toks.cuda(), repr_layers=[L], return_contacts=True)
        fused = model.predict_contacts(toks.cuda())
        pk = model.forward_varlen(toks.cuda(), repr_layers=[L], min_saving=None)  # no packed form in this mode: the padded forward
    monkeypatch.delenv("ESM_AMD_OPERAND")
    l2, mx = C.check_tensors("650M-dims f16x3 repr", o["representations"][L].cpu(), ref["representations"][L], floor["representations"][L],
                             nonpad, hard_l2=True)
    assert l2 < 4.5e-4 and mx < 5.5e-4, (l2, mx)
    l2, mx = C.check_tensors("650M-dims f16x3 logits", o["logits"].cpu(), ref["logits"], floor["logits"], nonpad, deep=True)
    assert l2 < 6e-4 and mx < 8e-4, (l2, mx)
    C.check_raw_argmax("650M-dims f16x3 token argmax", C.raw_argmax_agreement(o["logits"], ref["logits"], nonpad),
                       C.raw_argmax_agreement(floor["logits"], ref["logits"], nonpad))
    for b, n in ((0, 128), (1, 89)):
        _, zrel = C.contact_logit_errors(o["contacts"][b, :n, :n], ref["contacts"][b, :n, :n])
        _, zfl = C.contact_logit_errors(floor["contacts"][b, :n, :n], ref["contacts"][b, :n, :n])
        C.check(f"650M-dims f16x3 contact logits seq {b}", zrel, zrel, zfl, zfl, slack=C.CONTACT_SLACK, slack_l2=C.CONTACT_SLACK)
        assert (fused[b, :n, :n].cpu() - o["contacts"][b, :n, :n].cpu()).abs().max().item() < 1e-4
    assert torch.equal(pk["representations"][L][nonpad.cuda()], o["representations"][L][nonpad.cuda()])
