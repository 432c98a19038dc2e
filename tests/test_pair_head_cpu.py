"""The pairwise head without a GPU: the fp64 restatement (tests/_pair_head_ref.py) against what the REFERENCE's
LinearProjectionDistogramModel computed (tests/golden/pair_head_lmdesign.pt, written by tests/golden/make_golden_pair_head.py),
the distance binning against recorded ``np.digitize`` results, the checkpoint loader on a file the test writes, the energy
restatement against get_cce_loss' formula written out pair by pair, every refusal (Python and, on fake pointers, the C ABI: none
of those calls reaches the HIP runtime), and the mutation knobs of the restatement against its own bound."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _pair_head_ref as R
from esm_amd import PairHead, distogram_bins, distogram_from_pdb, _native as N
from esm_amd import pair_head as PH
from esm_amd.synth import synth_esm2_state_dict
from oracle.esm2_oracle import esm2_forward

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "pair_head_lmdesign.pt")
FAKE = ctypes.c_void_p(0x1000)


def err():
    return N.lib.esmk_last_error().decode()


def conv_state(C, seed):
    """The two convolutions in the layout of lm-design's checkpoint, from one seeded generator, at the scale nn.Conv2d constructs
    them at (uniform within 1 / sqrt(C), what LinearProjectionDistogramModel() holds before training).  The scale matters to the
    pin: the head sums C = 660 channels, so weights of order 1 would amplify the fp32 rounding of the CPU oracle's attention maps
    by about sqrt(660) and the 2e-5 of tests/test_oracle.py, set for the oracle's own outputs, would measure the host's BLAS."""
    g = torch.Generator().manual_seed(seed)
    a = 1.0 / C ** 0.5

    def u(*shape):
        return (torch.rand(*shape, generator=g) * 2 - 1) * a

    return {"conv1.weight": u(36, C, 1, 1), "conv1.bias": u(36), "conv2.weight": u(26, C, 1, 1), "conv2.bias": u(26)}


# ---- 1. the reference pin ----------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference():
    fix = torch.load(GOLDEN, weights_only=True)
    d = fix["dims"]
    L, E, H = d["L"], d["E"], d["H"]
    sd = synth_esm2_state_dict(L, E, H, seed=fix["model_seed"])
    attn = esm2_forward(sd, fix["tokens"], L, H, need_head_weights=True)["attentions"]  # [B,L,H,T,T]
    head = PairHead.from_linear_projection({"model": conv_state(L * H, fix["conv_seed"])})
    z, _ = R.pair_head_on_maps(attn, head.matrix(), head.bias(), head.n_sym)
    for name, key in (("dist", "logits"), ("omega", "omega_logits"), ("theta", "theta_logits"), ("phi", "phi_logits")):
        lo, hi = head.columns(name)
        want = fix[key].permute(0, 2, 3, 1).double()  # [B, n, S, S] -> [B, S, S, n]
        assert want.shape == z[..., lo:hi].shape
        assert (z[..., lo:hi] - want).abs().max().item() < 2e-5, name  # tests/test_oracle.py's bound


# ---- 2. the binning ----------------------------------------------------------------------------------------------------------
def test_distogram_bins_recorded_cases():
    # np.digitize(d, np.linspace(2.5, 20, 17)) recorded at and around the edges 2.5, 3.59375, ..., 18.90625, 20
    d = np.array([[0.0, 2.4999, 2.5, 3.59374], [3.59375, 7.9, 8.0, 18.90624], [18.90625, 19.999, 20.0, 1e9],
                  [float("nan"), float("inf"), 7.96875, 7.968749]])
    want = np.array([[0, 0, 1, 1], [2, 5, 6, 15], [16, 16, 17, 17], [255, 17, 6, 5]], dtype=np.uint8)
    got = distogram_bins(d)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(distogram_bins(torch.tensor(d)), want)
    assert np.array_equal(distogram_bins(np.array([[1.0, 5.0, 9.0]]), d_min=2.0, d_max=8.0, n_bins=4), [[0, 2, 3]])
    with pytest.raises(ValueError, match="n_bins"):
        distogram_bins(d, n_bins=1)


def test_distogram_from_pdb(tmp_path):
    def atom(i, name, res, x):
        return f"ATOM  {i:5d} {name:<4s} {res} A{i:4d}    {x:8.3f}{0.0:8.3f}{0.0:8.3f}  1.00  0.00\n"

    p = tmp_path / "x.pdb"
    p.write_text(atom(1, " CB", "ALA", 0.0) + atom(2, " CA", "GLY", 3.0) + atom(3, " CA", "SER", 9.0) + atom(4, " CB", "LEU", 30.0))
    seq, bins = distogram_from_pdb(str(p))
    assert seq == "AGSL"
    want = distogram_bins(np.array([[0.0, 3.0, np.nan, 30.0], [3.0, 0.0, np.nan, 27.0], [np.nan] * 4, [30.0, 27.0, np.nan, 0.0]]))
    assert np.array_equal(bins, want) and (bins[2] == 255).all() and bins[0, 3] == 17


# ---- 3. the checkpoint loader --------------------------------------------------------------------------------------------------
class _Dims:
    def __init__(self, L, H):
        self.num_layers, self.attention_heads = L, H


def test_from_linear_projection_on_a_written_file(tmp_path):
    state = conv_state(660, seed=5)
    path = tmp_path / "projection.pt"
    torch.save({"model": state, "epoch": 3}, path)
    head = PairHead.from_linear_projection(str(path), _Dims(33, 20))
    assert (head.n_sym, head.n_asym, head.n_out, head.channels) == (36, 26, 62, 660)
    assert [head.columns(n) for n in ("dist", "omega", "theta", "phi")] == [(0, 18), (18, 36), (36, 54), (54, 62)]
    w = head.matrix()
    assert w.shape == (660, 62) and w.dtype == torch.float32 and w.is_contiguous()
    assert torch.equal(w[:, :36], state["conv1.weight"][:, :, 0, 0].t()) and torch.equal(w[:, 36:], state["conv2.weight"][:, :, 0, 0].t())
    assert torch.equal(head.bias(), torch.cat([state["conv1.bias"], state["conv2.bias"]]))
    with pytest.raises(ValueError, match="660 input channels.*6 \\* 20 = 120"):
        PairHead.from_linear_projection(str(path), _Dims(6, 20))
    bad = dict(state)
    del bad["conv2.bias"]
    with pytest.raises(ValueError, match="conv2.bias"):
        PairHead.from_linear_projection(bad)
    bad = dict(state, **{"conv1.weight": state["conv1.weight"][:30]})
    with pytest.raises(ValueError, match=r"\[36, C, 1, 1\]"):
        PairHead.from_linear_projection(bad)


# ---- 4. the energy -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_sep,inv_temp", [(0, 1.0), (4, 0.5)])
def test_energy_restatement_is_get_cce_loss(min_sep, inv_temp):
    g = torch.Generator().manual_seed(3)
    B, S, n = 2, 11, 18
    logits = torch.randn(B, S, S, n, generator=g) * 2
    target = torch.randint(0, n, (S, S), generator=g)
    target[torch.rand(S, S, generator=g) < 0.3] = 255
    e, cnt = R.distogram_energy_ref(logits, target, min_sep, inv_temp)
    # utils/loss.py:10-29 pair by pair: mean over the masked ordered pairs of -log(p[label] + 1e-8)
    for b in range(B):
        tot, k = 0.0, 0
        for i in range(S):
            for j in range(S):
                if target[i, j] == 255 or abs(i - j) < min_sep:
                    continue
                zs = [inv_temp * float(v) for v in logits[b, i, j].double()]
                m = max(zs)
                p = math.exp(zs[int(target[i, j])] - m) / sum(math.exp(v - m) for v in zs)
                tot += -math.log(p + 1e-8)
                k += 1
        assert k == cnt and abs(float(e[b]) - tot / k) <= 1e-12 * abs(tot / k)
    e0, c0 = R.distogram_energy_ref(logits, torch.full((S, S), 255), 0, 1.0)
    assert c0 == 0 and e0.tolist() == [0.0] * B


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_pair_head_construction_refusals():
    w = torch.zeros(40, 12)
    with pytest.raises(ValueError, match="at most 64"):
        PairHead(w, None, torch.zeros(25, 12), None)
    with pytest.raises(ValueError, match="no output"):
        PairHead(None, None, None, None)
    with pytest.raises(ValueError, match="12 channels, w_asym 13"):
        PairHead(w, None, torch.zeros(2, 13), None)
    with pytest.raises(ValueError, match="b_sym has shape"):
        PairHead(w, torch.zeros(3), None, None)
    with pytest.raises(ValueError, match="not a slice"):
        PairHead(w, None, None, None, outputs={"x": ("sym", 0, 41)})
    with pytest.raises(ValueError, match="block must be"):
        PairHead(w, None, None, None, outputs={"x": ("both", 0, 4)})
    head = PairHead(w, None, torch.zeros(24, 12), None, outputs={"a": ("sym", 3, 9), "b": ("asym", 0, 24)})  # 64 outputs: the limit
    assert head.columns("a") == (3, 9) and head.columns("b") == (40, 64)


def test_pair_logits_refusals_by_name():
    from esm_amd.msa_transformer import MSATransformer

    head = PairHead(torch.zeros(2, 4), None, None, None)
    toks = torch.zeros(1, 5, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="MSA Transformer"):
        PH.pair_logits(object.__new__(MSATransformer), toks, head)
    with pytest.raises(NotImplementedError, match="varlen=True"):
        PH.pair_logits(_Dims(1, 4), toks, head, varlen=True)
    with pytest.raises(NotImplementedError, match="window"):
        PH.pair_logits(_Dims(1, 4), toks, head, window=16)
    with pytest.raises(TypeError, match="PairHead"):
        PH.pair_logits(_Dims(1, 4), toks, torch.zeros(4, 2))
    with pytest.raises(ValueError, match="input channels"):
        PH.pair_logits(_Dims(2, 4), toks, head)


def make(L=2, E=128, H=2):
    cfg = N.EsmkConfig(L, E, H, 4 * E, 33, 1, 32, 0, 2, 1, 1, 1, N.dtype_code(torch.float16), 0, 0, 0)
    h = ctypes.c_void_p()
    assert N.lib.esmk_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, err()
    return h


def test_c_abi_refusals():
    h = make()
    n, off = ctypes.c_size_t(), ctypes.c_size_t()
    lib = N.lib
    assert lib.esmk_set_pair_head(None, FAKE, FAKE, 1, 0) != 0 and "null model" in err()
    assert lib.esmk_set_pair_head(h, FAKE, FAKE, 40, 25) != 0 and "0 (clear) .. 64" in err()
    assert lib.esmk_set_pair_head(h, FAKE, FAKE, -1, 2) != 0 and "must not be negative" in err()
    assert lib.esmk_set_pair_head(h, None, FAKE, 1, 0) != 0 and "null weight or bias" in err()
    assert lib.esmk_set_pair_head(h, FAKE, None, 0, 1) != 0 and "null weight or bias" in err()
    assert lib.esmk_set_pair_head(h, None, None, 0, 0) == 0, err()  # clear
    # no head on the handle: the forward and its workspace query refuse
    assert lib.esmk_rows_pair_workspace_bytes(h, 1, 20, 0, ctypes.byref(n), ctypes.byref(off)) != 0 and "no pairwise head is set" in err()
    assert lib.esmk_forward_rows_pair(h, FAKE, FAKE, 1, 20, None, 0, None, FAKE, FAKE, 1 << 40, None) != 0
    assert "no pairwise head is set" in err()
    assert lib.esmk_forward_rows_pair(h, FAKE, FAKE, 1, 20, None, 0, None, None, FAKE, 1 << 40, None) != 0 and "null argument" in err()
    lib.esmk_destroy(h)
    mcfg = N.EsmkMsaConfig(1, 128, 2, 512, 33, 1, 32, 0, 2, 1, 0, 64, 1, N.dtype_code(torch.float16), 0)
    m = ctypes.c_void_p()
    assert lib.esmk_msa_create(ctypes.byref(mcfg), ctypes.byref(m)) == 0, err()
    assert lib.esmk_set_pair_head(m, FAKE, FAKE, 1, 0) != 0 and "MSA handle" in err()
    lib.esmk_destroy(m)
    # the single ops
    args = dict(B=1, H=2, T=20, L=2, D=64)

    def op(n_sym=3, n_asym=2, q=FAKE, ws=1 << 20, dt=N.F16, **kw):
        a = dict(args, **kw)
        return lib.esmk_op_pair_head(q, FAKE, FAKE, None, None, FAKE, None, n_sym, n_asym, FAKE, FAKE, ws, a["B"], a["H"], a["T"],
                                     a["L"], a["D"], 1, 1, 1, dt, None)

    assert op(q=None) != 0 and "null argument" in err()
    assert op(dt=N.F32) != 0 and "fp16 or bf16" in err()
    assert op(n_sym=40, n_asym=25) != 0 and "1 .. 64" in err()
    assert op(n_sym=0, n_asym=0) != 0 and "1 .. 64" in err()
    assert op(D=32) != 0 and "head_dim must be 64 or 128" in err()
    assert op(T=2) != 0 and "no pair map" in err()
    assert op(B=1 << 14, T=1 << 11) != 0 and "2^24" in err()
    assert op(ws=100) != 0 and "workspace too small" in err()
    assert lib.esmk_op_pair_head_workspace_bytes(2, 2, ctypes.byref(n)) == 0 and n.value == 4 * 64 * 4
    assert lib.esmk_op_pair_head_workspace_bytes(0, 2, ctypes.byref(n)) != 0

    def en(logits=FAKE, ld=62, first=0, n_bins=18, B=1, S=8, min_sep=0, inv_temp=1.0):
        return lib.esmk_op_distogram_energy(logits, ld, first, n_bins, FAKE, B, S, min_sep, inv_temp, FAKE, FAKE, None)

    assert en(logits=None) != 0 and "null argument" in err()
    assert en(S=0) != 0 and "positive" in err()
    assert en(S=40000) != 0 and "32768" in err()
    assert en(n_bins=256, ld=300) != 0 and "1 .. 255" in err()
    assert en(first=50) != 0 and "inside the ld outputs" in err()
    assert en(min_sep=-1) != 0 and "min_sep" in err()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert en(inv_temp=bad) != 0 and "inv_temp" in err()


# ---- 6. the bound discriminates ------------------------------------------------------------------------------------------------
def test_every_mutation_breaks_the_bound():
    g = torch.Generator().manual_seed(1)
    L, B, H, T, D, n_sym, n_asym = 3, 2, 4, 21, 64, 6, 5
    q = torch.randn(L, B, H, T, D, generator=g) * 0.6
    k = torch.randn(L, B, H, T, D, generator=g) * 0.6
    w = torch.randn(L * H, n_sym + n_asym, generator=g)
    bias = torch.randn(n_sym + n_asym, generator=g)
    tok = torch.randint(4, 24, (B, T), generator=g)
    tok[1, 15:] = 1
    ref = R.pair_head_ref(q, k, w, bias, n_sym, tokens=tok)
    # the unmutated restatement holds the bound: against itself on fp32-rounded operands of the last step, and on the maps
    maps = torch.stack([torch.stack([torch.softmax(
        (q[l, b].double() @ k[l, b].double().transpose(-1, -2)).masked_fill(tok[b].eq(1)[None, None, :], float("-inf")), -1)
        for l in range(L)]) for b in range(B)])  # [B,L,H,T,T]
    keep = tok.ne(1).double()
    maps = maps * keep[:, None, None, :, None] * keep[:, None, None, None, :]
    z, _ = R.pair_head_on_maps(maps, w, bias, n_sym)
    assert ((z - ref.z).abs() / ref.tol()).max().item() <= 1.0
    assert ((z.float().double() - ref.z).abs() / ref.tol()).max().item() <= 1.0
    for name, kw in (("drop a channel", dict(drop=[(1, 2)])), ("shift the layer's weights", dict(w_layer_shift=1)),
                     ("swap the blocks", dict(swap_blocks=True)), ("no transpose term", dict(no_transpose=True))):
        mut = R.pair_head_ref(q, k, w, bias, n_sym, tokens=tok, **kw)
        assert R.discrimination(ref, mut) > 10, name
        zm, _ = R.pair_head_on_maps(maps, w, bias, n_sym, **kw)
        assert ((zm - mut.z).abs() / ref.tol()).max().item() <= 1.0, name  # both restatements mutate alike
