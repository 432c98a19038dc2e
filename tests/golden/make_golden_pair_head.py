"""Record what the REFERENCE's LinearProjectionDistogramModel (examples/lm-design/utils/linear_projection.py:85-135) computes
into tests/golden/pair_head_lmdesign.pt, the fixture tests/test_pair_head_cpu.py pins the fp64 restatement of the head
(tests/_pair_head_ref.py) against.

    python tests/golden/make_golden_pair_head.py <checkout of the reference implementation>

The class hard-codes 20 x 33 attention channels, so the base model is a reference ESM2(33, 320, 20) with the synthetic weights
``synth_esm2_state_dict(33, 320, 20, seed)``; the two convolutions are drawn from a seeded generator.  linear_projection.py
imports ``omegaconf`` for type names only; where the package is not installed an empty stand-in module of that name is
registered before the import.  The fixture holds data only: the seeds, the tokens and the four logits tensors for B = 2 one-hot
sequences of T = 26 tokens without padding (about 0.3 MB)."""
import importlib.util
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "pair_head_lmdesign.pt")
DIMS = dict(L=33, E=320, H=20)
MODEL_SEED, CONV_SEED, TOKEN_SEED, B, T = 31, 32, 33, 2, 26


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


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


def tokens(seed):
    g = torch.Generator().manual_seed(seed)
    toks = torch.randint(4, 24, (B, T), generator=g, dtype=torch.int64)
    toks[:, 0] = 0
    toks[:, -1] = 2
    return toks


def main(reference):
    sys.path.insert(0, reference)  # ``esm`` is the reference here
    try:
        import omegaconf  # noqa: F401
    except ImportError:
        stand_in = types.ModuleType("omegaconf")
        stand_in.DictConfig = stand_in.OmegaConf = object
        sys.modules["omegaconf"] = stand_in
    import esm

    assert os.path.abspath(esm.__file__).startswith(os.path.abspath(reference)), esm.__file__
    synth = load_by_path("_synth", os.path.join(ROOT, "esm_amd", "synth.py"))
    lp = load_by_path("_linear_projection", os.path.join(reference, "examples", "lm-design", "utils", "linear_projection.py"))
    base = esm.model.esm2.ESM2(DIMS["L"], DIMS["E"], DIMS["H"]).eval()
    base.load_state_dict(synth.synth_esm2_state_dict(DIMS["L"], DIMS["E"], DIMS["H"], seed=MODEL_SEED))
    model = lp.LinearProjectionDistogramModel()
    model.base_model = base
    model.load_state_dict(conv_state(DIMS["L"] * DIMS["H"], CONV_SEED), strict=False)
    model.eval()
    toks = tokens(TOKEN_SEED)
    with torch.no_grad():
        out = model(torch.nn.functional.one_hot(toks, len(base.alphabet.all_toks)).float())
    fix = dict(dims=DIMS, model_seed=MODEL_SEED, conv_seed=CONV_SEED, tokens=toks,
               **{k: v.float().contiguous() for k, v in out.items()})  # [B, n, S, S] each
    torch.save(fix, OUT)
    print(OUT, os.path.getsize(OUT), {k: tuple(v.shape) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
