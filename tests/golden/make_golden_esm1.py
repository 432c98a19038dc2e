"""Generate the ESM-1 fixtures tests/golden/esm1_*.pt by running the REFERENCE implementation (/root/reference/esm, imported
read-only) on seeded synthetic weights (esm_amd.synth.synth_esm1_state_dict).

    python tests/golden/make_golden_esm1.py        # only works where /root/reference is mounted

Each case writes two files: ``esm1_<name>.pt`` (tokens, dims and seed, weight checksum, the reference's state-dict key list,
every representation, logits, contacts, the null-key figures) and ``esm1_<name>_attn.pt`` (attentions).  Padded query rows
carry values the engine does not reproduce (unspecified there), and every file must stay below the repository's size limit,
so tensors are stored on the real tokens only: ``x[tokens != pad]`` for representations and logits ([n_real, .]), per-sequence
``[len - 1, len - 1]`` contact crops and ``[L, H, len, len]`` attention crops (everything outside them is exactly zero in the
reference's output, which the generator asserts).

The generator also checks, asserts and records that the synthetic weights make the null key MATTER:
  null_mass      mean over layers, heads and real query rows of 1 - sum_j attentions[..., i, j]        >= 0.05
  null_removed   relative L2 change of the last representation when the CPU restatement (tests/_esm1_oracle.py) runs
                 without the null key                                                                  >= 1e-2
"""
import importlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = "/root/reference"

CASES = {
    # pads (one interior) and one <mask>
    "tiny_d64": dict(L=2, E=128, H=2, seed=41, B=3, T=21, final_bias=False, token_dropout=False, lengths=[21, 15, 21]),
    "mid_d64": dict(L=3, E=192, H=3, seed=42, B=2, T=70, final_bias=True, token_dropout=True, lengths=[70, 52]),
    # full and partial 64-key tiles, the 128-row query-block edge
    "edges_d64": dict(L=2, E=128, H=2, seed=43, B=4, T=130, final_bias=False, token_dropout=False, lengths=[64, 65, 128, 130]),
}
PAD, CLS, MASK = 1, 32, 33


def build_tokens(c):
    g = torch.Generator().manual_seed(c["seed"])
    toks = torch.randint(4, 24, (c["B"], c["T"]), generator=g, dtype=torch.int64)
    toks[:, 0] = CLS
    for b, n in enumerate(c["lengths"]):
        toks[b, n:] = PAD
    toks[0, 3] = MASK
    if c["token_dropout"]:
        toks[1, 7] = MASK
        toks[1, 9] = MASK
    if c["B"] == 3:
        toks[2, c["T"] // 2] = PAD  # an interior pad
    return toks


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from esm_amd.synth import esm1_args, synth_esm1_state_dict
    from _esm1_oracle import esm1_forward

    sys.path.insert(0, REFERENCE)
    for k in [k for k in sys.modules if k == "esm" or k.startswith("esm.")]:
        del sys.modules[k]
    ref = importlib.import_module("esm")
    assert ref.__file__.startswith(REFERENCE), ref.__file__
    alphabet = ref.Alphabet.from_architecture("protein_bert_base")
    assert (alphabet.padding_idx, alphabet.cls_idx, alphabet.mask_idx, len(alphabet)) == (PAD, CLS, MASK, 35)
    for name, c in CASES.items():
        L, E, H = c["L"], c["E"], c["H"]
        sd = synth_esm1_state_dict(L, E, H, seed=c["seed"], final_bias=c["final_bias"])
        model = ref.ProteinBertModel(esm1_args(L, E, H, c["final_bias"], c["token_dropout"]), alphabet).eval()
        model.load_state_dict(sd, strict=True)
        toks = build_tokens(c)
        with torch.no_grad():
            out = model(toks, repr_layers=list(range(L + 1)), return_contacts=True)
        real = toks.ne(PAD)
        attn, contacts = out["attentions"].float(), out["contacts"].float()
        # null-key mass on real query rows (real keys only: pad columns are zero)
        mass = (1 - attn.sum(-1)).permute(0, 3, 1, 2)[real]  # [n_real, L, H]
        null_mass = mass.mean().item()
        kw = dict(repr_layers=[L], token_dropout=c["token_dropout"])
        with_null = esm1_forward(sd, toks, L, H, **kw)["representations"][L][real]
        without = esm1_forward(sd, toks, L, H, null_key=False, **kw)["representations"][L][real]
        refL = out["representations"][L].float()[real]
        null_removed = ((without - refL).norm() / refL.norm()).item()
        restated = ((with_null - refL).norm() / refL.norm()).item()
        print(f"{name}: null-key mass {null_mass:.3f} (min over layers/heads {mass.mean(0).min().item():.3f}), without the null key "
              f"rel L2 {null_removed:.3e}, restatement rel L2 {restated:.1e}")
        assert null_mass >= 0.05, null_mass
        assert null_removed >= 1e-2, null_removed
        # crops: what lies outside them is zero (interior pads stay inside the crop)
        lens = [int(real[b].nonzero().max()) + 1 for b in range(c["B"])]
        chk_a, chk_c = attn.clone(), contacts.clone()
        for b, n in enumerate(lens):
            chk_a[b, :, :, :n, :n] = 0
        assert float(chk_a.abs().max()) == 0.0
        fix = {
            "dims": {k: c[k] for k in ("L", "E", "H", "seed", "final_bias", "token_dropout")},
            "tokens": toks,
            "lengths": lens,
            "weights_checksum": float(sum(v.double().sum() for v in sd.values())),
            "state_dict_keys": sorted(model.state_dict().keys()),
            "logits": out["logits"].float()[real].clone(),
            "representations": {k: v.float()[real].clone() for k, v in out["representations"].items()},
            "contacts": [contacts[b, :n - 1, :n - 1].clone() for b, n in enumerate(lens)],
            "null_mass": null_mass,
            "null_removed_rel_l2": null_removed,
            "reference_version": getattr(ref, "__version__", "?"),
            "torch_version": torch.__version__,
        }
        path = os.path.join(HERE, f"esm1_{name}.pt")
        torch.save(fix, path)
        apath = os.path.join(HERE, f"esm1_{name}_attn.pt")
        torch.save({"attentions": [attn[b, :, :, :n, :n].clone() for b, n in enumerate(lens)]}, apath)
        for q in (path, apath):
            print("  ->", q, os.path.getsize(q) // 1024, "KiB")
            assert os.path.getsize(q) < (1 << 20), "fixture above the 1 MiB limit for committed files"


if __name__ == "__main__":
    main()
