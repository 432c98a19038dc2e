"""The extraction driver (python -m esm_amd.extract, the mirror of the reference's scripts/extract.py) on an ESM-1
checkpoint: the reference's own ESM-1 regression for that script (per-token representations of the 34-layer model against
stored values), rebuilt offline on a synthetic checkpoint in the released files' format and checked against the CPU
restatement under the parity contract."""
import os
import subprocess
import sys

import pytest
import torch

import _contract as C
from _esm1_oracle import esm1_forward
from esm_amd.synth import synth_esm1_state_dict, write_esm1_checkpoint

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("extra", [[], ["--no_varlen"]], ids=["default", "padded"])
def test_extract_cli_on_an_esm1_checkpoint(tmp_path, extra):
    L, E, H = 3, 128, 2
    ckpt = write_esm1_checkpoint(str(tmp_path), "esm1_synth_t3", L, E, H, seed=8, final_bias=True)
    g = torch.Generator().manual_seed(5)
    aas = "LAGVSERTIDPKQNFYMHWC"
    seqs = {f"p{i}": "".join(aas[j] for j in torch.randint(0, 20, (n,), generator=g).tolist()) for i, n in enumerate([40, 131, 77])}
    fasta = tmp_path / "in.fasta"
    fasta.write_text("".join(f">{k}\n{v}\n" for k, v in seqs.items()))
    out_dir = tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=ROOT, TORCH_FORCE_NO_WEIGHTS_ONLY_LOAD="1")
    subprocess.run([sys.executable, "-m", "esm_amd.extract", ckpt, str(fasta), str(out_dir), "--repr_layers", "-1", "0",
                    "--include", "mean", "per_tok", "contacts", "--toks_per_batch", "600"] + extra, check=True, env=env, cwd=ROOT,
                   timeout=600)
    sd = synth_esm1_state_dict(L, E, H, seed=8, final_bias=True)
    from esm_amd import Alphabet

    alphabet = Alphabet.from_architecture("protein_bert_base")
    for label, s in seqs.items():
        toks = torch.tensor([[alphabet.cls_idx] + alphabet.encode(s)])  # BOS only
        ref = esm1_forward(sd, toks, L, H, repr_layers=[0, L], return_contacts=True)
        floor = C.floor_forward(sd, toks, L, H, fold=False, forward=esm1_forward, repr_layers=[L])["representations"][L][0]
        r = torch.load(out_dir / f"{label}.pt", weights_only=False)
        assert r["label"] == label and sorted(r["representations"]) == [0, L]
        full = ref["representations"][L][0]
        want, got = full[1:len(s) + 1], r["representations"][L]
        assert got.shape == want.shape
        C.check_tensors(f"esm1 extract[{' '.join(extra)}] {label} repr[{L}]", got, want, floor[1:len(s) + 1])
        full0 = ref["representations"][0][0]
        assert (r["representations"][0] - full0[1:len(s) + 1]).abs().max().item() < 1e-5 * full0.abs().max().item()
        bound = max(C.CONTRACT, C.SLACK_TOY * C.errors(floor, full)[1]) * full.abs().max().item()
        assert (r["mean_representations"][L] - want.mean(0)).abs().max().item() <= bound
        assert r["contacts"].shape == (len(s), len(s))
        assert (r["contacts"] - ref["contacts"][0]).abs().max().item() < 5e-3
