"""Cut a deep a3m alignment down to the rows the MSA Transformer takes, on the MI355X:

    python -m esm_amd.subsample_msa --msa-path in.a3m --num-seqs 128 --strategy greedy --output out.a3m [--weights-out w.npy]

The preprocessing step of the reference's contact notebook in front of ``predict_contacts`` (``greedy_select``), plus the
reweighted and uniform draws of ``esm_amd.msa_select``.  Every record of the file is read with its insertions removed
(``esm_amd.fasta.read_msa``); the chosen records are written that way, the query first and the others in file order.  Prints
the number of rows N, the number of columns L and the effective number of sequences Neff at ``--theta``; ``--weights-out``
saves the fp64 sequence weights of all N rows.
"""
import argparse
import pathlib
import sys
import types

from . import msa_select


def create_parser():
    p = argparse.ArgumentParser(prog="python -m esm_amd.subsample_msa",
                                description="Choose the rows of an MSA on the MI355X: diversity-greedy or reweighted.")
    p.add_argument("--msa-path", type=pathlib.Path, required=True, help="a3m file; its first record is the query")
    p.add_argument("--num-seqs", type=int, required=True, help="number of rows to keep (the query included)")
    p.add_argument("--strategy", type=str, default="greedy", choices=msa_select.STRATEGIES)
    p.add_argument("--theta", type=float, default=0.2, help="Hamming distance below which two rows are neighbours")
    p.add_argument("--seed", type=int, default=0, help="seed of the weighted / uniform draw")
    p.add_argument("--subsample", type=int, default=0, help="which draw of that seed (weighted / uniform)")
    p.add_argument("--output", type=pathlib.Path, required=True, help="a3m file to write")
    p.add_argument("--weights-out", type=pathlib.Path, default=None, help=".npy file for the fp64 sequence weights of all rows")
    return p


def parse_args(argv=None):
    parser = create_parser()
    args = parser.parse_args(argv)
    if args.num_seqs < 1:
        parser.error("--num-seqs must be at least 1")
    if args.subsample < 0 or args.seed < 0:
        parser.error("--seed and --subsample must not be negative")
    return args


def main(argv=None):
    args = parse_args(argv)
    from .fasta import read_msa

    msa = read_msa(args.msa_path, None)
    if not msa:
        raise SystemExit(f"esm_amd.subsample_msa: {args.msa_path} holds no sequence")
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("esm_amd.subsample_msa: no GPU: the engine has no CPU path")
    enc = msa_select.encode_msa(msa)
    counts = msa_select.msa_neighbor_counts(enc, args.theta)
    weights = 1.0 / counts.to(torch.float64)
    idx = msa_select.subsample_indices(enc, args.num_seqs, args.strategy, args.theta, args.seed, args.subsample, counts=counts)
    with open(args.output, "w") as fh:
        for i in idx:
            fh.write(f">{msa[i][0]}\n{msa[i][1]}\n")
    if args.weights_out is not None:
        import numpy as np

        np.save(args.weights_out, weights.cpu().numpy())
    print(f"N = {enc.shape[0]}  L = {enc.shape[1]}  Neff = {float(weights.sum()):.1f} (theta {args.theta})  kept {len(idx)} rows "
          f"({args.strategy}) -> {args.output}")
    return 0


class _CallableModule(types.ModuleType):
    """``esm_amd.subsample_msa`` names both this command-line module and the function ``esm_amd.msa_select.subsample_msa``
    that the package exports; importing the module rebinds the package attribute to it, so the module forwards calls."""

    def __call__(self, *args, **kwargs):
        return msa_select.subsample_msa(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule

if __name__ == "__main__":
    sys.exit(main())
