"""Label a deep mutational scan with zero-shot scores of one or more MSA Transformer models:

    python -m esm_amd.predict_msa --model-location esm_msa1b_t12_100M_UR50S --msa-path protein.a3m --dms-input scan.csv \\
        --mutation-col mutant --dms-output scored.csv --offset-idx 1

The MSA branch of the reference's ``examples/variant-prediction/predict.py`` (:161-184): ``--msa-samples`` records of the a3m
file (insertions removed, ``esm_amd.fasta.read_msa``) are the MSA, its first row is the wild type, and every model adds one
column, named after its ``--model-location``, to the table.  Which records: ``--msa-subsample first`` (the default, what the
reference does) parses and takes the first ``--msa-samples``; ``greedy``, ``weighted`` and ``uniform`` read the whole file and
choose that many rows on the device (``esm_amd.msa_select``: the contact notebook's diversity-greedy pick, the reweighted draw
of the ESM-1v paper at ``--msa-theta``, a uniform draw; the query always stays the first row).  ``--msa-ensemble K`` scores K
different ``weighted`` / ``uniform`` subsamples (``--msa-seed``) and writes their mean.  The scores come from
``esm_amd.msa_scoring``: the masked copies of the MSA run as batches that fill the GPU instead of one forward per column, and
only the positions the table names are scored.  The table is read and written by ``esm_amd.predict`` (``csv`` module; the
output starts with an unnamed row-index column, as the reference's ``DataFrame.to_csv`` writes it).

``--scoring-strategy wt-marginals`` (one forward of the unmasked MSA) is an extension: the reference takes only
masked-marginals for MSAs.  A row may hold several substitutions joined by ``--mutation-sep`` ('A42G:K50R'): all of its
positions are masked in the first row at once and log p(mutant) - log p(wild type) is summed over them.
"""
import argparse
import pathlib
import sys

from .msa_scoring import STRATEGIES
from .predict import read_table, write_table

SUBSAMPLE_CHOICES = ("first", "greedy", "weighted", "uniform")


def create_parser():
    p = argparse.ArgumentParser(prog="python -m esm_amd.predict_msa",
                                description="Score the substitutions of a deep mutational scan with the MSA Transformer on "
                                            "the MI355X.")
    p.add_argument("--model-location", type=str, nargs="+", required=True,
                   help="checkpoint file(s) or name(s) of pretrained MSA Transformer model(s); one output column each")
    p.add_argument("--msa-path", type=pathlib.Path, required=True, help="a3m file of the MSA; its first record is the wild type")
    p.add_argument("--msa-samples", type=int, default=400, help="number of sequences to take from the start of the MSA")
    p.add_argument("--sequence", type=str, default=None,
                   help="wild-type sequence the mutations refer to; when given it must equal the first row of the MSA")
    p.add_argument("--dms-input", type=pathlib.Path, required=True, help="CSV file of the deep mutational scan")
    p.add_argument("--mutation-col", type=str, default="mutant", help="column holding the mutation as 'A42G'")
    p.add_argument("--dms-output", type=pathlib.Path, required=True, help="CSV file to write: the input plus the scores")
    p.add_argument("--mutation-sep", type=str, default=":",
                   help="separator of the substitutions of a multi-mutant row, as in 'A42G:K50R'")
    p.add_argument("--offset-idx", type=int, default=0, help="index of the first residue in the mutation column's numbering")
    p.add_argument("--scoring-strategy", type=str, default="masked-marginals", choices=STRATEGIES)
    p.add_argument("--msa-subsample", type=str, default="first", choices=SUBSAMPLE_CHOICES,
                   help="how the --msa-samples rows are chosen: the first records, the diversity-greedy pick, or a draw with "
                        "(weighted) or without (uniform) sequence reweighting; the query is always kept")
    p.add_argument("--msa-theta", type=float, default=0.2,
                   help="Hamming distance below which two rows are neighbours (sequence weights of --msa-subsample weighted)")
    p.add_argument("--msa-seed", type=int, default=0, help="seed of the weighted / uniform draw")
    p.add_argument("--msa-ensemble", type=int, default=1,
                   help="score this many different subsamples and write the mean (weighted or uniform only)")
    return p


def parse_args(argv=None):
    """The parsed command line, or SystemExit: --msa-ensemble K > 1 needs a subsample that differs from draw to draw."""
    parser = create_parser()
    args = parser.parse_args(argv)
    if args.msa_ensemble < 1:
        parser.error("--msa-ensemble must be at least 1")
    if args.msa_ensemble > 1 and args.msa_subsample not in ("weighted", "uniform"):
        parser.error(f"--msa-ensemble {args.msa_ensemble} needs --msa-subsample weighted or uniform: "
                     f"'{args.msa_subsample}' gives the same rows every time")
    return args


def load_msa(path, nseq, sequence=None):
    """``read_msa`` plus the checks of the command line: a non-empty MSA whose first row is ``sequence`` (when given)."""
    from .fasta import read_msa

    msa = read_msa(path, nseq)
    if not msa:
        raise SystemExit(f"esm_amd.predict_msa: {path} holds no sequence (--msa-samples {nseq})")
    if sequence is not None and sequence != msa[0][1]:
        raise SystemExit(f"esm_amd.predict_msa: --sequence does not equal the first row of {path}")
    return msa


def score_table(model, alphabet, msa, mutations, strategy="masked-marginals", offset_idx=0, sep=":"):
    """One score per mutation string of the table: ``esm_amd.msa_scoring.msa_score_variants`` on the first row of ``msa``."""
    from . import msa_scoring

    return msa_scoring.msa_score_variants(model, alphabet, msa, list(mutations), strategy, offset_idx, sep or ":")


def score_table_ensemble(model, alphabet, msa, mutations, num_seqs, n_subsamples, subsample, theta=0.2, seed=0,
                         strategy="masked-marginals", offset_idx=0, sep=":"):
    """The ensemble mean per mutation string: ``esm_amd.msa_scoring.msa_score_variants_ensemble`` on the full ``msa``."""
    from . import msa_scoring

    return msa_scoring.msa_score_variants_ensemble(model, alphabet, msa, list(mutations), num_seqs, n_subsamples, subsample,
                                                   theta, seed, strategy, offset_idx, sep or ":")[0]


def main(argv=None):
    args = parse_args(argv)
    first = args.msa_subsample == "first"
    msa = load_msa(args.msa_path, args.msa_samples if first else None, args.sequence)
    import torch

    from . import pretrained
    from .msa_transformer import MSATransformer

    fields, rows = read_table(args.dms_input, args.mutation_col)
    mutations = [row[args.mutation_col] for row in rows]
    for location in args.model_location:
        model, alphabet = pretrained.load_model_and_alphabet(location)
        if not isinstance(model, MSATransformer):
            raise SystemExit(f"esm_amd.predict_msa: {location} is not an MSA Transformer: use python -m esm_amd.predict")
        if not torch.cuda.is_available():
            raise SystemExit("esm_amd.predict_msa: no GPU: the engine has no CPU path")
        model = model.eval().cuda()
        if args.msa_ensemble > 1:
            scores = score_table_ensemble(model, alphabet, msa, mutations, args.msa_samples, args.msa_ensemble,
                                          args.msa_subsample, args.msa_theta, args.msa_seed, args.scoring_strategy,
                                          args.offset_idx, args.mutation_sep)
        else:
            picked = msa
            if not first:
                from . import msa_select

                picked = msa_select.subsample_msa(msa, args.msa_samples, args.msa_subsample, args.msa_theta, args.msa_seed)
            scores = score_table(model, alphabet, picked, mutations, args.scoring_strategy, args.offset_idx, args.mutation_sep)
        for row, s in zip(rows, scores):
            row[location] = repr(float(s))
        fields.append(location)
    write_table(args.dms_output, fields, rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
