"""Score every sequence of a FASTA or CSV file with one model — rank a library of designed sequences, or insertion / deletion
variants by the score of the full mutated sequence:

    python -m esm_amd.score_sequences --model-location esm2_t33_650M_UR50D --fasta designs.fasta --output scored.csv
    python -m esm_amd.score_sequences --model-location esm1v_t33_650M_UR90S_1 --csv designs.csv --sequence-col sequence \\
        --output scored.csv --strategy wt-marginals

One output row per sequence: ``label,length,pll,pseudo_perplexity``.

pseudo-ppl    (default) ``pll`` is the pseudo-log-likelihood of the sequence: every residue masked in turn, the
              log-probability of the true residue at the masked position, summed (``esm_amd.scoring.pseudo_log_likelihood``:
              all residues, not the reference's ``range(1, len(sequence) - 1)``).
wt-marginals  ``pll`` is the sum of the log-probabilities of the true residues in ONE unmasked forward per sequence.
``pseudo_perplexity`` is ``exp(-pll / length)``; ``length`` counts residues.

The sequences of such a file differ in length, so the masked copies run token-packed (``varlen=True``: no compute on padding,
sums in a fixed order).  ``--no-varlen`` runs the padded path: the same table of log-probabilities bit for bit, so the same
file for wt-marginals; for pseudo-ppl the padded sum goes through atomics in no fixed order and may differ in the last digits.
``--window N`` (``--window max`` on ESM-1b / ESM-1v) scores sequences LONGER than the window inside model-sized windows
(``esm_amd.windows``: every residue in the window centred on it for pseudo-ppl, overlapping windows with every row from the window
it is most central in for wt-marginals); ``--no-wrap`` cuts raw token slices instead of tokenised fragments.  Shorter sequences are
scored as without the option.
The CSV is read with the ``csv`` module; labels come from ``--label-col`` or are the 0-based row numbers.
"""
import argparse
import csv
import math
import pathlib
import sys

STRATEGIES = ("pseudo-ppl", "wt-marginals")
PER_CALL = 256  # sequences per call; their masked copies are chunked to the GPU's size inside


def create_parser():
    p = argparse.ArgumentParser(prog="python -m esm_amd.score_sequences",
                                description="Pseudo-log-likelihood of every sequence of a FASTA or CSV file on the MI355X.")
    p.add_argument("--model-location", type=str, required=True, help="checkpoint file or name of a pretrained model")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--fasta", type=pathlib.Path, help="FASTA file of the sequences")
    src.add_argument("--csv", type=pathlib.Path, help="CSV file with one sequence per row (needs --sequence-col)")
    p.add_argument("--sequence-col", type=str, default=None, help="column of --csv that holds the sequence")
    p.add_argument("--label-col", type=str, default=None, help="column of --csv that holds the label (default: the row number)")
    p.add_argument("--output", type=pathlib.Path, required=True, help="CSV file to write: label, length, pll, pseudo_perplexity")
    p.add_argument("--strategy", type=str, default="pseudo-ppl", choices=STRATEGIES)
    p.add_argument("--no-varlen", action="store_true", help="run the padded path instead of the token-packed one")
    from .windows import window_arg

    p.add_argument("--window", type=window_arg, default=None, metavar="{N,max}",
                   help="tokens per window (special tokens included) for sequences longer than the model's window; 'max': the "
                        "size of the position table of ESM-1b / ESM-1v")
    p.add_argument("--no-wrap", action="store_true", help="with --window: raw token slices instead of tokenised fragments")
    return p


def read_records(args, parser):
    """[(label, sequence)] of the input file."""
    if args.fasta is not None:
        if args.sequence_col is not None or args.label_col is not None:
            parser.error("--sequence-col / --label-col go with --csv")
        from .fasta import FastaBatchedDataset

        data = FastaBatchedDataset.from_file(args.fasta)
        return list(zip(data.sequence_labels, data.sequence_strs))
    if args.sequence_col is None:
        parser.error("--csv needs --sequence-col")
    with open(args.csv, newline="") as fh:
        reader = csv.DictReader(fh)
        rows = list(reader)
        fields = list(reader.fieldnames or [])
    for col in (args.sequence_col, args.label_col):
        if col is not None and col not in fields:
            raise SystemExit(f"{args.csv}: no column {col!r} (columns: {', '.join(fields)})")
    return [(row[args.label_col] if args.label_col else str(i), row[args.sequence_col].strip()) for i, row in enumerate(rows)]


def score_records(model, alphabet, records, strategy="pseudo-ppl", varlen=True, window=None, wrap=True):
    """One float per record: the pseudo-log-likelihood (pseudo-ppl) or the sum of the unmasked log-probabilities of the true
    residues (wt-marginals) of every sequence, ``PER_CALL`` sequences per call.  A sequence longer than an ESM-1b model's
    positional limit raises the ValueError of ``esm_amd.scoring`` unless ``window`` is given: then it is scored inside
    model-sized windows (``esm_amd.windows``)."""
    import torch

    from . import ops, scoring

    if strategy not in STRATEGIES:
        raise ValueError(f"unknown scoring strategy {strategy!r}")
    convert = alphabet.get_batch_converter()
    win = {} if window is None else dict(window=window, wrap=wrap)
    scores = []
    for lo in range(0, len(records), PER_CALL):
        _, _, tokens = convert(records[lo:lo + PER_CALL])
        if strategy == "pseudo-ppl":
            scores += model.pseudo_log_likelihood(tokens, varlen=varlen, **win).tolist()
            continue
        table = model.wt_marginals(tokens, varlen=varlen, **win)
        tok = tokens.to(table.device)
        want = tok.ne(model.padding_idx)  # the residues: no <cls>, no <eos>, no <pad>
        if model.prepend_bos:
            want[:, 0] = False
        if model.append_eos:
            want &= tok.ne(model.eos_idx)
        src, pos = want.nonzero(as_tuple=True)
        if src.numel() == 0:
            scores += [0.0] * tokens.shape[0]
            continue
        off = torch.zeros((tokens.shape[0] + 1,), dtype=torch.int64, device=table.device)
        off[1:] = torch.bincount(src, minlength=tokens.shape[0]).cumsum(0)
        # fp32 terms added in fp64 in ascending order of position by one lane per sequence
        scores += ops.sum_target_rows(table[src, pos].contiguous(), tok[src, pos].to(torch.int32), off.to(torch.int32)).tolist()
    return scores


def write_scores(path, records, scores):
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["label", "length", "pll", "pseudo_perplexity"])
        for (label, seq), s in zip(records, scores):
            w.writerow([label, len(seq), repr(float(s)), repr(math.exp(-float(s) / len(seq))) if seq else "nan"])


def main(argv=None):
    parser = create_parser()
    args = parser.parse_args(argv)
    records = read_records(args, parser)
    import torch

    from . import pretrained
    from .msa_transformer import MSATransformer

    model, alphabet = pretrained.load_model_and_alphabet(args.model_location)
    if isinstance(model, MSATransformer):
        raise SystemExit(f"esm_amd.score_sequences: {args.model_location} is an MSA Transformer, which scores one MSA plus a query "
                         "row (python -m esm_amd.predict_msa), not single sequences")
    if not torch.cuda.is_available():
        raise SystemExit("esm_amd.score_sequences: no GPU: the engine has no CPU path")
    model = model.eval().cuda()
    with torch.no_grad():
        scores = score_records(model, alphabet, records, args.strategy, varlen=not args.no_varlen, window=args.window,
                               wrap=not args.no_wrap)
    write_scores(args.output, records, scores)
    return 0


if __name__ == "__main__":
    sys.exit(main())
