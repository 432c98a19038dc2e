"""Label a deep mutational scan with zero-shot scores of one or more models:

    python -m esm_amd.predict --model-location esm1v_t33_650M_UR90S_1 --sequence MKT... --dms-input scan.csv \\
        --mutation-col mutant --dms-output scored.csv --offset-idx 1 --scoring-strategy masked-marginals

The options are those of the reference's ``examples/variant-prediction/predict.py``; every model adds one column, named
after its ``--model-location``, to the table.  The scores come from ``esm_amd.scoring``: one batched engine call per chunk of
masked positions instead of one forward per position.  The table is read and written with the ``csv`` module (pandas is not
needed); like the reference's ``DataFrame.to_csv`` the output starts with an unnamed row-index column.

One difference in the numbers: ``--scoring-strategy pseudo-ppl`` scores the reference's positions (token positions
1 .. len(sequence) - 2 of every mutated sequence) but sums the log-probability of the token that was MASKED at each of them.
The reference's ``compute_pppl`` (predict.py:143) looks the target up as ``sequence[i]`` at token position i, which behind the
<cls> token is the NEXT residue, so its column differs from this one.  wt-marginals and masked-marginals give the reference's
numbers.

A row may hold several substitutions joined by ``--mutation-sep`` (default ':', e.g. 'A42G:K50R').  Such a variant gets the
masked-marginal score of the ESM-1v paper: all of its positions masked in one forward, log p(mutant) - log p(wild type) summed
over them (``esm_amd.scoring.score_variants``); wt-marginals sums the same terms from the wild-type table, pseudo-ppl scores
the sequence with all substitutions made.  A table without the separator is scored exactly as before.

``--window N`` (or ``--window max`` on ESM-1b / ESM-1v: the size of the position table) scores a protein LONGER than the window:
every mutated site inside a model-sized window centred on it, a multi-mutant row in one window that holds all of its sites
(``esm_amd.windows``).  The windows are fragments tokenised like the whole (<cls> / <eos> of their own); ``--no-wrap`` cuts raw
token slices instead.  A sequence that fits is scored exactly as without the option.

The MSA Transformer (``--msa-path``) is not served here: asking for it is an error that points to
``python -m esm_amd.predict_msa``, which scores a table with an MSA (``esm_amd.msa_scoring``).
"""
import argparse
import csv
import pathlib
import sys

STRATEGIES = ("wt-marginals", "pseudo-ppl", "masked-marginals")


def create_parser():
    p = argparse.ArgumentParser(prog="python -m esm_amd.predict",
                                description="Score the substitutions of a deep mutational scan with ESM models on the MI355X.")
    p.add_argument("--model-location", type=str, nargs="+", required=True,
                   help="checkpoint file(s) or name(s) of pretrained model(s); one output column each")
    p.add_argument("--sequence", type=str, required=True, help="wild-type sequence the mutations refer to")
    p.add_argument("--dms-input", type=pathlib.Path, required=True, help="CSV file of the deep mutational scan")
    p.add_argument("--mutation-col", type=str, default="mutant", help="column holding the mutation as 'A42G'")
    p.add_argument("--dms-output", type=pathlib.Path, required=True, help="CSV file to write: the input plus the scores")
    p.add_argument("--mutation-sep", type=str, default=":",
                   help="separator of the substitutions of a multi-mutant row, as in 'A42G:K50R'")
    p.add_argument("--offset-idx", type=int, default=0, help="index of the first residue in the mutation column's numbering")
    p.add_argument("--scoring-strategy", type=str, default="wt-marginals", choices=STRATEGIES)
    p.add_argument("--msa-path", type=pathlib.Path, default=None,
                   help="(MSA Transformer only; not served here: use python -m esm_amd.predict_msa)")
    p.add_argument("--msa-samples", type=int, default=400, help="(MSA Transformer only)")
    p.add_argument("--nogpu", action="store_true", help="accepted for compatibility; the engine has no CPU path")
    from .windows import window_arg

    p.add_argument("--window", type=window_arg, default=None, metavar="{N,max}",
                   help="tokens per window (special tokens included) for a sequence longer than the model's window; 'max': the "
                        "size of the position table of ESM-1b / ESM-1v")
    p.add_argument("--no-wrap", action="store_true", help="with --window: raw token slices instead of tokenised fragments")
    return p


def read_table(path, mutation_col):
    with open(path, newline="") as fh:
        reader = csv.DictReader(fh)
        rows = list(reader)
        fields = list(reader.fieldnames or [])
    if mutation_col not in fields:
        raise SystemExit(f"{path}: no column {mutation_col!r} (columns: {', '.join(fields)})")
    return fields, rows


def write_table(path, fields, rows):
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow([""] + fields)
        for i, row in enumerate(rows):
            w.writerow([i] + [row.get(f, "") for f in fields])


def score_table(model, alphabet, sequence, mutations, strategy, offset_idx=0, sep=":", window=None, wrap=True):
    """One score per mutation string.

    A table of single substitutions: wt-marginals / masked-marginals give log p(mutant) - log p(wild type) at the position,
    from one table of log-probabilities of the wild-type sequence; pseudo-ppl gives the pseudo-log-likelihood of every
    MUTATED sequence over the reference's positions (``esm_amd.scoring.pseudo_log_likelihood``), all mutants in one batch —
    the log-probability of the masked token itself, not of ``sequence[i]`` one residue behind it as the reference's
    ``compute_pppl`` reads it (module docstring).

    A table in which some row joins several substitutions with ``sep`` ('A42G:K50R') is scored, every row of it, by
    ``esm_amd.scoring.score_variants``: joint masks, summed marginals.

    ``window`` / ``wrap``: a sequence longer than the window is scored inside model-sized windows (``esm_amd.windows``)."""
    import torch

    from . import scoring

    scoring._refuse_msa(model)
    mutations = list(mutations)
    win = {} if window is None else dict(window=window, wrap=wrap)
    if sep and any(sep in mutation for mutation in mutations):
        return scoring.score_variants(model, alphabet, sequence, mutations, strategy, offset_idx, sep, **win)
    convert = alphabet.get_batch_converter()
    if strategy == "pseudo-ppl":
        mutated = []
        for mutation in mutations:
            wt, idx, mt = scoring.parse_mutation(mutation, offset_idx)
            if not 0 <= idx < len(sequence) or sequence[idx] != wt:
                raise ValueError(f"{mutation}: the listed wild type does not match the provided sequence")
            mutated.append((mutation, sequence[:idx] + mt + sequence[idx + 1:]))
        scores = []
        per_call = 256  # mutants per call; their masked copies are chunked to the GPU's size inside
        for lo in range(0, len(mutated), per_call):
            _, _, tokens = convert(mutated[lo:lo + per_call])
            pll = model.pseudo_log_likelihood(tokens, positions=range(1, len(sequence) - 1), **win)
            scores += pll.tolist()
        return scores
    _, _, tokens = convert([("protein1", sequence)])
    with torch.no_grad():
        table = model.wt_marginals(tokens, **win) if strategy == "wt-marginals" else model.masked_marginals(tokens, **win)
    return scoring.score_mutations(table.cpu(), sequence, mutations, alphabet, offset_idx)


def main(argv=None):
    args = create_parser().parse_args(argv)
    if args.msa_path is not None:
        raise SystemExit("esm_amd.predict: the MSA Transformer (--msa-path) is not supported: the engine's scoring path "
                         "(esmk_forward_rows) takes ESM-2, ESM-1b / ESM-1v and ESM-1 models; score a table with an MSA through "
                         "python -m esm_amd.predict_msa")
    import torch

    from . import pretrained
    from .msa_transformer import MSATransformer

    fields, rows = read_table(args.dms_input, args.mutation_col)
    mutations = [row[args.mutation_col] for row in rows]
    for location in args.model_location:
        model, alphabet = pretrained.load_model_and_alphabet(location)
        if isinstance(model, MSATransformer):
            raise SystemExit(f"esm_amd.predict: {location} is an MSA Transformer, which the engine's scoring path does not serve here: "
                             "use python -m esm_amd.predict_msa")
        if not torch.cuda.is_available():
            raise SystemExit("esm_amd.predict: no GPU: the engine has no CPU path")
        model = model.eval().cuda()
        scores = score_table(model, alphabet, args.sequence, mutations, args.scoring_strategy, args.offset_idx,
                             args.mutation_sep, window=args.window, wrap=not args.no_wrap)
        for row, s in zip(rows, scores):
            row[location] = repr(float(s))
        fields.append(location)
    write_table(args.dms_output, fields, rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
