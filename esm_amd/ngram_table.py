"""Write the background of the n-gram term from a FASTA file (``esm_amd.ngram.Background``), counted on the host in numpy.

    python -m esm_amd.ngram_table --fasta F [--orders 1 2 3] [--floor 1e-5] --output bg.npz
"""
import argparse
import sys

from .ngram import MAX_ORDER, STANDARD_ALPHABET, Background


def read_fasta(path):
    """The sequences of a FASTA file, upper-cased, in file order."""
    seqs, parts = [], None
    with open(path) as fh:
        for line in fh:
            line = line.strip()
            if line.startswith(">"):
                if parts is not None:
                    seqs.append("".join(parts))
                parts = []
            elif line and parts is not None:
                parts.append(line.upper())
    if parts is not None:
        seqs.append("".join(parts))
    return seqs


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m esm_amd.ngram_table", description="Count an n-gram background for "
                                "`python -m esm_amd.design --w-ngram W --ngram-table bg.npz`.")
    p.add_argument("--fasta", required=True)
    p.add_argument("--orders", type=int, nargs="+", default=[1, 2, 3], choices=range(1, MAX_ORDER + 1))
    p.add_argument("--floor", type=float, default=1e-5, help="the least probability of a table; also that of an unseen n-gram")
    p.add_argument("--alphabet", default=STANDARD_ALPHABET)
    p.add_argument("--output", required=True, help=".npz file")
    a = p.parse_args(argv)
    if not 0.0 < a.floor < float("inf"):
        p.error("--floor must be positive and finite")
    return a


def main(argv=None):
    a = parse_args(argv)
    seqs = read_fasta(a.fasta)
    if not seqs:
        raise SystemExit(f"esm_amd.ngram_table: {a.fasta} holds no FASTA record")
    bg = Background.from_sequences(seqs, orders=a.orders, alphabet=a.alphabet, floor=a.floor)
    bg.save(a.output)
    print(f"{len(seqs)} sequences, orders {list(bg.orders)}, {len(bg.alphabet)} letters -> {a.output}", file=sys.stderr)


if __name__ == "__main__":
    main()
