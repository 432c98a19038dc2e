"""Draw sequences from one model, every step on the MI355X:

    python -m esm_amd.sample --model-location esm2_t33_650M_UR50D --sequence MKTAYIAKQR --num-chains 8 --sweeps 4 \\
        --output samples.fasta
    python -m esm_amd.sample --model-location esm2_t33_650M_UR50D --fasta scaffolds.fasta --mode inpaint --output filled.fasta

gibbs    (default) ``--sweeps`` Gibbs sweeps around every input sequence: each sweep visits all residues once in a random
         order, ``--per-step`` of them masked and redrawn together (``esm_amd.sampling.gibbs_sample``).
inpaint  ``_`` or ``<mask>`` in the input marks the positions to fill; everything else stays (``esm_amd.sampling.inpaint``).
         ``--order confidence`` (or ``entropy``) fills the most confident positions first instead of a random order.

``--top-k`` / ``--top-p`` put a top-k / nucleus filter in front of every draw, in either mode.

``--steer VEC.npy --steer-layer K [--steer-gain A]`` draws from the STEERED model: A times the fp32 [embed_dim] direction in
VEC.npy is added to every residue's stream after K layers in every forward of the run (``model.stream_edits``;
``esm_amd.mean_difference`` makes such a direction).  Without them the run is the unsteered one, call for call.

Every input record is run as ``--num-chains`` chains.  Chain ids count through the output (record r, copy c: r * num_chains +
c), and a draw depends on (seed, chain id) alone, so one record of the output can be drawn again by itself.  The output is a
FASTA file; a record is named ``<label>|chain=<id>|seed=<seed>``.
"""
import argparse
import contextlib
import pathlib
import sys

MODES = ("gibbs", "inpaint")
ORDERS = ("random", "confidence", "entropy")
PER_CALL = 64  # chains per call


def create_parser():
    p = argparse.ArgumentParser(prog="python -m esm_amd.sample",
                                description="Gibbs sampling / mask in-painting with a protein language model on the MI355X.")
    p.add_argument("--model-location", type=str, required=True, help="checkpoint file or name of a pretrained model")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--sequence", type=str, help="one starting sequence (inpaint: '_' or '<mask>' marks a position to fill)")
    src.add_argument("--fasta", type=pathlib.Path, help="FASTA file of starting sequences")
    p.add_argument("--mode", type=str, default="gibbs", choices=MODES)
    p.add_argument("--sweeps", type=int, default=1, help="Gibbs sweeps (gibbs only)")
    p.add_argument("--per-step", type=int, default=1, help="positions masked and drawn together in one step")
    p.add_argument("--temperature", type=float, default=1.0, help="0: the argmax")
    p.add_argument("--top-k", type=int, default=0, help="draw from the k most probable candidates only (0: all)")
    p.add_argument("--top-p", type=float, default=1.0, help="draw from the nucleus of this probability mass only (1: all)")
    p.add_argument("--order", type=str, default="random", choices=ORDERS,
                   help="inpaint only: a random order, or the most confident positions first (max log q / negative entropy)")
    p.add_argument("--num-chains", type=int, default=1, help="chains per input sequence")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--steer", type=pathlib.Path, default=None, help=".npy file of an [embed_dim] direction added to every residue's stream")
    p.add_argument("--steer-layer", type=int, default=None, help="the stream after this many layers takes the direction (0 .. L)")
    p.add_argument("--steer-gain", type=float, default=1.0, help="multiple of the direction that is added")
    p.add_argument("--output", type=pathlib.Path, required=True, help="FASTA file to write")
    return p


def parse_args(argv=None):
    parser = create_parser()
    args = parser.parse_args(argv)
    if args.sweeps < 0:
        parser.error("--sweeps must not be negative")
    if args.per_step <= 0:
        parser.error("--per-step must be positive")
    if args.num_chains <= 0:
        parser.error("--num-chains must be positive")
    if not args.temperature >= 0.0 or args.temperature == float("inf"):
        parser.error("--temperature must be finite and not negative")
    if not 0 <= args.seed < 2 ** 64:
        parser.error("--seed must lie in [0, 2^64)")
    if not 0 <= args.top_k <= 64:
        parser.error("--top-k must lie in 0 .. 64 (0: no top-k filter)")
    if not 0.0 < args.top_p <= 1.0:
        parser.error("--top-p must lie in (0, 1] (1: no nucleus filter)")
    if (args.steer is None) != (args.steer_layer is None):
        parser.error("--steer and --steer-layer go together")
    if args.steer is None and args.steer_gain != 1.0:
        parser.error("--steer-gain needs --steer")
    if args.order != "random" and args.mode != "inpaint":
        parser.error("--order applies to --mode inpaint only: a Gibbs sweep has no masked positions to rank")
    return args


def read_records(args):
    """[(label, sequence)] of the input."""
    if args.sequence is not None:
        return [("sequence", args.sequence.strip())]
    from .fasta import FastaBatchedDataset

    data = FastaBatchedDataset.from_file(args.fasta)
    return list(zip(data.sequence_labels, data.sequence_strs))


def prepare_sequence(sequence, mode):
    """The string the alphabet tokenises: for inpaint ``_`` becomes ``<mask>``.  A gibbs input must not hold either."""
    if mode == "inpaint":
        sequence = sequence.replace("_", "<mask>")
        if "<mask>" not in sequence:
            raise ValueError("inpaint: the sequence holds no '_' or '<mask>': there is nothing to fill")
        return sequence
    if "_" in sequence or "<mask>" in sequence:
        raise ValueError("gibbs: the sequence holds '_' or '<mask>'; those mark positions for --mode inpaint")
    return sequence


def chain_records(records, num_chains, mode):
    """[(label, chain id, prepared sequence)]: ``num_chains`` copies of every record, chain ids counting through."""
    return [(label, r * num_chains + c, prepare_sequence(seq, mode)) for r, (label, seq) in enumerate(records)
            for c in range(num_chains)]


def decode(alphabet, row):
    """The residues of one row of final tokens: without <cls>, <eos> and <pad>."""
    skip = {alphabet.padding_idx, alphabet.cls_idx, alphabet.eos_idx}
    return "".join(alphabet.get_tok(int(t)) for t in row if int(t) not in skip)


def steering(model, args):
    """The context the draws run in: ``model.stream_edits`` with the ``--steer`` direction, or nothing at all."""
    if getattr(args, "steer", None) is None:
        return contextlib.nullcontext()
    import numpy as np
    import torch

    from .interventions import StreamEdit

    vec = torch.from_numpy(np.load(args.steer).astype(np.float32).reshape(-1))
    return model.stream_edits([StreamEdit(args.steer_layer, "add", vec, gain=args.steer_gain, positions="residues")])


def sample_records(model, alphabet, chains, args):
    """The final sequence of every chain, ``PER_CALL`` chains per call."""
    with steering(model, args):
        return _sample_records(model, alphabet, chains, args)


def _sample_records(model, alphabet, chains, args):
    convert = alphabet.get_batch_converter()
    out = []
    for lo in range(0, len(chains), PER_CALL):
        part = chains[lo:lo + PER_CALL]
        _, _, tokens = convert([(label, seq) for label, _, seq in part])
        ids = [cid for _, cid, _ in part]
        if args.mode == "gibbs":
            final = model.gibbs_sample(tokens, args.sweeps, per_step=args.per_step, temperature=args.temperature, seed=args.seed,
                                       chain_ids=ids, top_k=args.top_k, top_p=args.top_p)
        else:
            final = model.inpaint(tokens, per_step=args.per_step, temperature=args.temperature, seed=args.seed, chain_ids=ids,
                                  top_k=args.top_k, top_p=args.top_p, order=args.order)
        out += [decode(alphabet, row) for row in final.cpu().tolist()]
    return out


def write_fasta(path, chains, sequences, seed):
    with open(path, "w") as fh:
        for (label, cid, _), seq in zip(chains, sequences):
            fh.write(f">{label}|chain={cid}|seed={seed}\n{seq}\n")


def main(argv=None):
    args = parse_args(argv)
    chains = chain_records(read_records(args), args.num_chains, args.mode)
    import torch

    from . import pretrained
    from .msa_transformer import MSATransformer

    model, alphabet = pretrained.load_model_and_alphabet(args.model_location)
    if isinstance(model, MSATransformer):
        raise SystemExit(f"esm_amd.sample: {args.model_location} is an MSA Transformer; sampling draws single sequences "
                         "(ESM-2, ESM-1b / ESM-1v and ESM-1 models)")
    if not torch.cuda.is_available():
        raise SystemExit("esm_amd.sample: no GPU: the engine has no CPU path")
    model = model.eval().cuda()
    write_fasta(args.output, chains, sample_records(model, alphabet, chains, args), args.seed)
    return 0


if __name__ == "__main__":
    sys.exit(main())
