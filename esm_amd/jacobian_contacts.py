"""Contact maps from the categorical Jacobian of one model, every step on the MI355X:

    python -m esm_amd.jacobian_contacts --model-location esm2_t33_650M_UR50D --sequence MKTAYIAKQR --output-dir out
    python -m esm_amd.jacobian_contacts --model-location esm2_t33_650M_UR50D --fasta proteins.fasta --output-dir out \\
        --save-jacobian --allowed ACDEFGHIKLMNPQRSTVWY

For every input record ``<label>.contacts.npy`` (fp32 [L, L], ``esm_amd.jacobian.jacobian_contacts``) is written to
``--output-dir``, and with ``--save-jacobian`` also ``<label>.jacobian.npy``: the centred tensor fp32 [L, nA, L, nA] (400 L^2
floats for the 20 standard residues: 1.7 GB at L = 1022).  Records are processed one at a time: one Jacobian lives on the
device.  ``--allowed``: the candidate residues, in the order given (default the 20 standard ones).  Characters of a label that
do not belong in a file name become ``_``.
"""
import argparse
import pathlib
import re
import sys
import types


def create_parser():
    p = argparse.ArgumentParser(prog="python -m esm_amd.jacobian_contacts",
                                description="Categorical-Jacobian contact maps with a protein language model on the MI355X.")
    p.add_argument("--model-location", type=str, required=True, help="checkpoint file or name of a pretrained model")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--sequence", type=str, help="one sequence")
    src.add_argument("--fasta", type=pathlib.Path, help="FASTA file of sequences")
    p.add_argument("--output-dir", type=pathlib.Path, required=True, help="directory of the .npy files")
    p.add_argument("--save-jacobian", action="store_true", help="also write the centred tensor [L, nA, L, nA]")
    p.add_argument("--allowed", type=str, default=None, help="candidate residues, e.g. ACDEFGHIKLMNPQRSTVWY (the default)")
    p.add_argument("--chunk", type=int, default=None, help="substituted copies per forward call (default: what fills the GPU)")
    return p


def parse_args(argv=None):
    parser = create_parser()
    args = parser.parse_args(argv)
    if args.allowed is not None and (not args.allowed or len(set(args.allowed)) != len(args.allowed)):
        parser.error("--allowed must name at least one residue and none twice")
    if args.chunk is not None and args.chunk <= 0:
        parser.error("--chunk must be positive")
    return args


def read_records(args):
    """[(label, sequence)] of the input."""
    if args.sequence is not None:
        return [("sequence", args.sequence.strip())]
    from .fasta import FastaBatchedDataset

    data = FastaBatchedDataset.from_file(args.fasta)
    return list(zip(data.sequence_labels, data.sequence_strs))


def output_paths(output_dir, label, save_jacobian=False):
    """(contacts file, Jacobian file or None) of one record."""
    stem = re.sub(r"[^A-Za-z0-9._+-]", "_", label.split()[0] if label.split() else "") or "sequence"
    out = pathlib.Path(output_dir)
    return out / f"{stem}.contacts.npy", (out / f"{stem}.jacobian.npy") if save_jacobian else None


def main(argv=None):
    args = parse_args(argv)
    records = read_records(args)
    import numpy as np
    import torch

    from . import pretrained
    from .msa_transformer import MSATransformer

    model, alphabet = pretrained.load_model_and_alphabet(args.model_location)
    if isinstance(model, MSATransformer):
        raise SystemExit(f"esm_amd.jacobian_contacts: {args.model_location} is an MSA Transformer; the categorical Jacobian "
                         "substitutes in single sequences (ESM-2, ESM-1b / ESM-1v and ESM-1 models)")
    if not torch.cuda.is_available():
        raise SystemExit("esm_amd.jacobian_contacts: no GPU: the engine has no CPU path")
    model = model.eval().cuda()
    convert = alphabet.get_batch_converter()
    args.output_dir.mkdir(parents=True, exist_ok=True)
    for label, sequence in records:  # one at a time: one Jacobian on the device
        _, _, tokens = convert([(label, sequence)])
        contacts_file, jacobian_file = output_paths(args.output_dir, label, args.save_jacobian)
        got = model.jacobian_contacts(tokens, allowed=args.allowed, chunk=args.chunk, return_jacobian=args.save_jacobian)
        contacts, jac = got if args.save_jacobian else (got, None)
        np.save(contacts_file, contacts.cpu().numpy())
        if jac is not None:
            np.save(jacobian_file, jac.cpu().numpy())
            del jac, got
    return 0


class _CallableModule(types.ModuleType):
    """``esm_amd.jacobian_contacts`` is both the function the package exports and this module: importing the module rebinds
    the package attribute to it, so the module forwards calls to the function."""

    def __call__(self, model, tokens, **kwargs):
        from .jacobian import jacobian_contacts

        return jacobian_contacts(model, tokens, **kwargs)


if __name__ == "__main__":
    sys.exit(main())
else:
    sys.modules[__name__].__class__ = _CallableModule
