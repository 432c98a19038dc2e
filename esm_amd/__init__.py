"""esm_amd — an MI355X (gfx950) native forward engine for ESM-2 behind the public Python surface
of facebookresearch/esm.  ``import esm`` (the shim package next to this one) re-exports the same
names, so reference scripts such as ``scripts/extract.py`` run unchanged.

Importing this package does not load the HIP library; ``esm_amd._native`` does, on the first
forward (or explicitly), and raises if libesmk.so is missing — there is no CPU fallback.
"""
from .alphabet import Alphabet, BatchConverter, MSABatchConverter  # noqa: F401
from .fasta import FastaBatchedDataset, read_alignment_lines, read_fasta, read_msa  # noqa: F401
from .esm2 import ESM2  # noqa: F401
from . import checkpoint as pretrained  # noqa: F401
from .scoring import (masked_joint, masked_marginals, parse_variant, pseudo_log_likelihood, score_mutations,  # noqa: F401
                      score_variants, wt_marginals)
from .msa_scoring import (msa_forward_rows, msa_masked_joint, msa_masked_marginals, msa_score_variants,  # noqa: F401
                          msa_score_variants_ensemble, msa_wt_marginals)
from .msa_select import (encode_msa, msa_mismatches, msa_neff, msa_neighbor_counts, msa_sequence_weights,  # noqa: F401
                         subsample_indices, subsample_msa)

from .sampling import gibbs_sample, inpaint  # noqa: F401
from .jacobian import categorical_jacobian, jacobian_contacts  # noqa: F401
from .windows import forward_windows  # noqa: F401
from .interventions import StreamEdit, forward_edited, mean_difference, stream_edits  # noqa: F401
from .pair_head import PairHead, distogram_bins, distogram_from_pdb  # noqa: F401
from .sae import SparseAutoencoder  # noqa: F401


def __getattr__(name):
    # esm_amd.design is the design module, which is callable as its own main function (``esm_amd.design(model, tokens, ...)``
    # is ``esm_amd.design.design``); loaded on first use, so that ``python -m esm_amd.design`` runs a module not yet imported
    if name in ("design", "design_energy", "contacts_from_pdb", "DistogramTarget"):
        import importlib

        module = importlib.import_module(".design", __name__)
        return module if name == "design" else getattr(module, name)
    if name == "pair_logits":  # likewise a module that is its own main function (``python -m esm_amd.pair_logits``)
        import importlib

        return importlib.import_module(".pair_logits", __name__)
    if name == "sae_features":  # and ``python -m esm_amd.sae_features``
        import importlib

        return importlib.import_module(".sae_features", __name__)
    if name in ("align", "align_embeddings", "alignment_strings"):  # esm_amd/align.py, also ``python -m esm_amd.align``
        import importlib

        module = importlib.import_module(".align", __name__)
        return module if name == "align" else getattr(module, name)
    if name in ("search", "EmbeddingIndex", "search_and_align"):  # esm_amd/search.py, also ``python -m esm_amd.search``
        import importlib

        module = importlib.import_module(".search", __name__)
        return module if name == "search" else getattr(module, name)
    if name in ("cluster", "cluster_embeddings"):  # esm_amd/cluster.py, also ``python -m esm_amd.cluster``
        import importlib

        module = importlib.import_module(".cluster", __name__)
        return module if name == "cluster" else getattr(module, name)
    if name == "build_msa":  # esm_amd/build_msa.py: ``python -m esm_amd.build_msa``, and callable as msa_build.build_msa
        import importlib

        return importlib.import_module(".build_msa", __name__)
    if name in ("msa_build", "build_msas", "BuiltMSA"):  # esm_amd/msa_build.py: search hits to a query-anchored MSA
        import importlib

        module = importlib.import_module(".msa_build", __name__)
        return module if name == "msa_build" else getattr(module, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__version__ = "0.1.0"
