"""Query-anchored a3m alignments from the hits of an embedding search, on the MI355X (esm_amd/msa_build.py):

    python -m esm_amd.build_msa --model-location M --index db.npz --query Q.fasta --output-dir DIR [--top 1024] [--depth N]
        [--min-coverage 0.5] [--max-identity 0.9] [--min-query-identity 0] [--subsample first|greedy|weighted|uniform]
        [--mode local|global] [--gap-open o] [--gap-extend e] [--no-enhance] [--no-insertions] [--summary OUT.tsv]

One ``<label>.a3m`` per query, the file ``predict_msa --msa-path`` and ``subsample_msa --msa-path`` read.
"""
import sys
import types

from .msa_build import main, parse_args  # noqa: F401


class _CallableModule(types.ModuleType):
    """``esm_amd.build_msa`` names both this command-line module and the function ``esm_amd.msa_build.build_msa`` that the
    package exports; importing the module rebinds the package attribute to it, so the module forwards calls."""

    def __call__(self, *args, **kwargs):
        from .msa_build import build_msa

        return build_msa(*args, **kwargs)


if __name__ == "__main__":
    sys.exit(main())
else:
    sys.modules[__name__].__class__ = _CallableModule
