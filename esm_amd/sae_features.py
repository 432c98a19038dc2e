"""``esm_amd.sae_features(model, tokens, sae, layer)`` and ``python -m esm_amd.sae_features``: the sparse-autoencoder features of
a representation (esm_amd/sae.py).  The module is callable, as ``esm_amd.design`` and ``esm_amd.pair_logits`` are."""
import sys

from .sae import main, parse_args, sae_features  # noqa: F401


class _CallableModule(type(sys)):
    def __call__(self, *args, **kwargs):
        return sae_features(*args, **kwargs)


if __name__ == "__main__":
    raise SystemExit(main())
else:
    sys.modules[__name__].__class__ = _CallableModule
