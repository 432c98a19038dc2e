"""``esm_amd.pair_logits(model, tokens, head)`` and ``python -m esm_amd.pair_logits``: the pair logits of a linear head on the
attention maps (esm_amd/pair_head.py).  The module is callable, as ``esm_amd.design`` is."""
import sys

from .pair_head import main, pair_logits, parse_args  # noqa: F401


class _CallableModule(type(sys)):
    def __call__(self, *args, **kwargs):
        return pair_logits(*args, **kwargs)


if __name__ == "__main__":
    raise SystemExit(main())
else:
    sys.modules[__name__].__class__ = _CallableModule
