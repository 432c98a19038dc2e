"""Regenerate tests/golden/msa_select_greedy.json: the rows the reference's own ``greedy_select`` keeps.

    python tests/golden/make_golden_msa_select.py --notebook <facebookresearch/esm checkout>/examples/contact_prediction.ipynb

The function is read out of the notebook's "Subsampling MSA" cell AT RUN TIME and executed (numpy and scipy's ``cdist``
needed); nothing of the cell is copied into this repository.  It is run on the generator alignment of tests/_msa_select_ref.py
(257 x 64, seed 0) at ``num_seqs`` 32 for ``max`` and ``min``, and the indices of the records it returns are recorded.  At L = 64
the notebook's float means of count / 64 are exact, so the engine's integer rule has to reproduce both lists
(tests/test_msa_select_cpu.py, tests/test_msa_select_gpu.py)."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

N, L, SEED, NUM = 257, 64, 0, 32


def notebook_function(path, name="greedy_select"):
    with open(path) as fh:
        book = json.load(fh)
    for cell in book["cells"]:
        src = "".join(cell.get("source", []))
        if cell.get("cell_type") == "code" and f"def {name}(" in src:
            import typing

            import numpy as np
            from scipy.spatial.distance import cdist

            space = {"np": np, "cdist": cdist}
            space.update({k: getattr(typing, k) for k in ("List", "Tuple", "Optional", "Dict", "Union", "Callable")})
            exec(compile(src, f"{path}:{name}", "exec"), space)
            return space[name]
    raise SystemExit(f"no code cell of {path} defines {name}")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--notebook", required=True, help="examples/contact_prediction.ipynb of the reference")
    ap.add_argument("--output", default=os.path.join(HERE, "msa_select_greedy.json"))
    args = ap.parse_args(argv)
    import _msa_select_ref as M

    select = notebook_function(args.notebook)
    msa = M.records(M.family_msa(N, L, SEED))
    label_row = {label: i for i, (label, _) in enumerate(msa)}
    out = {"generator": {"n": N, "L": L, "seed": SEED}, "num_seqs": NUM}
    for mode in ("max", "min"):
        out[mode] = [label_row[label] for label, _ in select(msa, NUM, mode=mode)]
        assert len(out[mode]) == NUM and out[mode] == sorted(set(out[mode]))
    with open(args.output, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(args.output)


if __name__ == "__main__":
    main()
