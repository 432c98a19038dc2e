"""The background of lm-design's n-gram term (``esm_amd.design``: ``w_ngram``, ``ngram``): per order n a dense fp64 table of the
probability of every n-gram over an alphabet, counted from sequences of the caller's choice.

The reference keeps its background as pickled dictionaries next to its code (``examples/lm-design/utils/ngram_stats/*.p``) and turns
them into probabilities on import: the n-grams inside its 20 letters are counted, ``q = max(count / total, 1e-5)``, and a key the
dictionary does not hold reads as ``1e-5`` (``utils/ngram.py``).  ``Background.from_sequences`` does the same from sequences, and the
tables are dense — key = sum_k code[k] * A^(n-1-k), the first residue most significant — so that the device op
(``esmk_op_ngram_energy``) indexes them directly.  No pickle is read and no table ships with the project:

    python -m esm_amd.ngram_table --fasta uniref_sample.fasta --output bg.npz
    python -m esm_amd.design ... --w-ngram 1 --ngram-table bg.npz
"""
import numpy as np

STANDARD_ALPHABET = "ACDEFGHIKLMNPQRSTVWY"
MAX_ORDER = 4  # of esmk_op_ngram_energy
MAX_LETTERS = 32


def _codes(seq, alphabet):
    """int64 [len(seq)]: the index of every character in ``alphabet``, -1 outside it."""
    lut = np.full(256, -1, dtype=np.int64)
    for i, ch in enumerate(alphabet):
        lut[ord(ch)] = i
    raw = np.frombuffer(seq.encode("latin-1", "replace"), dtype=np.uint8)
    return lut[raw]


def window_keys(codes, n, A):
    """The keys of the valid windows of order ``n`` of one coded sequence, in window order (int64)."""
    codes = np.asarray(codes, dtype=np.int64)
    W = codes.shape[0] - n + 1
    if W <= 0:
        return np.zeros((0,), dtype=np.int64)
    key = np.zeros((W,), dtype=np.int64)
    valid = np.ones((W,), dtype=bool)
    for k in range(n):
        part = codes[k: k + W]
        valid &= part >= 0
        key = key * A + part
    return key[valid]


class Background:
    """``alphabet`` (a string of A <= 32 distinct letters), ``orders`` (ascending, within 1 .. 4) and ``tables``: order n -> fp64
    ``[A^n]`` of positive probabilities."""

    def __init__(self, alphabet, tables):
        alphabet = str(alphabet)
        if not 1 <= len(alphabet) <= MAX_LETTERS or len(set(alphabet)) != len(alphabet) or any(ord(c) > 255 for c in alphabet):
            raise ValueError(f"alphabet: 1 .. {MAX_LETTERS} distinct one-byte letters")
        A = len(alphabet)
        self.alphabet = alphabet
        self.tables = {}
        for n in sorted(int(n) for n in tables):
            if not 1 <= n <= MAX_ORDER:
                raise ValueError(f"n-gram order {n}: one of 1 .. {MAX_ORDER}")
            q = np.ascontiguousarray(np.asarray(tables[n], dtype=np.float64).reshape(-1))
            if q.shape[0] != A ** n:
                raise ValueError(f"the table of order {n} has {q.shape[0]} entries, not {A} ** {n}")
            if not bool((np.isfinite(q) & (q > 0.0)).all()):
                raise ValueError(f"the table of order {n} holds an entry that is not finite and positive (apply a floor)")
            self.tables[n] = q
        if not self.tables:
            raise ValueError("a background needs the table of at least one order")
        self.orders = tuple(self.tables)

    @classmethod
    def from_sequences(cls, seqs, orders=(1, 2, 3), alphabet=STANDARD_ALPHABET, floor=1e-5):
        """Counts the n-grams of the windows inside ``alphabet`` over ``seqs`` (strings): ``q = max(count / total, floor)`` with
        ``total`` the counted windows of that order, and ``floor`` for a key no window has."""
        floor = float(floor)
        if not (0.0 < floor < float("inf")):
            raise ValueError("floor must be positive and finite: every entry of a table is divided by")
        orders = sorted(set(int(n) for n in orders))
        if not orders or orders[0] < 1 or orders[-1] > MAX_ORDER:
            raise ValueError(f"orders: at least one of 1 .. {MAX_ORDER}")
        A = len(alphabet)
        counts = {n: np.zeros((A ** n,), dtype=np.int64) for n in orders}
        for seq in seqs:
            codes = _codes(seq, alphabet)
            for n in orders:
                counts[n] += np.bincount(window_keys(codes, n, A), minlength=A ** n)
        tables = {}
        for n in orders:
            total = int(counts[n].sum())
            q = counts[n].astype(np.float64) / np.float64(total) if total > 0 else np.zeros((A ** n,), dtype=np.float64)
            tables[n] = np.maximum(q, floor)
        return cls(alphabet, tables)

    def save(self, path):
        """An ``.npz`` file: ``alphabet``, ``orders`` and ``q<n>`` per order; plain arrays, nothing pickled."""
        arrays = {"alphabet": np.frombuffer(self.alphabet.encode("latin-1"), dtype=np.uint8),
                  "orders": np.asarray(self.orders, dtype=np.int64)}
        for n, q in self.tables.items():
            arrays[f"q{n}"] = q
        with open(path, "wb") as fh:
            np.savez(fh, **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            alphabet = bytes(z["alphabet"].astype(np.uint8)).decode("latin-1")
            return cls(alphabet, {int(n): z[f"q{int(n)}"] for n in z["orders"]})

    def token_codes(self, alphabet):
        """int32 [V]: the code of every token of a model ``alphabet`` (``esm.Alphabet``) — the index of a one-letter token in this
        background's alphabet, -1 for every other token."""
        code = np.full((len(alphabet.all_toks),), -1, dtype=np.int32)
        for i, tok in enumerate(alphabet.all_toks):
            if len(tok) == 1 and tok in self.alphabet:
                code[i] = self.alphabet.index(tok)
        return code

    def subset(self, orders):
        """The background of some of its orders."""
        return Background(self.alphabet, {int(n): self.tables[int(n)] for n in orders})
