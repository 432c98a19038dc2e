"""Proteins longer than the model's window, end to end (esm_amd/windows.py; ``window=`` on the scoring methods,
``model.forward_windows``, ``--window`` on the three command lines) on the synthetic models of esm_amd/synth.py, L = 2, E = 128,
H = 2: ESM-1b built with max_positions = 40 (``window="max"`` is 40), ESM-2 with window 32, the original ESM-1 with window 32.
Every batch holds three sequences of 40, 41 and 97 tokens, padded to 97: for the ESM-1b model the first one fits, the second
is one over; windows of 32 cut all three, and a window of 40 shows on every model that a sequence that fits keeps its bits.

Every kernel of the forward is batch-invariant, so every comparison is bit for bit (``torch.equal``) with what the EXISTING API
gives the window copy alone — the copies, starts, grids and owners coming from the restatement of the definitions in
tests/_windows_ref.py — except the blend, which is held to (K + 2) 2^-23 max_k |x_k| per element of the fp64 blend of those same
per-window rows (tests/test_windows_ops_gpu.py)."""
import argparse
import csv
import functools

import numpy as np
import pytest
import torch

import _windows_ref as ref
import esm
from esm_amd import ops, scoring
from esm_amd.synth import esm1_args, synth_esm1_state_dict, synth_esm1b_state_dict, synth_esm2_state_dict

pytestmark = pytest.mark.gpu
L, E, H = 2, 128, 2
AAS = "ACDEFGHIKLMNPQRSTVWY"
TOKEN_LENGTHS = (40, 41, 97)


def esm1b_model(max_positions=40):
    args = argparse.Namespace(arch="roberta_large", layers=L, embed_dim=E, ffn_embed_dim=4 * E, attention_heads=H,
                              max_positions=max_positions, token_dropout=True, emb_layer_norm_before=True)
    model = esm.ProteinBertModel(args, esm.Alphabet.from_architecture("roberta_large")).eval()
    model.load_state_dict(synth_esm1b_state_dict(L, E, H, seed=5, max_positions=max_positions), strict=True)
    return model.cuda()


def esm2_model():
    model = esm.ESM2(L, E, H).eval()
    model.load_state_dict(synth_esm2_state_dict(L, E, H, seed=3))
    return model.cuda()


def esm1_model():
    model = esm.ProteinBertModel(esm1_args(L, E, H, final_bias=True, token_dropout=True),
                                 esm.Alphabet.from_architecture("protein_bert_base")).eval()
    model.load_state_dict(synth_esm1_state_dict(L, E, H, seed=7, final_bias=True), strict=True)
    return model.cuda()


KINDS = {"esm1b": (esm1b_model, "max", 40), "esm2": (esm2_model, 32, 32), "esm1": (esm1_model, 32, 32)}


class Case:
    def __init__(self, kind):
        make, self.window, self.Tw = KINDS[kind]
        self.kind = kind
        self.model = make()
        self.alphabet = self.model.alphabet
        self.h, self.t = int(self.model.prepend_bos), int(self.model.append_eos)
        g = torch.Generator().manual_seed(7)
        self.seqs = [(f"seq{n}", "".join(AAS[i] for i in torch.randint(0, 20, (n - self.h - self.t,), generator=g).tolist()))
                     for n in TOKEN_LENGTHS]
        _, _, toks = self.alphabet.get_batch_converter()(self.seqs)
        assert tuple(toks.shape) == (3, 97)
        self.cpu = toks
        self.tokens = toks.cuda()
        self.long = [b for b, n in enumerate(TOKEN_LENGTHS) if n > self.Tw]  # the sequences of the batch that are windowed
        self.tables = {}

    def geometry(self, b, wrap):
        return ref.geometry(TOKEN_LENGTHS[b], self.Tw, wrap, self.h, self.t)

    def copy(self, b, s, wrap):
        """The window copy of sequence b at start s, [1, Tw] on the device."""
        row = self.cpu[b, :TOKEN_LENGTHS[b]].tolist()
        copy = ref.window_copy(row, s, self.Tw, wrap, self.h, self.t, self.model.cls_idx, self.model.eos_idx)
        assert len(copy) == self.Tw
        return torch.tensor([copy], dtype=torch.int64).cuda()

    def windowed_table(self, wrap):
        """``masked_marginals(tokens, window=...)`` of the whole batch, computed once per wrap mode and left unchanged."""
        if wrap not in self.tables:
            self.tables[wrap] = self.model.masked_marginals(self.tokens, window=self.window, wrap=wrap)
        return self.tables[wrap]

    def window_batch(self, wrap, stride=None):
        """(win_tokens [nW, Tw] on the device, [(b, n, R, lo, hi, starts, w0)]): the grid windows of the long sequences,
        sequence-major, as ``forward_windows`` and ``wt_marginals`` run them."""
        rows, meta = [], []
        for b in self.long:
            R, lo, hi = self.geometry(b, wrap)
            starts = ref.grid(R, lo, hi, stride)
            meta.append((b, TOKEN_LENGTHS[b], R, lo, hi, starts, len(rows)))
            rows += [self.copy(b, s, wrap) for s in starts]
        return torch.cat(rows), meta

    def per_window(self, win, chunk, **kw):
        """``model(win[lo:hi], ...)`` in chunks of ``chunk`` windows, concatenated."""
        chunk = win.shape[0] if chunk is None else chunk  # the default chunk, 65536 // Tw windows, holds them all
        assert win.shape[0] <= max(1, 65536 // self.Tw)
        parts = [self.model(win[lo:lo + chunk], repr_layers=[0, 2], **kw) for lo in range(0, win.shape[0], chunk)]
        out = {"logits": torch.cat([p["logits"] for p in parts]),
               "representations": {l: torch.cat([p["representations"][l] for p in parts]) for l in (0, 2)}}
        if "contacts" in parts[0]:
            out["contacts"] = torch.cat([p["contacts"] for p in parts])
        return out

    def owner_rows(self, meta, wrap):
        """(b, p, flat window row) of every source row of the long sequences, by the owner rule."""
        hh = self.h if wrap else 0
        bs, ps, rows = [], [], []
        for b, n, R, lo, hi, starts, w0 in meta:
            for p in range(n):
                if p < lo:
                    w, col = 0, 0
                elif p >= hi:
                    w, col = len(starts) - 1, self.Tw - 1
                else:
                    w = ref.owner_of(p, starts, R)
                    col = p - starts[w] + hh
                bs.append(b)
                ps.append(p)
                rows.append((w0 + w) * self.Tw + col)
        return torch.tensor(bs).cuda(), torch.tensor(ps).cuda(), torch.tensor(rows).cuda()


@functools.lru_cache(maxsize=None)
def case(kind):
    return Case(kind)


ALL = list(KINDS)


def test_without_window_the_long_batch_is_refused_and_a_sequence_that_fits_keeps_its_bits():
    c = case("esm1b")
    with pytest.raises(ValueError, match="Sequence length 97 above maximum"):
        c.model(c.tokens)
    with pytest.raises(ValueError, match="Sequence length 97 above maximum"):
        c.model.masked_marginals(c.tokens)
    with pytest.raises(ValueError, match="Sequence length 97 above maximum"):
        c.model.wt_marginals(c.tokens)
    with pytest.raises(ValueError, match="above maximum"):
        c.model.masked_marginals(c.tokens, window=41)
    for kind in ALL:  # a window of 40 tokens: the first sequence fits on every model
        c = case(kind)
        short = c.tokens[0:1, :40].contiguous()
        table = c.windowed_table(True) if c.Tw == 40 else c.model.masked_marginals(c.tokens, window=40)
        assert torch.equal(table[0, :40], c.model.masked_marginals(short)[0]), kind
        assert not table[0, 40:].any() and table[1, :41].any() and table[2].any()
        assert torch.equal(c.model.wt_marginals(c.tokens, window=40)[0, :40], c.model.wt_marginals(short)[0]), kind
        got = c.model.forward_windows(c.tokens, repr_layers=[0, 2], window=40, return_contacts=True)
        alone = c.model(short, repr_layers=[0, 2], return_contacts=True)
        assert torch.equal(got["logits"][0, :40], alone["logits"][0]), kind
        for l in (0, 2):
            assert torch.equal(got["representations"][l][0, :40], alone["representations"][l][0]), (kind, l)
        S = 40 - c.h - c.t
        assert torch.equal(got["contacts"][0, :S, :S], alone["contacts"][0]), kind
        assert not got["contacts"][0, S:].any() and not got["contacts"][0, :, S:].any()
        assert not got["logits"][0, 40:].any()


@pytest.mark.parametrize("wrap", [True, False], ids=["wrapped", "raw"])
@pytest.mark.parametrize("kind", ALL)
def test_masked_marginals_rows_are_those_of_the_window_alone(kind, wrap):
    c = case(kind)
    got = c.windowed_table(wrap)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 97, c.model.alphabet_size)
    hh = c.h if wrap else 0
    loop = {}
    for b in c.long:
        n = TOKEN_LENGTHS[b]
        R, lo, hi = c.geometry(b, wrap)
        for p in range(n):
            if p < lo:  # the source's <cls>: column 0 of the first window
                s, col = lo, 0
            elif p >= hi:  # the source's <eos>: the last column of the last window
                s, col = hi - R, c.Tw - 1
            else:
                s = ref.start_of(p, R, lo, hi)
                col = p - s + hh
            if (b, s) not in loop:  # the existing API on the window copy alone: its B = 1 loop over the copy's positions
                loop[(b, s)] = c.model.masked_marginals(c.copy(b, s, wrap))[0]
            assert torch.equal(got[b, p], loop[(b, s)][col]), (kind, wrap, b, p, s)
        assert not got[b, n:].any()  # <pad> rows stay zero
    some = c.model.masked_marginals(c.tokens, positions=[[3], [0, 17, 40], [5, 50, 96]], window=c.window, wrap=wrap)
    want = torch.zeros_like(got)
    for b, ps in enumerate([[3], [0, 17, 40], [5, 50, 96]]):
        want[b, ps] = got[b, ps]
    assert torch.equal(some, want)


@pytest.mark.parametrize("kind", ALL)
def test_masked_joint_and_score_variants_across_a_grid_boundary(kind):
    c = case(kind)
    b, n = 2, 97
    R, lo, hi = c.geometry(b, True)
    starts = ref.grid(R, lo, hi)
    edge = starts[2]
    sites = [edge - 2, edge + 6]  # one site on either side of a grid start; their window is no grid window
    s = ref.start_of_set(sites, R, lo, hi)
    assert s not in starts
    off, pos, lp, logits = c.model.masked_joint(c.tokens, [sites, [3, 7], [10, 10 + R - 1]], src=[b, 0, b], window=c.window,
                                                return_logits=True)
    assert off.tolist() == [0, 2, 4, 6] and pos.tolist() == sites + [3, 7, 10, 10 + R - 1]
    _, _, want, want_logits = c.model.masked_joint(c.copy(b, s, True), [[p - s + c.h for p in sites]], return_logits=True)
    assert torch.equal(lp[0:2], want) and torch.equal(logits[0:2], want_logits)
    if 0 in c.long:
        R0, lo0, hi0 = c.geometry(0, True)
        s0 = ref.start_of_set([3, 7], R0, lo0, hi0)
        _, _, want = c.model.masked_joint(c.copy(0, s0, True), [[3 - s0 + c.h, 7 - s0 + c.h]])
    else:  # a set of a sequence that fits, in the same call: the unwindowed path
        _, _, want = c.model.masked_joint(c.tokens[0:1, :40].contiguous(), [[3, 7]])
    assert torch.equal(lp[2:4], want)
    # a set that spans exactly R tokens fits into one window only: the one that starts at its first position
    _, _, want = c.model.masked_joint(c.copy(b, 10, True), [[c.h, c.h + R - 1]])
    assert torch.equal(lp[4:6], want)
    with pytest.raises(ValueError, match="does not fit"):
        c.model.masked_joint(c.tokens, [[10, 10 + R]], src=[b], window=c.window)
    # score_variants: the fp64 sum, in ascending order of position, of the fp32 differences of those rows
    seq = c.seqs[b][1]
    i0, i1 = sites[0] - c.h, sites[1] - c.h
    m0, m1 = [next(a for a in AAS if a != seq[i]) for i in (i0, i1)]
    variants = [f"{seq[i1]}{i1 + 1}{m1}:{seq[i0]}{i0 + 1}{m0}", f"{seq[i0]}{i0 + 1}{m0}"]
    got = c.model.score_variants(c.alphabet, seq, variants, offset_idx=1, window=c.window)
    idx = c.alphabet.get_idx
    terms = [(lp[0, idx(m0)] - lp[0, idx(seq[i0])]).item(), (lp[1, idx(m1)] - lp[1, idx(seq[i1])]).item()]
    assert got[0] == 0.0 + terms[0] + terms[1]
    single = c.model.masked_marginals(c.tokens[b:b + 1], positions=[sites[0]], window=c.window)[0, sites[0]]
    assert got[1] == (single[idx(m0)] - single[idx(seq[i0])]).item()
    far = f"{seq[0]}1{'A' if seq[0] != 'A' else 'C'}:{seq[R]}{R + 1}{'A' if seq[R] != 'A' else 'C'}"
    with pytest.raises(ValueError, match="does not fit"):
        c.model.score_variants(c.alphabet, seq, [far], offset_idx=1, window=c.window)
    wt = c.model.score_variants(c.alphabet, seq, variants, strategy="wt-marginals", offset_idx=1, window=c.window)
    table = c.model.wt_marginals(c.tokens[b:b + 1], window=c.window)[0]
    t0, t1 = table[sites[0]], table[sites[1]]
    assert wt[0] == 0.0 + (t0[idx(m0)] - t0[idx(seq[i0])]).item() + (t1[idx(m1)] - t1[idx(seq[i1])]).item()


@pytest.mark.parametrize("kind,wrap", [(k, True) for k in ALL] + [("esm2", False)])
def test_wt_marginals_and_owner_stitch_are_the_owner_rows(kind, wrap):
    c = case(kind)
    win, meta = c.window_batch(wrap)
    bs, ps, rows = c.owner_rows(meta, wrap)
    V = c.model.alphabet_size
    table = c.model.wt_marginals(c.tokens, window=c.window, wrap=wrap)
    alone = c.model.wt_marginals(win).view(-1, V)  # the existing API on the window copies
    assert torch.equal(table[bs, ps], alone[rows])
    assert not table[1, 41:].any()
    if 0 not in c.long:
        assert torch.equal(table[0, :40], c.model.wt_marginals(c.tokens[0:1, :40].contiguous())[0])
    for chunk in (None, 2):
        got = c.model.forward_windows(c.tokens, repr_layers=[0, 2], window=c.window, wrap=wrap, chunk=chunk)
        want = c.per_window(win, chunk)
        assert sorted(got) == ["logits", "representations"] and sorted(got["representations"]) == [0, 2]
        assert tuple(got["logits"].shape) == (3, 97, V) and tuple(got["representations"][2].shape) == (3, 97, E)
        assert torch.equal(got["logits"][bs, ps], want["logits"].view(-1, V)[rows]), (kind, chunk)
        for l in (0, 2):
            assert torch.equal(got["representations"][l][bs, ps], want["representations"][l].view(-1, E)[rows]), (kind, chunk, l)
            assert not got["representations"][l][1, 41:].any()
    stride = c.model.forward_windows(c.tokens, repr_layers=[2], window=c.window, wrap=wrap, stride=7)
    win7, meta7 = c.window_batch(wrap, stride=7)
    bs, ps, rows = c.owner_rows(meta7, wrap)
    assert torch.equal(stride["representations"][2][bs, ps], c.per_window(win7, None)["representations"][2].view(-1, E)[rows])


@pytest.mark.parametrize("kind", ALL)
def test_blend_stitch_against_the_fp64_blend_of_the_window_rows(kind):
    c = case(kind)
    win, meta = c.window_batch(True)
    want = c.per_window(win, None)
    got = c.model.forward_windows(c.tokens, repr_layers=[0, 2], window=c.window, stitch="blend")
    owner = c.model.forward_windows(c.tokens, repr_layers=[0, 2], window=c.window)
    assert torch.equal(got["logits"], owner["logits"])  # logits are always owner rows
    off, src, w, where = [0], [], [], []
    for b, n, R, lo, hi, starts, w0 in meta:
        for p in range(lo, hi):
            for k, s in enumerate(starts):
                if s <= p < s + R:
                    src.append((w0 + k) * c.Tw + p - s + c.h)
                    w.append(ref.weight(p - s, R))
            off.append(len(src))
            where.append((b, p))
        for p in list(range(0, lo)) + list(range(hi, n)):  # the source's <cls> / <eos>: owner rows, never blended
            for l in (0, 2):
                assert torch.equal(got["representations"][l][b, p], owner["representations"][l][b, p])
    counts = np.diff(off)
    assert counts.min() == 1 and counts.max() >= 2
    bs, ps = torch.tensor([b for b, _ in where]).cuda(), torch.tensor([p for _, p in where]).cuda()
    for l in (0, 2):
        x = want["representations"][l].view(-1, E).cpu().numpy()
        blend, bound = ref.blend_ref(x, off, src, np.asarray(w, dtype=np.float32))
        mine = got["representations"][l][bs, ps].cpu().numpy()
        one = counts == 1
        assert np.array_equal(mine[one], blend[one].astype(np.float32)), "rows of one contributing window are copied"
        err = np.abs(mine.astype(np.float64) - blend)
        assert (err <= bound).all(), f"{kind} layer {l}: error {err.max():.3e} above the bound"


@pytest.mark.parametrize("kind", ALL)
def test_contact_maps_are_stitched_from_the_owner_windows(kind):
    c = case(kind)
    win, meta = c.window_batch(True)
    for chunk in (None, 2):
        got = c.model.forward_windows(c.tokens, window=c.window, return_contacts=True, chunk=chunk)["contacts"]
        S = 97 - c.h - c.t
        assert tuple(got.shape) == (3, S, S)
        maps = c.per_window(win, chunk, return_contacts=True)["contacts"]
        for b, n, R, lo, hi, starts, w0 in meta:
            Lb = hi - lo
            want = ref.stitch_contacts_ref(maps[w0:w0 + len(starts)].cpu().numpy(), starts, Lb, lo)
            mine = got[b, :Lb, :Lb].cpu().numpy()
            hole = np.isnan(want)
            assert np.array_equal(np.isnan(mine), hole), (kind, b, chunk)
            assert np.array_equal(mine[~hole].view(np.uint32), want[~hole].view(np.uint32)), (kind, b, chunk)
            assert hole.any() == (Lb > R) and not hole[np.arange(Lb), np.arange(Lb)].any()
            assert not got[b, Lb:].any() and not got[b, :, Lb:].any()  # beyond the sequence's own length: 0
    with pytest.raises(ValueError, match="wrap=True"):
        c.model.forward_windows(c.tokens, window=c.window, wrap=False, return_contacts=True)


@pytest.mark.parametrize("kind", ALL)
def test_pseudo_log_likelihood_is_the_sequential_sum(kind):
    c = case(kind)
    table = c.windowed_table(True).cpu()
    got = c.model.pseudo_log_likelihood(c.tokens, window=c.window)
    assert got.dtype == torch.float64 and tuple(got.shape) == (3,)
    for b, n in enumerate(TOKEN_LENGTHS):
        acc = 0.0
        for p in range(c.h, n - c.t):
            acc += table[b, p, c.cpu[b, p]].item()
        assert got[b].item() == acc, (kind, b)


@pytest.mark.parametrize("kind", ["esm1b", "esm2"])
def test_varlen_with_window_gives_the_same_tables(kind):
    c = case(kind)
    assert torch.equal(c.model.masked_marginals(c.tokens, window=c.window, varlen=True), c.windowed_table(True))
    assert torch.equal(c.model.wt_marginals(c.tokens, window=c.window, varlen=True), c.model.wt_marginals(c.tokens, window=c.window))
    assert torch.equal(c.model.pseudo_log_likelihood(c.tokens, window=c.window, varlen=True),
                       c.model.pseudo_log_likelihood(c.tokens, window=c.window))


def test_windowed_table_does_not_depend_on_the_run_or_the_chunks():
    c = case("esm2")
    first = c.windowed_table(True)
    assert torch.equal(c.model.masked_marginals(c.tokens, window=c.window), first)
    assert torch.equal(c.model.masked_marginals(c.tokens, window=c.window, chunk=1), first)


# ---- the command lines ----------------------------------------------------------------------------------------------------
def test_predict_cli_with_window_max(tmp_path, monkeypatch):
    from esm_amd import predict, pretrained

    c = case("esm1b")
    monkeypatch.setattr(pretrained, "load_model_and_alphabet", lambda location: (c.model, c.alphabet))
    seq = c.seqs[2][1]
    muts = [f"{seq[i]}{i + 1}{next(a for a in AAS if a != seq[i])}" for i in (0, 18, 47, 94)]
    src = tmp_path / "scan.csv"
    src.write_text("mutant\n" + "".join(f"{m}\n" for m in muts))
    tokens = c.tokens[2:3]
    want = {"masked-marginals": scoring.score_mutations(c.model.masked_marginals(tokens, window="max").cpu(), seq, muts, c.alphabet, 1),
            "wt-marginals": scoring.score_mutations(c.model.wt_marginals(tokens, window="max").cpu(), seq, muts, c.alphabet, 1)}
    for strategy, scores in want.items():
        out = tmp_path / f"{strategy}.csv"
        args = ["--model-location", "synth", "--sequence", seq, "--dms-input", str(src), "--dms-output", str(out), "--offset-idx", "1",
                "--scoring-strategy", strategy]
        with pytest.raises(ValueError, match="above maximum"):
            predict.main(args)
        assert predict.main(args + ["--window", "max"]) == 0
        rows = list(csv.DictReader(open(out, newline="")))
        assert [r["mutant"] for r in rows] == muts and [float(r["synth"]) for r in rows] == [float(s) for s in scores], strategy
    out = tmp_path / "raw.csv"
    assert predict.main(["--model-location", "synth", "--sequence", seq, "--dms-input", str(src), "--dms-output", str(out),
                         "--offset-idx", "1", "--scoring-strategy", "masked-marginals", "--window", "max", "--no-wrap"]) == 0
    raw = scoring.score_mutations(c.model.masked_marginals(tokens, window="max", wrap=False).cpu(), seq, muts, c.alphabet, 1)
    assert [float(r["synth"]) for r in csv.DictReader(open(out, newline=""))] == [float(s) for s in raw]


def test_score_sequences_cli_with_window(tmp_path):
    from esm_amd import score_sequences
    from esm_amd.synth import write_esm2_checkpoint

    c = case("esm2")
    path = write_esm2_checkpoint(str(tmp_path), "esm2_t2_synth", L, E, H, seed=3)
    fasta = tmp_path / "lib.fasta"
    fasta.write_text("".join(f">{label}\n{seq}\n" for label, seq in c.seqs))
    model, alphabet = esm.pretrained.load_model_and_alphabet(path)
    model = model.eval().cuda()
    want = model.pseudo_log_likelihood(c.cpu, varlen=True, window=32).tolist()
    out = tmp_path / "scored.csv"
    assert score_sequences.main(["--model-location", path, "--fasta", str(fasta), "--output", str(out), "--window", "32"]) == 0
    rows = list(csv.DictReader(open(out, newline="")))
    assert [r["label"] for r in rows] == [label for label, _ in c.seqs]
    assert [float(r["pll"]) for r in rows] == want
    assert want == c.model.pseudo_log_likelihood(c.tokens, window=32).tolist()  # the checkpoint holds the same weights
    # a window of 40: the first sequence fits and scores as without the option, the others do not
    plain, wide = tmp_path / "plain.csv", tmp_path / "wide.csv"
    assert score_sequences.main(["--model-location", path, "--fasta", str(fasta), "--output", str(plain)]) == 0
    assert score_sequences.main(["--model-location", path, "--fasta", str(fasta), "--output", str(wide), "--window", "40"]) == 0
    rows_plain, rows_wide = (list(csv.DictReader(open(f, newline=""))) for f in (plain, wide))
    assert rows_plain[0]["pll"] == rows_wide[0]["pll"] and rows_plain[2]["pll"] != rows_wide[2]["pll"]
    assert rows_plain[0]["pll"] != rows[0]["pll"]


def test_extract_cli_with_window(tmp_path):
    from esm_amd import extract
    from esm_amd.synth import write_esm2_checkpoint

    c = case("esm2")
    path = write_esm2_checkpoint(str(tmp_path), "esm2_t2_synth", L, E, H, seed=3)
    fasta = tmp_path / "lib.fasta"
    fasta.write_text("".join(f">{label}\n{seq}\n" for label, seq in c.seqs))
    out_dir = tmp_path / "out"
    extract.main([path, str(fasta), str(out_dir), "--repr_layers", "2", "--include", "mean", "per_tok", "contacts", "--window", "32"])
    assert c.long == [0, 1, 2]  # windows of 32 tokens cut all three
    for b in c.long:
        label, seq = c.seqs[b]
        n = len(seq)
        tokens = c.tokens[b:b + 1, :TOKEN_LENGTHS[b]].contiguous()
        want = c.model.forward_windows(tokens, repr_layers=[2], window=32, return_contacts=True)
        got = torch.load(out_dir / f"{label}.pt", weights_only=False)
        rep = want["representations"][2]
        assert torch.equal(got["representations"][2], rep[0, 1:n + 1].cpu())
        mean = ops.masked_row_mean(rep.contiguous(), torch.tensor([n], dtype=torch.int32).cuda(), first_row=1)
        assert torch.equal(got["mean_representations"][2], mean[0].cpu())
        ct = want["contacts"][0, :n, :n].cpu()
        assert tuple(got["contacts"].shape) == (n, n)
        assert torch.equal(torch.isnan(got["contacts"]), torch.isnan(ct))
        assert torch.equal(torch.nan_to_num(got["contacts"]), torch.nan_to_num(ct))
        assert bool(torch.isnan(ct).any()) == (n > 30)
    # a window of 40 tokens, blended: the first sequence fits and goes with the regular batches, as without --window
    plain, wide = tmp_path / "plain", tmp_path / "wide"
    extract.main([path, str(fasta), str(plain), "--repr_layers", "2", "--include", "per_tok"])
    extract.main([path, str(fasta), str(wide), "--repr_layers", "2", "--include", "per_tok", "--window", "40",
                  "--window-stitch", "blend", "--window-stride", "9"])
    name = f"{c.seqs[0][0]}.pt"
    a, b = torch.load(plain / name, weights_only=False), torch.load(wide / name, weights_only=False)
    assert tuple(a["representations"][2].shape) == (38, E) and torch.equal(a["representations"][2], b["representations"][2])
    want = c.model.forward_windows(c.tokens[2:3], repr_layers=[2], window=40, stride=9, stitch="blend")["representations"][2]
    got = torch.load(wide / f"{c.seqs[2][0]}.pt", weights_only=False)["representations"][2]
    assert tuple(got.shape) == (95, E) and torch.equal(got, want[0, 1:96].cpu())
