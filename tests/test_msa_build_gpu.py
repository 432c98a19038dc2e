"""``build_msa`` / ``build_msas`` (esm_amd/msa_build.py) through the synthetic ESM-2 of esm_amd/synth.py (L = 3, E = 128) on a
planted family: the device pipeline against the references of tests/_msa_build_ref.py applied to the same ``search_and_align``
output — exactly, in ``msa``, ``stats``, ``hit_ids``, ``scores`` and row order — at filter settings chosen from the reference's
own numbers so that each filter drops and keeps something; the depth cut, several identity blocks, two queries at once, the
tokens and the a3m file into a synthetic MSA Transformer, and the command line."""
import argparse
import functools

import numpy as np
import pytest
import torch

import _msa_build_ref as ref
import esm
import esm_amd
from esm_amd import msa_build as MB
from esm_amd import search as S
from esm_amd.synth import synth_esm2_state_dict, synth_msa_state_dict

pytestmark = pytest.mark.gpu
ALPHABET = esm.Alphabet.from_architecture("ESM-1b")
AA = list("ACDEFGHIKLMNPQRSTVWY")


def mutate(rng, seq, rate):
    return "".join(str(rng.choice([a for a in AA if a != ch])) if rng.random() < rate else ch for ch in seq)


@functools.lru_cache(maxsize=None)
def world():
    """(model, index on the device, queries, the search_and_align output on the host).  The database: two planted families —
    each a query's copies with substitutions, a truncation, an internal insertion, an internal deletion and an exact
    duplicate — and unrelated random sequences, 40 records of 20 .. 60 residues."""
    rng = np.random.default_rng(2024)
    rand = lambda n: "".join(rng.choice(AA, size=n))
    queries = [("query0", rand(48)), ("query1", rand(37))]
    db = []
    for k, (_, q) in enumerate(queries):
        n = len(q)
        fam = [(f"f{k}_sub{int(100 * r)}{v}", mutate(rng, q, r)) for r in (0.15, 0.3, 0.45) for v in "ab"][:6 if k == 0 else 3]
        m = mutate(rng, q, 0.25)
        fam.append((f"f{k}_trunc", m[n // 5:n // 5 + (3 * n) // 5]))
        m = mutate(rng, q, 0.2)
        fam.append((f"f{k}_ins", m[:n // 2] + rand(5) + m[n // 2:]))
        m = mutate(rng, q, 0.2)
        fam.append((f"f{k}_del", m[:n // 3] + m[n // 3 + 7:]))
        fam.append((f"f{k}_dup", q))
        db += fam
    db += [(f"u{i}", rand(int(rng.integers(20, 61)))) for i in range(40 - len(db))]
    order = rng.permutation(len(db))
    db = [db[i] for i in order]
    assert len(db) == 40 and all(20 <= len(s) <= 60 for _, s in db)
    model = esm.ESM2(3, 128, 2).eval()
    model.load_state_dict(synth_esm2_state_dict(3, 128, 2, seed=11), strict=True)
    model = model.cuda()
    index = S.EmbeddingIndex.build(model, ALPHABET, db, layer=2, model_name="synth").to("cuda")
    out = esm_amd.search_and_align(model, ALPHABET, queries, index, top_k=40, mode="local", enhance=True)["alignment"]
    host = {k: v.cpu().numpy() for k, v in out.items()}
    return model, index, queries, host


def reference(q, **kw):
    """(rows in rank order, msa, stats, passed, hit ids with -1 in front, scores with +inf in front, the hits' sequences, the
    query's slice of col_offsets) of query q by tests/_msa_build_ref.py on the aligner's output."""
    _, index, queries, al = world()
    sel = np.nonzero(al["pairs"][:, 0] == q)[0]
    p0, p1 = int(sel[0]), int(sel[-1]) + 1
    ids = al["pairs"][p0:p1, 1]
    seqs = [index.sequences[t] for t in ids]
    offs = al["col_offsets"][p0:p1 + 1]
    rows, msa, stats, passed = ref.build(queries[q][1], seqs, al["score"][p0:p1], al["cols"], offs, **kw)
    return (rows, msa, stats, passed, np.concatenate([[-1], ids]).astype(np.int32),
            np.concatenate([[np.inf], al["score"][p0:p1]]).astype(np.float32), seqs, offs)


def check(built, q, rows, what, **kw):
    _, index, queries, _ = world()
    _, msa, stats, _, ids, scores, _, _ = reference(q, **kw)
    assert built.msa.dtype == torch.uint8 and built.msa.is_cuda and built.msa.is_contiguous()
    assert built.hit_ids.cpu().tolist() == ids[rows].tolist(), what  # the rows and their order
    assert np.array_equal(built.msa.cpu().numpy(), msa[rows]), what
    assert np.array_equal(built.stats.cpu().numpy(), stats[rows]), what
    assert np.array_equal(built.scores.cpu().numpy().view(np.int32), scores[rows].view(np.int32)), what
    assert built.labels == [queries[q][0]] + [index.labels[t] for t in ids[rows][1:]], what
    assert built.hit_ids.dtype == torch.int32 and built.stats.dtype == torch.int32 and built.scores.dtype == torch.float32


def chosen_settings(q):
    """(min_coverage, max_identity) from the reference's numbers on the planted set: a coverage between two neighbouring
    values of n_match / Lq, and an identity at which the walk drops and keeps, each leaving at least three hits and
    dropping at least one."""
    _, _, queries, _ = world()
    Lq = len(queries[q][1])
    _, msa, stats, _, _, _, _, _ = reference(q, min_coverage=0.0, max_identity=None)
    nm = np.sort(stats[1:, 0])[::-1]
    steps = [k for k in range(3, len(nm)) if nm[k] < nm[k - 1] and nm[k - 1] >= 1]  # k hits stay, the others go
    k = next((k for k in steps if k >= 6), steps[0])
    min_coverage = (int(nm[k]) + int(nm[k - 1])) / 2.0 / Lq
    rows, _, _, passed = reference(q, min_coverage=min_coverage, max_identity=None)[:4]
    assert len(rows) - 1 == k and int((~passed).sum()) == len(nm) - k
    ident = ref.pair_identity(msa, Lq, ref.GAP, 8)
    found = {}
    for t in sorted({float(v) for v in ident[rows][:, rows].ravel() if 0.0 < v < 1.0}, reverse=True):
        kept = ref.redundancy_walk(ident, rows, t)
        if len(kept) - 1 >= 3 and len(kept) < len(rows):
            found.setdefault(len(rows) - len(kept) >= 2, t)  # preferred: the duplicate and at least one more hit go
    assert found, "no identity threshold drops and keeps on the planted set"
    return min_coverage, found.get(True, found.get(False))


def test_build_msa_equals_the_reference():
    model, index, queries, al = world()
    for q in (0, 1):
        dup = index.labels.index(f"f{q}_dup")
        assert dup in al["pairs"][al["pairs"][:, 0] == q, 1]
        # the defaults
        built = model.build_msa(ALPHABET, queries[q], index, top_k=40)
        rows, _, stats, passed, ids, _, _, _ = reference(q)
        check(built, q, rows, (q, "defaults"))
        assert dup not in built.hit_ids.cpu().tolist() and passed[1 + ids[1:].tolist().index(dup)]  # covered by the query
        assert built.hit_ids[0] == -1 and bytes(built.msa[0].cpu().numpy()).decode() == queries[q][1]
        assert built.counts["hits"] == 40 and int(built.counts["after_row_filter"]) == int(passed.sum())
        assert built.counts["after_redundancy_filter"] == built.counts["kept"] == len(rows) == len(built)
        print(f"query {q}: defaults keep {len(rows) - 1} of 40 hits, {int(passed.sum()) - 1} pass the row filter")
        # each filter at a value that drops and keeps
        min_coverage, max_identity = chosen_settings(q)
        kw = dict(min_coverage=min_coverage, max_identity=max_identity)
        rows, _, _, passed = reference(q, **kw)[:4]
        n_cov = int(passed.sum()) - 1
        assert 3 <= len(rows) - 1 <= n_cov - 1 and n_cov <= 39  # each filter drops at least one hit and keeps at least three
        print(f"query {q}: min_coverage {min_coverage:.4f} keeps {n_cov} of 40, max_identity {max_identity:.4f} keeps {len(rows) - 1} of those")
        built = esm_amd.build_msa(model, ALPHABET, queries[q], index, top_k=40, **kw)
        check(built, q, rows, (q, kw), **kw)
        assert dup not in built.hit_ids.cpu().tolist()
        # the row filter alone, the query identity, no overlap floor
        for kw in (dict(max_identity=None, min_coverage=min_coverage), dict(min_query_identity=0.5, min_coverage=0.2, max_identity=1.0),
                   dict(min_coverage=0.0, min_overlap=1, max_identity=0.6)):
            built = esm_amd.build_msa(model, ALPHABET, queries[q], index, top_k=40, **kw)
            check(built, q, reference(q, **kw)[0], (q, kw), **kw)
        rows = reference(q, max_identity=None, min_coverage=min_coverage)[0]
        assert dup in [int(reference(q)[4][r]) for r in rows]  # without the redundancy filter the duplicate stays


def test_depth_first_and_greedy():
    model, index, queries, _ = world()
    kw = dict(min_coverage=0.0, max_identity=None)
    rows, msa, _, _, _, _, _, _ = reference(0, **kw)
    assert len(rows) > 12
    built = model.build_msa(ALPHABET, queries[0], index, top_k=40, depth=12, **kw)
    check(built, 0, rows[:12], "first", **kw)
    assert built.counts["after_redundancy_filter"] == len(rows) and built.counts["kept"] == 12
    pick = esm_amd.subsample_indices(torch.from_numpy(msa[rows]).cuda(), 12, strategy="greedy")
    assert pick[0] == 0 and len(pick) == 12 and pick != list(range(12))
    built = model.build_msa(ALPHABET, queries[0], index, top_k=40, depth=12, subsample="greedy", **kw)
    check(built, 0, [rows[i] for i in pick], "greedy", **kw)
    check(model.build_msa(ALPHABET, queries[0], index, top_k=40, depth=1000, **kw), 0, rows, "deeper than the rows", **kw)
    check(model.build_msa(ALPHABET, queries[0], index, top_k=40, depth=1, **kw), 0, rows[:1], "the query alone", **kw)


def test_identity_blocks_and_two_queries():
    model, index, queries, _ = world()
    kw = dict(min_coverage=0.1, max_identity=0.7)
    rows = reference(0, **kw)[0]
    for max_bytes in (44 * 4 * 7, 1):  # blocks of 7 rows and of one row of the 41
        assert len(MB.identity_blocks(41, max_bytes)) in (6, 41)
        check(model.build_msa(ALPHABET, queries[0], index, top_k=40, max_bytes=max_bytes, **kw), 0, rows, ("max_bytes", max_bytes), **kw)
    both = model.build_msas(ALPHABET, queries, index, top_k=40, **kw)
    assert len(both) == 2
    for q in (0, 1):
        one = model.build_msa(ALPHABET, queries[q], index, top_k=40, **kw)
        check(both[q], q, reference(q, **kw)[0], ("build_msas", q), **kw)
        assert torch.equal(one.msa, both[q].msa) and torch.equal(one.hit_ids, both[q].hit_ids) and one.labels == both[q].labels
        assert one.a3m_lines() == both[q].a3m_lines()
    # fewer hits than the database; a query without hits that pass is the query alone
    few = model.build_msa(ALPHABET, queries[0], index, top_k=5, **kw)
    assert few.counts["hits"] == 5 and few.hit_ids[0] == -1
    alone = model.build_msa(ALPHABET, queries[0], index, top_k=40, min_coverage=1.0, min_query_identity=1.0, max_identity=0.0)
    assert len(alone) == 1 and alone.records() == [queries[0]]


def test_tokens_and_file_into_the_msa_transformer(tmp_path):
    model, index, queries, _ = world()
    built = model.build_msa(ALPHABET, queries[0], index, top_k=40, min_coverage=0.3, depth=8)
    assert 3 <= len(built) <= 8
    rows, _, _, _, ids, _, seqs, offs = reference(0, min_coverage=0.3)
    rows = rows[:8]
    path = tmp_path / "q0.a3m"
    built.write_a3m(path)
    _, _, _, al = world()
    paths = [al["cols"][offs[r - 1]:offs[r]] for r in rows[1:]]
    text = ref.a3m_text(built.labels, [r for _, r in built.records()], [seqs[r - 1] for r in rows[1:]], paths)
    assert open(path).read() == text
    back = esm_amd.read_msa(path)
    assert back == built.records()
    args = argparse.Namespace(layers=2, embed_dim=128, ffn_embed_dim=256, attention_heads=2, dropout=0.1, attention_dropout=0.1,
                              activation_dropout=0.1, max_positions=1024, embed_positions_msa=True, embed_positions_msa_dim=128,
                              max_tokens=2 ** 14, max_tokens_per_msa=2 ** 14)
    msa_alphabet = esm.Alphabet.from_architecture("msa_transformer")
    msa_model = esm.MSATransformer(args, msa_alphabet).eval()
    msa_model.load_state_dict(synth_msa_state_dict(2, 128, 2, 256, seed=1), strict=True)
    msa_model = msa_model.cuda()
    tok = built.tokens(msa_alphabet)
    assert tok.is_cuda and tuple(tok.shape) == (1, len(built), len(queries[0][1]) + 1)
    assert torch.equal(tok.cpu(), msa_alphabet.get_batch_converter()(back)[2])
    wt = queries[0][1]
    variants = [f"{wt[3]}4{'A' if wt[3] != 'A' else 'C'}", f"{wt[10]}11{'W' if wt[10] != 'W' else 'Y'}:{wt[20]}21{'K' if wt[20] != 'K' else 'R'}"]
    direct = msa_model.msa_score_variants(msa_alphabet, built.records(), variants, offset_idx=1)
    via_file = msa_model.msa_score_variants(msa_alphabet, back, variants, offset_idx=1)
    assert direct == via_file and all(np.isfinite(direct))
    table = esm_amd.msa_masked_marginals(msa_model, tok, positions=[4])  # the device tokens as they stand
    want = esm_amd.msa_masked_marginals(msa_model, msa_alphabet.get_batch_converter()(back)[2], positions=[4])
    assert torch.equal(table, want)
    assert esm_amd.msa_neff(built.msa) > 0 and len(esm_amd.subsample_msa(built.msa, 2)) == 2


def test_command_line(tmp_path, monkeypatch):
    from esm_amd import checkpoint

    model, index, queries, _ = world()
    other = esm.ESM2(3, 96, 6).eval()
    monkeypatch.setattr(checkpoint, "load_model_and_alphabet", lambda location: ({"synth": model, "other": other}[location], ALPHABET))
    npz, out_dir, summary = str(tmp_path / "db.npz"), tmp_path / "msas", str(tmp_path / "summary.tsv")
    index.save(npz)
    (tmp_path / "q.fa").write_text("".join(f">{label} a description\n{seq}\n" for label, seq in queries))
    base = ["--model-location", "synth", "--index", npz, "--query", str(tmp_path / "q.fa"), "--output-dir", str(out_dir)]
    assert MB.main(base + ["--top", "40", "--min-coverage", "0.3", "--max-identity", "0.8", "--depth", "9", "--summary", summary]) == 0
    built = model.build_msas(ALPHABET, queries, index, top_k=40, min_coverage=0.3, max_identity=0.8, depth=9)
    lines = [ln.split("\t") for ln in open(summary).read().splitlines()]
    assert lines[0] == list(MB.SUMMARY_HEADER) and len(lines) == 3
    for q, b in enumerate(built):
        assert open(out_dir / f"{queries[q][0]}.a3m").read() == "\n".join(b.a3m_lines()) + "\n"
        assert esm_amd.read_msa(out_dir / f"{queries[q][0]}.a3m") == b.records()
        rows, _, _, passed = reference(q, min_coverage=0.3, max_identity=0.8)[:4]
        assert lines[1 + q] == [queries[q][0], "40", str(int(passed.sum())), str(len(rows)), str(min(len(rows), 9)), f"{esm_amd.msa_neff(b.msa):.3f}"]
    assert MB.main(base + ["--top", "40", "--no-insertions", "--mode", "global", "--no-enhance", "--gap-open", "2"]) == 0
    b = model.build_msa(ALPHABET, queries[0], index, top_k=40, mode="global", enhance=False, gap_open=2.0)
    assert open(out_dir / "query0.a3m").read() == "\n".join(b.a3m_lines(insertions=False)) + "\n"
    with pytest.raises(ValueError, match="embed_dim = 128, the model has embed_dim = 96"):
        MB.main(["--model-location", "other"] + base[2:])
    bare = S.EmbeddingIndex(index.vectors, index.labels, index.lengths, None, index.meta)
    bare.save(npz)
    with pytest.raises(ValueError, match="no sequences"):
        MB.main(base)
