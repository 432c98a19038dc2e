"""Free end gaps and several hits per pair end to end (esm_amd/align.py, esm_amd/msa_build.py): ``align_embeddings`` against the
numpy reference on the similarity the call itself computed, blocks against one block, the defaults against a call without the
new keywords, the MSA rows of two hits of one target, and ``model.align`` on the tiny synthetic ESM-2."""
import numpy as np
import pytest
import torch

import _align_free_ref as fr
import esm
import esm_amd
from esm_amd import align as A
from esm_amd import msa_build as MB
from esm_amd.synth import synth_esm2_state_dict, synth_tokens

pytestmark = pytest.mark.gpu
E = 64
LEN_A, LEN_B = [7, 64, 1, 65], [130, 1, 65, 7, 64]
PATH_KEYS = ("score", "end", "start", "n_cols", "n_match", "col_offsets", "cols")


def reps(seed=0):
    g = torch.Generator().manual_seed(seed)
    return ([torch.randn((n, E), generator=g).cuda() for n in LEN_A], [torch.randn((n, E), generator=g).cuda() for n in LEN_B])


def same(a, b, keys=PATH_KEYS, what=""):
    for key in keys:
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype, (what, key)
        assert torch.equal(a[key], b[key]), (what, key)


def check_against_reference(out, sims, mode, mask, K):
    """every entry of ``out`` against ``hits()`` on the pair's similarity"""
    host = {k: out[k].cpu().numpy() for k in PATH_KEYS + ("pairs",) + (("hit", "valid") if K > 1 else ())}
    off = host["col_offsets"]
    P = len(sims)
    assert len(host["score"]) == P * K and len(off) == P * K + 1
    for p in range(P):
        want, _ = fr.hits(sims[p], K, mode, 1.0, 0.1, mask)
        for k in range(K):
            q, w = p * K + k, want[k]
            what = (mode, mask, p, k, sims[p].shape)
            assert host["score"][q:q + 1].view(np.uint32)[0] == np.float32(w["score"]).reshape(1).view(np.uint32)[0], what
            assert tuple(host["end"][q]) == w["end"] and tuple(host["start"][q]) == w["start"], what
            assert np.array_equal(host["cols"][off[q]:off[q + 1]], w["cols"]) and host["n_match"][q] == w["n_match"], what
            assert host["n_cols"][q] == len(w["cols"]), what
            if K > 1:
                assert host["hit"][q] == k and tuple(host["pairs"][q]) == tuple(host["pairs"][p * K]), what
                assert bool(host["valid"][q]) == (float(w["score"]) > 0.0 and w["n_match"] >= 1), what
        if K > 1:  # the valid hits of a pair form a prefix
            v = host["valid"][p * K:(p + 1) * K]
            assert not (~v[:-1] & v[1:]).any(), (p, v)


def test_align_embeddings_against_the_reference():
    ra, rb = reps()
    plain = esm_amd.align_embeddings(ra, rb, mode="global", return_similarity=True)  # the same S bits in every call below
    sims = [s.cpu().numpy() for s in plain["similarity"]]
    assert [s.shape for s in sims] == [(a, b) for a in LEN_A for b in LEN_B]
    out = esm_amd.align_embeddings(ra, rb, free_ends="b", return_similarity=True)
    assert set(out) == set(plain)
    for s, t in zip(sims, out["similarity"]):
        assert np.array_equal(s.view(np.uint32), t.cpu().numpy().view(np.uint32))
    check_against_reference(out, sims, "global", 12, 1)
    host = out["start"].cpu().numpy()
    assert (host[:, 0] == 0).all() and (out["end"].cpu().numpy()[:, 0] == np.repeat(LEN_A, len(LEN_B))).all()  # a end to end
    for mode, mask, fe in (("local", 0, None), ("global", 12, "b"), ("global", 9, ["a_start", "b_end"])):
        two = esm_amd.align_embeddings(ra, rb, mode=mode, free_ends=fe, hits_per_pair=2)
        assert set(two) == set(PATH_KEYS) | {"pairs", "hit", "valid"} and two["valid"].dtype == torch.bool and two["hit"].dtype == torch.int32
        check_against_reference(two, sims, mode, mask, 2)
        for k in two:
            assert not torch.isnan(two[k].float()).any(), k
    # min_hit_score moves ``valid`` and nothing else
    strict = esm_amd.align_embeddings(ra, rb, mode="local", hits_per_pair=2, min_hit_score=1.5)
    loose = esm_amd.align_embeddings(ra, rb, mode="local", hits_per_pair=2)
    same(strict, loose)
    assert torch.equal(strict["valid"], (loose["score"] > 1.5) & (loose["n_match"] >= 1))


@pytest.mark.parametrize("mode,fe,K", [("global", "b", 1), ("local", None, 3), ("global", "both", 2)])
def test_blocks_give_the_bits_of_one_block(mode, fe, K):
    ra, rb = reps(1)
    every = A.check_pairs(None, len(LEN_A), len(LEN_B))
    budget = int(0.55 * A.block_bytes(LEN_A, LEN_B, every, E))
    assert len(A.plan_blocks(LEN_A, LEN_B, every, E, budget)) >= 3
    kw = dict(mode=mode, free_ends=fe, hits_per_pair=K)
    one, cut = esm_amd.align_embeddings(ra, rb, **kw), esm_amd.align_embeddings(ra, rb, max_bytes=budget, **kw)
    same(one, cut, keys=PATH_KEYS + ("pairs",) + (("hit", "valid") if K > 1 else ()))
    some = [(3, 0), (0, 4), (1, 2)]  # a sparse list: the same entries
    listed = esm_amd.align_embeddings(ra, rb, pairs=some, **kw)
    idx = torch.tensor([(a * len(LEN_B) + b) * K + k for a, b in some for k in range(K)], device="cuda")
    for key in ("score", "end", "start", "n_cols", "n_match"):
        assert torch.equal(listed[key], one[key][idx]), key


@pytest.mark.parametrize("mode", ["global", "local"])
def test_defaults_are_the_call_without_the_keywords(mode):
    ra, rb = reps(2)
    base = esm_amd.align_embeddings(ra, rb, mode=mode)
    spelled = esm_amd.align_embeddings(ra, rb, mode=mode, free_ends=None, hits_per_pair=1, min_hit_score=0.0)
    zero = esm_amd.align_embeddings(ra, rb, mode=mode, free_ends=0)
    assert set(base) == set(spelled) == set(zero) == set(PATH_KEYS) | {"pairs"}
    same(base, spelled, keys=PATH_KEYS + ("pairs",))
    same(base, zero, keys=PATH_KEYS + ("pairs",))
    assert set(esm_amd.align_embeddings(ra, rb, mode=mode, paths=False, hits_per_pair=1)) == {"pairs", "score", "end"}


def test_two_hits_of_one_target_give_two_rows():
    class Index:
        labels = ["t0", "t1"]
        sequences = ["GG" + "ACDEFGHIKLMN" + "PPPP" + "ACDEFGHIKLMW" + "GG", "ACDEFGHIKLMNQQ"]

    query = ("q", "ACDEFGHIKLMN")
    diag = lambda c: np.stack([np.arange(12), c + np.arange(12)], 1)
    # (pair, hit): t0 holds the query twice (columns 2 and 18), t1 once; t1's second entry is empty and not valid
    paths = [diag(2), diag(18), diag(0), np.zeros((0, 2), dtype=np.int64)]
    n_cols = np.array([len(p) for p in paths])
    alignment = dict(pairs=torch.tensor([[0, 0], [0, 0], [0, 1], [0, 1]], dtype=torch.int32).cuda(),
                     score=torch.tensor([12.0, 10.0, 11.0, 0.0]).cuda(), n_cols=torch.tensor(n_cols, dtype=torch.int32).cuda(),
                     cols=torch.tensor(np.concatenate(paths), dtype=torch.int32).cuda(),
                     col_offsets=torch.tensor(np.concatenate([[0], np.cumsum(n_cols)])).cuda(),
                     hit=torch.tensor([0, 1, 0, 1], dtype=torch.int32).cuda(), valid=torch.tensor([True, True, True, False]).cuda())
    (built,) = MB.msas_from_alignment([query], Index(), alignment, max_identity=None)
    assert built.labels == ["q", "t0", "t1", "t0|hit=1"]  # by score: 12, 11, 10
    assert built.hit_ids.cpu().tolist() == [-1, 0, 1, 0] and built.scores.cpu().tolist()[1:] == [12.0, 11.0, 10.0]
    assert [r for _, r in built.records()] == ["ACDEFGHIKLMN", "ACDEFGHIKLMN", "ACDEFGHIKLMN", "ACDEFGHIKLMW"]
    assert built.a3m_lines()[6:] == [">t0|hit=1", "ACDEFGHIKLMW"]
    # msa_from_hits with the numbers given directly; equal scores: the prefilter's order, then k
    cols, off = alignment["cols"], alignment["col_offsets"][:4]
    tie = MB.msa_from_hits(query, Index(), [0, 0, 1], torch.tensor([5.0, 5.0, 5.0]).cuda(), cols, off, max_identity=None, hit_numbers=[0, 1, 0])
    assert tie.labels == ["q", "t0", "t0|hit=1", "t1"]
    # a single-hit alignment goes through untouched
    single = {k: v for k, v in alignment.items() if k not in ("hit", "valid")}
    (built1,) = MB.msas_from_alignment([query], Index(), single, max_identity=None)
    assert built1.labels[:3] == ["q", "t0", "t1"] and len(built1) == 4 and built1.labels[3] == "t0"  # (the empty path is dropped)


def test_model_align_with_free_ends():
    L, H = 3, 2
    model = esm.ESM2(L, 128, H).eval()
    model.load_state_dict(synth_esm2_state_dict(L, 128, H, seed=11), strict=True)
    model = model.cuda()

    def tokens_of(lengths, seed):
        toks = synth_tokens(len(lengths), max(lengths), seed=seed)
        for k, n in enumerate(lengths):
            toks[k, n + 1] = 2
            toks[k, n + 2:] = 1
        return toks.cuda()

    ta, tb = tokens_of([17, 9], 3), tokens_of([39, 25, 8], 4)
    out = model.align(ta, tb, free_ends="b", return_similarity=True)
    check_against_reference(out, [s.cpu().numpy() for s in out["similarity"]], "global", 12, 1)
    plain = model.align(ta, tb, return_similarity=True)
    sims = [s.cpu().numpy() for s in plain["similarity"]]
    assert (out["score"] >= plain["score"]).all()  # every global path is a path of the free-end mode
    check_against_reference(model.align(ta, tb, mode="local", hits_per_pair=2, enhance=False), sims, "local", 0, 2)
    with pytest.raises(ValueError, match="mode='global' only"):
        model.align(ta, tb, mode="local", free_ends="b")
