"""The host side of design (esm_amd/design.py) without a GPU: ``contacts_from_pdb`` on a PDB text written here, the batch plan
and the refusals raised before a device is asked for, the head-group pin of ``esmk_forward_rows_contacts`` as the workspace plan
sees it, the argument checks of the new C entries (refused before any HIP call, on fake pointers as in tests/test_sampling_cpu.py),
the numpy references of tests/_design_ref.py on hand-worked cases, and the command line."""
import argparse
import ctypes
import math

import numpy as np
import pytest
import torch

import _design_ref as R
import _sampling_ref as SR
import esm
import esm_amd
from esm_amd import _native as N

D = __import__("importlib").import_module("esm_amd.design")
FAKE = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused first


def err():
    return N.lib.esmk_last_error().decode()


# ---- contacts_from_pdb ------------------------------------------------------------------------------------------------------
def atom(serial, name, res, chain, num, x, y, z):
    return "ATOM  %5d  %-3s %3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00\n" % (serial, name, res, chain, num, x, y, z)


SEQ_A = "MKTAGLVDEFSW"  # residue 4 is the glycine, residue 8 (E) has no C-beta in the file
NAMES = dict(zip("MKTAGLVDEFSW", ("MET", "LYS", "THR", "ALA", "GLY", "LEU", "VAL", "ASP", "GLU", "PHE", "SER", "TRP")))


def pdb_text():
    """Chain A: 12 residues on a line, C-alpha at x = 3.8 i, C-beta 1.5 above it; the glycine's C-alpha pushed 0.9 along x.
    Chain B: three residues next to the start of chain A (they must not enter chain A's map)."""
    lines, serial = ["HEADER    TEST\n"], 1
    for i, aa in enumerate(SEQ_A):
        x = 3.8 * i + (0.9 if aa == "G" else 0.0)
        lines.append(atom(serial, "N", NAMES[aa], "A", 10 + i, x - 1.0, 0.0, 0.0))
        lines.append(atom(serial + 1, "CA", NAMES[aa], "A", 10 + i, x, 0.0, 0.0))
        serial += 2
        if aa != "G" and i != 8:
            lines.append(atom(serial, "CB", NAMES[aa], "A", 10 + i, x, 1.5, 0.0))
            serial += 1
    lines.append("TER\n")
    for i, aa in enumerate("AKW"):
        lines.append(atom(serial, "CA", NAMES[aa], "B", 1 + i, 3.8 * i, 3.0, 0.0))
        lines.append(atom(serial + 1, "CB", NAMES[aa], "B", 1 + i, 3.8 * i, 4.5, 0.0))
        serial += 2
    lines.append("HETATM%5d  O   HOH A 900       0.000   0.000   0.000  1.00  0.00\n" % serial)
    lines.append("END\n")
    return "".join(lines)


def test_contacts_from_pdb(tmp_path):
    path = tmp_path / "two_chains.pdb"
    path.write_text(pdb_text())
    seq, target = esm_amd.contacts_from_pdb(str(path))
    assert seq == SEQ_A and target.dtype == np.uint8 and target.shape == (12, 12)
    # spacing 3.8: neighbours up to two apart are closer than 8 (7.6), three apart are not (11.4) ...
    want = (np.abs(np.arange(12)[:, None] - np.arange(12)[None, :]) <= 2).astype(np.uint8)
    # ... but the glycine's C-alpha sits at x = 16.1, y = 0: 8.63 from residue 2's C-beta (x = 7.6, y = 1.5), 6.87 from residue 6's
    want[4, 2] = want[2, 4] = 0
    assert math.hypot(16.1 - 7.6, 1.5) > 8.0 > math.hypot(22.8 - 16.1, 1.5)
    want[8, :] = want[:, 8] = 2  # no C-beta: its C-alpha is NOT taken
    assert np.array_equal(target, want)
    assert target[4, 4] == 1 and target[4, 6] == 1 and target[4, 3] == 1 and target[4, 7] == 0 and target[0, 3] == 0
    again = D.contacts_from_pdb(str(path), chain="A")
    assert again[0] == seq and np.array_equal(again[1], target)
    seq_b, target_b = D.contacts_from_pdb(str(path), chain="B")
    assert seq_b == "AKW" and np.array_equal(target_b, np.ones((3, 3), dtype=np.uint8))
    _, wide = D.contacts_from_pdb(str(path), chain="A", cutoff=12.0)
    assert wide[0, 3] == 1 and wide[0, 4] == 0 and wide[8, 0] == 2
    with pytest.raises(ValueError, match="no ATOM record"):
        D.contacts_from_pdb(str(path), chain="Z")


def test_target_map_forms():
    f = torch.tensor([[0.9, 0.5, float("nan")], [0.2, 0.51, 0.0], [1.0, 0.0, 0.7]])
    assert D.target_map(f).tolist() == [[1, 0, 2], [0, 1, 0], [1, 0, 1]]
    assert D.target_map(np.array([[True, False], [False, True]])).tolist() == [[1, 0], [0, 1]]
    assert D.target_map(np.array([[0, 2], [1, 0]], dtype=np.uint8)).dtype == torch.uint8
    for bad in (np.zeros((2, 3)), np.zeros(4), np.array([[0, 3], [0, 0]])):
        with pytest.raises(ValueError):
            D.target_map(bad)
    with pytest.raises(ValueError, match="all chains have the target's length"):
        D.target_map(np.zeros((5, 5)), S=4)


# ---- the host plan and the refusals -------------------------------------------------------------------------------------------
def test_batch_sizes_from_max_bytes():
    def bytes_of(B):
        return 1000 + 300 * B

    assert D.batch_size(bytes_of, 64, 1 << 30) == 64
    assert D.batch_size(bytes_of, 64, 1000 + 300 * 10) == 10  # 7 batches of at most 10
    assert D.batch_size(bytes_of, 64, 1000 + 300 * 33) == 32  # 33 would fit, but two batches of 32 are the even cut
    assert D.batch_size(bytes_of, 5, 1300) == 1
    with pytest.raises(ValueError, match="one chain alone"):
        D.batch_size(bytes_of, 5, 1299)
    with pytest.raises(ValueError):
        D.batch_size(bytes_of, 0, 1 << 30)
    assert D.inverse_temperatures(2.0, 3) == [0.5, 0.5, 0.5] and D.inverse_temperatures([1.0, 0.0], 2) == [1.0, float("inf")]
    for bad in ((-1.0, 2), ([1.0], 2), (float("inf"), 1), (float("nan"), 1)):
        with pytest.raises(ValueError):
            D.inverse_temperatures(*bad)


def msa_model():
    args = argparse.Namespace(layers=1, embed_dim=64, ffn_embed_dim=128, attention_heads=2, dropout=0.1, attention_dropout=0.1,
                              activation_dropout=0.1, max_positions=1024, embed_positions_msa=True, embed_positions_msa_dim=64,
                              max_tokens=2 ** 14, max_tokens_per_msa=2 ** 14)
    return esm.MSATransformer(args, esm.Alphabet.from_architecture("msa_transformer"))


def test_refusals_before_a_device_is_asked_for():
    model = esm.ESM2(1, 128, 2)
    a = model.alphabet
    toks = torch.tensor([[0, 5, 6, 7, 8, 2], [0, 9, 10, 11, 12, 2]])
    target = np.zeros((4, 4), dtype=np.uint8)
    with pytest.raises(ValueError, match="all chains have the target's length"):
        model.design(toks, np.zeros((5, 5), dtype=np.uint8), 3)
    padded = toks.clone()
    padded[1, 4:] = torch.tensor([2, 1])
    with pytest.raises(ValueError, match="<pad>"):
        model.design(padded, target, 3)
    with pytest.raises(ValueError, match="force_new with proposal='lm'"):
        model.design(toks, target, 3, proposal="lm", force_new=True)
    outside = toks.clone()
    outside[1, 2] = a.get_idx("X")
    with pytest.raises(ValueError, match="outside `allowed` at designable position 2"):
        model.design(outside, target, 3, proposal="lm")
    with pytest.raises(ValueError, match="outside `allowed`"):
        model.design(toks, target, 3, proposal="lm", allowed="AC")
    for kw in (dict(proposal="gibbs"), dict(contact_loss="mse"), dict(min_sep=0), dict(temperature=[1.0, 1.0]), dict(w_contact=0, w_lm=0),
               dict(temperature=-1.0), dict(proposal="lm", proposal_temperature=0.0), dict(chain_ids=[1]), dict(seed=-1)):
        with pytest.raises(ValueError):
            model.design(toks, target, 3, **kw)
    with pytest.raises(ValueError, match="target=None needs w_contact=0"):
        model.design(toks, None, 3)
    with pytest.raises(ValueError, match="<pad>"):
        model.design_energy(padded, target)
    # what passes every host check reaches the device question
    for call in (lambda: model.design(toks, target, 3), lambda: model.design(toks, None, 3, w_contact=0),
                 lambda: model.design(toks, target, 3, proposal="lm"), lambda: model.design_energy(toks, target),
                 lambda: esm_amd.design(model, toks, target, 3)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    msa = msa_model()
    mt = torch.zeros((1, 2, 8), dtype=torch.int64)
    for call in (lambda: msa.design(mt, target, 3), lambda: msa.design_energy(mt, target), lambda: D.design(msa, mt, target, 3),
                 lambda: D.design_energy(msa, mt, target)):
        with pytest.raises(NotImplementedError, match="MSA Transformer"):
            call()
    assert esm_amd.design is D and esm_amd.design_energy is D.design_energy


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def make(E=128, H=8, V=33, **kw):
    cfg = N.EsmkConfig(2, E, H, 4 * E, V, 1, 32, 0, 2, 1, 1, 1, N.dtype_code(torch.float16), 0, 0, 0)
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    assert N.lib.esmk_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, err()
    return h


def test_the_entry_plans_the_head_groups_of_one_sequence():
    """esmk_debug_contact_groups: H = 8, head_dim 16 at T = 300 is 9 (query block, key chunk) pairs per sequence: 8 groups at B = 1
    (contacts_head_groups(9, 8, 16): ceil(1024 / 9) = 114 > H) and 4 at B = 24 (216 pairs: ceil(1024 / 216) = 5 groups of 2 heads
    hold the 8 heads in 4) — the pinned entry takes 8 whatever B is, and its workspace holds the accumulators of that count."""
    h = make()
    g = ctypes.c_int32()

    def groups(B, T, pinned):
        assert N.lib.esmk_debug_contact_groups(h, B, T, pinned, ctypes.byref(g)) == 0, err()
        return g.value

    assert groups(1, 300, 0) == 8 and groups(24, 300, 0) == 4 and groups(24, 300, 1) == 8 and groups(1, 300, 1) == 8
    for B in (1, 2, 7, 24, 200):
        for T in (9, 70, 128, 129, 300, 1024):
            assert groups(B, T, 1) == groups(1, T, 0) >= groups(B, T, 0)
    assert N.lib.esmk_debug_contact_groups(h, 0, 300, 1, ctypes.byref(g)) != 0 and "must be positive" in err()
    assert N.lib.esmk_debug_contact_groups(None, 1, 300, 1, ctypes.byref(g)) != 0 and "null" in err()
    n, off, plain, rows = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    q = N.lib.esmk_rows_contacts_workspace_bytes
    B, T = 24, 300
    assert q(h, B, T, 5, ctypes.byref(n), ctypes.byref(off)) == 0, err()
    assert N.lib.esmk_workspace_bytes(h, B, T, N.OUT_CONTACTS, ctypes.byref(plain)) == 0
    assert N.lib.esmk_rows_workspace_bytes(h, B, T, 5, ctypes.byref(rows), None) == 0
    extra = (8 - 4) * B * T * T * 4  # four more accumulators than esmk_forward plans at this B
    assert n.value >= plain.value + extra and n.value - off.value >= 5 * 33 * 4 and off.value % 256 == 0
    assert n.value >= rows.value + 8 * B * T * T * 4
    sizes = []
    for b in (1, 2, 3, 24, 25):
        assert q(h, b, T, b * 298, ctypes.byref(n), None) == 0
        sizes.append(n.value)
    assert sizes == sorted(sizes) and len(set(sizes)) == 5  # grows with B: esm_amd.design.batch_size may search it
    assert q(h, 2, T, 0, ctypes.byref(n), None) == 0  # n_sel = 0 is allowed
    N.lib.esmk_destroy(h)


def test_rows_contacts_argument_checks():
    h = make()
    need = ctypes.c_size_t()
    assert N.lib.esmk_rows_contacts_workspace_bytes(h, 2, 70, 5, ctypes.byref(need), None) == 0

    def call(handle=h, packed=FAKE, tokens=FAKE, B=2, T=70, sel=FAKE, n_sel=5, out=FAKE, ct=FAKE, ws=FAKE, ws_bytes=1 << 40):
        return N.lib.esmk_forward_rows_contacts(handle, packed, tokens, B, T, sel, n_sel, out, ct, ws, ctypes.c_size_t(ws_bytes), None)

    who = "esmk_forward_rows_contacts: "
    for kw in (dict(handle=None), dict(packed=None), dict(tokens=None), dict(sel=None), dict(out=None), dict(ct=None), dict(ws=None),
               dict(n_sel=0, ct=None)):
        assert call(**kw) != 0 and who + "null argument" in err(), kw
    assert call(n_sel=-1) != 0 and who + "n_sel must not be negative" in err()
    assert call(B=0) != 0 and who + "B and T must be positive" in err()
    assert call(B=1 << 12, T=1 << 13) != 0 and who + "B*T exceeds 2^24 rows" in err()
    assert call(T=2) != 0 and who + "no residue" in err()
    assert call(ws_bytes=need.value - 1) != 0 and who + "workspace too small" in err()
    q = N.lib.esmk_rows_contacts_workspace_bytes
    assert q(h, 2, 70, 5, None, None) != 0 and "esmk_rows_contacts_workspace_bytes: null" in err()
    assert q(h, 2, 70, -1, ctypes.byref(need), None) != 0 and "n_sel must not be negative" in err()
    N.lib.esmk_destroy(h)
    big = make(V=65)
    assert call(handle=big) != 0 and who + "vocabulary above 64 entries" in err()
    N.lib.esmk_destroy(big)
    cfg = N.EsmkMsaConfig(2, 128, 2, 256, 33, 1, 32, 0, 2, 1, 0, 1026, 1, N.dtype_code(torch.float16), 0)
    hm = ctypes.c_void_p()
    assert N.lib.esmk_msa_create(ctypes.byref(cfg), ctypes.byref(hm)) == 0
    assert call(handle=hm) != 0 and who + "MSA handle" in err()
    assert q(hm, 2, 70, 5, ctypes.byref(need), None) != 0 and "MSA handle" in err()
    g = ctypes.c_int32()
    assert N.lib.esmk_debug_contact_groups(hm, 1, 70, 1, ctypes.byref(g)) != 0 and "MSA handle" in err()
    N.lib.esmk_destroy(hm)


def test_design_op_argument_checks():
    lib = N.lib

    def p(tokens=FAKE, slot=None, off=FAKE, pos=FAKE, cid=FAKE, mask=0xFFFFF0, force=1, seed=1, step=0, site=FAKE, old=FAKE, tok=FAKE,
          n=4, B=4, T=70, total=9, V=33):
        return lib.esmk_op_propose_mutations(tokens, slot, off, pos, cid, mask, force, seed, step, site, old, tok, n, B, T, total, V,
                                             None)

    for kw in (dict(tokens=None), dict(off=None), dict(pos=None), dict(cid=None), dict(site=None), dict(old=None), dict(tok=None)):
        assert p(**kw) != 0 and err() == "esmk_op_propose_mutations: null argument", kw
    for kw in (dict(n=0), dict(B=0), dict(T=-1)):
        assert p(**kw) != 0 and "n_chain, B and T must be positive" in err(), kw
    assert p(total=-1) != 0 and "total must not be negative" in err()
    assert p(V=65) != 0 and "V must be in 1 .. 64" in err()
    assert p(step=-1) != 0 and "step must not be negative" in err()
    assert p(B=1 << 12, T=1 << 13) != 0 and "2^24" in err()

    def e(ct=FAKE, target=FAKE, out=FAKE, count=FAKE, B=2, S=68, min_sep=6, kind=0):
        return lib.esmk_op_contact_energy(ct, target, out, count, B, S, min_sep, kind, None)

    for kw in (dict(ct=None), dict(target=None), dict(out=None), dict(count=None)):
        assert e(**kw) != 0 and err() == "esmk_op_contact_energy: null argument", kw
    assert e(B=0) != 0 and "B and S must be positive" in err()
    assert e(S=32769) != 0 and "S above 32768" in err()
    assert e(min_sep=0) != 0 and "min_sep must be at least 1" in err()
    for kind in (-1, 2):
        assert e(kind=kind) != 0 and "kind must be 0 (pos) or 1 (bce)" in err()

    def a(tokens=FAKE, slot=None, site=FAKE, tok=FAKE, cid=FAKE, ec=FAKE, lp=FAKE, n_res=FAKE, h=None, wc=1.0, wl=1.0, inv_t=1.0,
          seed=1, step=0, e_cur=FAKE, ecc=None, elc=None, acc=FAKE, u=None, ep=None, n=4, B=4, T=70):
        return lib.esmk_op_mh_accept(tokens, slot, site, tok, cid, ec, lp, n_res, h, wc, wl, inv_t, seed, step, e_cur, ecc, elc, acc, u,
                                     ep, n, B, T, None)

    for kw in (dict(tokens=None), dict(site=None), dict(tok=None), dict(cid=None), dict(e_cur=None), dict(acc=None)):
        assert a(**kw) != 0 and err() == "esmk_op_mh_accept: null argument", kw
    assert a(n_res=None) != 0 and "lp_sum without n_res" in err()
    assert a(n=0) != 0 and "n_chain, B and T must be positive" in err()
    for bad in (-1.0, float("nan")):
        assert a(inv_t=bad) != 0 and "inv_temperature must not be negative or NaN" in err()
    for kw in (dict(wc=float("inf")), dict(wl=float("nan"))):
        assert a(**kw) != 0 and "weights must be finite" in err(), kw
    assert a(step=-1) != 0 and "step must not be negative" in err()

    def hr(lp=FAKE, old=FAKE, new=FAKE, inv_t=1.0, out=FAKE, n=4, V=33):
        return lib.esmk_op_hastings_rows(lp, old, new, inv_t, out, n, V, None)

    for kw in (dict(lp=None), dict(old=None), dict(new=None), dict(out=None)):
        assert hr(**kw) != 0 and err() == "esmk_op_hastings_rows: null argument", kw
    assert hr(n=0) != 0 and "n must be in 1 .. 2^24" in err()
    assert hr(V=65) != 0 and "V must be in 1 .. 64" in err()
    for bad in (-1.0, float("inf"), float("nan")):
        assert hr(inv_t=bad) != 0 and "inv_t_prop must be finite and not negative" in err()


# ---- the references on hand-worked cases --------------------------------------------------------------------------------------
def test_reference_proposal():
    seed, chain, step = 0xABCDEF0123, 9, 4
    w = SR.philox4x32_10((chain, step, 2, 0), (seed & 0xFFFFFFFF, seed >> 32))
    assert R.words(seed, chain, step, R.PROPOSAL) == [int(x) for x in w]
    assert R.words(seed, chain, step, R.ACCEPTANCE)[0] == int(SR.philox4x32_10((chain, step, 3, 0), (seed & 0xFFFFFFFF, seed >> 32))[0])
    row = [0] + [5 + (i % 20) for i in range(68)] + [2]
    positions = list(range(1, 69))
    mask = sum(1 << v for v in range(4, 24))
    site, old, tok = R.proposal(seed, chain, step, positions, row, mask, True)
    assert site == positions[(int(w[0]) * 68) >> 32] and old == row[site]
    cand = [v for v in range(4, 24) if v != old]
    assert tok == cand[(int(w[1]) * 19) >> 32] and tok != old
    assert R.proposal(seed, chain, step, positions, row, mask, False)[2] == list(range(4, 24))[(int(w[1]) * 20) >> 32]
    assert R.proposal(seed, chain, step, [], row, mask, True) == (-1, -1, -1)
    assert R.proposal(seed, chain, step, [7], row, 1 << 9, False) == (7, row[7], 9)
    assert R.proposal(seed, chain, step, [7], row, 1 << row[7], True) == (7, row[7], -1)  # the only candidate is the current token
    assert R.proposal(seed, chain, step, [7], row, 1 << row[7], False) == (7, row[7], row[7])
    # a current token outside the candidate set takes nothing away from it
    assert R.proposal(seed, chain, step, [0], row, mask, True)[2] == list(range(4, 24))[(int(w[1]) * 20) >> 32]
    sites = [R.proposal(seed, 3, s, positions, row, mask, True)[0] for s in range(2000)]
    counts = np.bincount(sites, minlength=69)[1:]
    assert counts.min() > 8 and counts.max() < 60  # 29.4 expected per site
    u = [R.accept_uniform(seed, 3, s) for s in range(2000)]
    assert 0 <= min(u) and max(u) < 1 and abs(np.mean(u) - 0.5) < 0.03 and all(x * 2 ** 24 == int(x * 2 ** 24) for x in u)


def test_reference_energy_on_worked_maps():
    p = np.array([[0.9, 0.5, 0.25], [0.5, 0.9, 1.0], [0.25, 1.0, 0.0]], dtype=np.float32)
    target = np.array([[1, 1, 0], [1, 1, 1], [0, 1, 1]], dtype=np.uint8)
    top = math.log(1.0 - 2.0 ** -24)  # the clamp of p = 1
    e, n, bound = R.contact_energy(p, target, 1, "pos")
    assert n == 2 and e == -((math.log(0.5) + top) / 2) and 0 < bound < 1e-15
    e, n, _ = R.contact_energy(p, target, 1, "bce")
    assert n == 3 and abs(e + (math.log(0.5) + math.log(0.75) + top) / 3) < 1e-16
    assert R.contact_energy(p, target, 2, "pos") == (0.0, 0, 0.0)  # the one pair two apart is no target contact
    e, n, _ = R.contact_energy(p, target, 2, "bce")
    assert n == 1 and e == -math.log(0.75)
    assert R.contact_energy(p, target, 3, "bce") == (0.0, 0, 0.0)
    ignore = target.copy()
    ignore[0, 1] = 2
    assert R.contact_energy(p, ignore, 1, "pos")[:2] == (-top, 1)
    zero = np.zeros((3, 3), dtype=np.float32)
    assert R.contact_energy(zero, target, 1, "pos")[0] == -math.log(2.0 ** -24)  # the clamp of p = 0
    assert R.contact_energy(zero, np.zeros((3, 3), dtype=np.uint8), 1, "bce")[0] == -math.log(1.0 - 2.0 ** -24)
    # only the upper triangle is read
    lower = target.copy()
    lower[2, 0] = 1
    assert R.contact_energy(p, lower, 1, "bce") == R.contact_energy(p, target, 1, "bce")


def test_reference_acceptance_rule():
    assert R.combine(1.0, 2.0, 1.0, -30.0, 10) == (5.0, 3.0)
    assert R.combine(0.5, 2.0, 0.0, -30.0, 10) == (1.0, 3.0) and R.combine(0.0, 2.0, 2.0, -30.0, 0) == (0.0, 0.0)
    assert R.accept(1.0, 2.0, 1.0, 0.0, 0.999, 5) == (True, False)   # downhill
    assert R.accept(2.0, 2.0, 1.0, 0.0, 0.999, 5) == (True, False)   # level: a = 0
    assert R.accept(3.0, 2.0, 1.0, 0.0, 0.3, 5) == (True, False)     # exp(-1) = 0.368
    assert R.accept(3.0, 2.0, 1.0, 0.0, 0.4, 5) == (False, False)
    assert R.accept(3.0, 2.0, 1.0, 1.5, 0.99, 5) == (True, False)    # the Hastings term lifts it over 0
    assert R.accept(1.0, 2.0, 1.0, -2.0, 0.4, 5) == (False, False)   # ... or pulls a downhill move under
    assert R.accept(1.0, 2.0, 1.0, 0.0, 0.0, -1) == (False, False)   # nothing was proposed
    inf = float("inf")
    assert R.accept(2.0, 2.0, inf, 9.0, 0.5, 5) == (True, False) and R.accept(2.0 + 1e-12, 2.0, inf, 9.0, 0.0, 5) == (False, False)
    assert R.accept(3.0, 2.0, 1e-6, 0.0, 0.99, 5)[0] and not R.accept(float("nan"), 2.0, 1.0, 0.0, 0.0, 5)[0]
    assert R.accept(3.0, 2.0, 1.0, 0.0, math.exp(-1.0) + 2.0 ** -41, 5) == (False, True)
    assert R.accept(3.0, 2.0, 1.0, 0.0, math.exp(-1.0) - 2.0 ** -39, 5) == (True, False)


def test_the_synthetic_acceptance_cases_have_no_undecided_decision():
    for hastings in (True, False):
        case = R.accept_case(with_hastings=hastings)
        assert (case["tok"] < 0).sum() == 24
        for wc, wl in R.ACCEPT_WEIGHTS:
            for step, t in enumerate(R.ACCEPT_TEMPERATURES):
                e_prop, u, acc, und = R.accept_reference(case, wc, wl, t, step)
                assert und.sum() == 0 and not acc[case["tok"] < 0].any()
                if (wc, wl) == (1.0, 1.0):
                    dE = e_prop - case["e_cur"]
                    assert (dE[1::3] == 0).all() and (dE[0::3] < 0).all() and (dE[2::3] > 0).all()
                    if t == 0.0:
                        assert np.array_equal(acc, (dE <= 0) & (case["tok"] >= 0))
                    if t == 1e6 and not hastings:
                        assert acc[case["tok"] >= 0].mean() > 0.99
                    if t == 1.0 and not hastings:
                        up = (dE > 0) & (case["tok"] >= 0)
                        assert acc[(dE <= 0) & (case["tok"] >= 0)].all() and 0 < acc[up].sum() < up.sum()


# ---- the command line -----------------------------------------------------------------------------------------------------------
def test_cli_parsing_and_files(tmp_path):
    base = ["--model-location", "m.pt", "--output", "o.fasta"]
    a = D.parse_args(base + ["--target-pdb", "t.pdb", "--chain", "B"])
    assert (a.target_pdb, a.chain, a.num_chains, a.steps, a.proposal, a.w_contact, a.w_lm, a.seed) == ("t.pdb", "B", 1, 1000, "uniform",
                                                                                                      1.0, 1.0, 0)
    assert a.temperature is None and a.anneal is None and a.init == "random" and a.log is None
    a = D.parse_args(base + ["--no-target", "--length", "50", "--num-chains", "8", "--steps", "20", "--anneal", "2:0.5", "--proposal",
                             "lm", "--w-lm", "3", "--seed", "7", "--log", "l.csv", "--init-sequence", "MK"])
    assert a.no_target and a.length == 50 and a.anneal == (2.0, 0.5) and a.proposal == "lm" and a.log == "l.csv" and a.seed == 7
    for bad in (base, base + ["--no-target"], base + ["--target-npy", "t.npy", "--length", "5"],
                base + ["--target-npy", "t.npy", "--target-pdb", "t.pdb"], base + ["--target-npy", "t.npy", "--chain", "A"],
                base + ["--target-npy", "t.npy", "--anneal", "1:0"], base + ["--target-npy", "t.npy", "--anneal", "1:2", "--temperature", "1"],
                base + ["--target-npy", "t.npy", "--num-chains", "0"], base + ["--target-npy", "t.npy", "--proposal", "gibbs"],
                base + ["--target-npy", "t.npy", "--init", "native"], ["--target-npy", "t.npy", "--output", "o"]):
        with pytest.raises(SystemExit):
            D.parse_args(bad)
    ladder = D.anneal_ladder(2.0, 0.5, 3)
    assert ladder[0] == 2.0 and abs(ladder[1] - 1.0) < 1e-15 and abs(ladder[2] - 0.5) < 1e-15 and D.anneal_ladder(2.0, 0.5, 1) == [2.0]
    seqs = D.random_sequences(3, 11, seed=5)
    assert seqs == D.random_sequences(3, 11, seed=5) != D.random_sequences(3, 11, seed=6)
    assert all(len(s) == 11 and set(s) <= set("ACDEFGHIKLMNPQRSTVWY") for s in seqs)
    out = tmp_path / "o.fasta"
    D.write_fasta(out, "design", [0, 1], ["MA", "MC"], [1.25, 0.5], seed=5)
    assert out.read_text() == ">design|chain=0|seed=5|energy=1.250000\nMA\n>design|chain=1|seed=5|energy=0.500000\nMC\n"
    traj = {k: torch.zeros((2, 2), dtype=torch.float64) for k in D.TRAJECTORY_FIELDS}
    D.write_log(tmp_path / "l.csv", traj, [4, 5])
    rows = (tmp_path / "l.csv").read_text().splitlines()
    assert rows[0] == "step,chain," + ",".join(D.TRAJECTORY_FIELDS) and len(rows) == 5 and rows[4].startswith("1,5,")


def test_cli_refuses_an_msa_model(tmp_path, monkeypatch):
    from esm_amd import pretrained

    model = msa_model()
    alphabet = esm.Alphabet.from_architecture("msa_transformer")
    monkeypatch.setattr(pretrained, "load_model_and_alphabet", lambda location: (model, alphabet))
    with pytest.raises(SystemExit, match="MSA Transformer"):
        D.main(["--model-location", "msa.pt", "--no-target", "--length", "5", "--output", str(tmp_path / "o.fasta")])
    assert not (tmp_path / "o.fasta").exists()


def test_the_measurement_switch_unpins_the_workspace_plan_only_while_set():
    """esmk_debug_set("rows_contacts_own_groups", 1): the entry plans the batch's own group count (tools/design_throughput.py
    times what the pin costs); 0, the default, is the pin again."""
    h = make()
    n = ctypes.c_size_t()
    q = N.lib.esmk_rows_contacts_workspace_bytes
    assert q(h, 24, 300, 5, ctypes.byref(n), None) == 0
    pinned = n.value
    assert N.lib.esmk_debug_set(b"rows_contacts_own_groups", 1.0) == 0
    try:
        assert q(h, 24, 300, 5, ctypes.byref(n), None) == 0
        assert pinned - n.value == (8 - 4) * 24 * 300 * 300 * 4
    finally:
        assert N.lib.esmk_debug_set(b"rows_contacts_own_groups", 0.0) == 0
    assert q(h, 24, 300, 5, ctypes.byref(n), None) == 0 and n.value == pinned
    N.lib.esmk_destroy(h)
