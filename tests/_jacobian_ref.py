"""Shared by the categorical-Jacobian tests: fp64 torch restatements of the definition (centring, coupling map, average product
correction), the B = 1 ``forward`` loop that defines the raw tensor, and the error bounds, each derived where it is computed.
EPS = 2^-24 is the largest relative error of one rounding to fp32 (half an ulp)."""
import torch

EPS = 2.0 ** -24
AXES = (3, 2, 1, 0)  # the order of the passes: b, j, a, i


# ---- the raw tensor ---------------------------------------------------------------------------------------------------------
def residue_positions(model, tokens_1d):
    """Token positions of the residues: the non-pad tokens without the <cls> / <eos> the alphabet adds."""
    keep = tokens_1d.ne(model.padding_idx)
    if model.prepend_bos:
        keep[0] = False
    if model.append_eos:
        keep &= tokens_1d.ne(model.eos_idx)
    return keep.nonzero().view(-1).tolist()


def loop_jacobian(model, tokens, cols):
    """The definition on this model's own ``forward`` at B = 1: one forward per (position, candidate), fp32
    ``J[i, a, j, b] = logits(copy(i, a))[p_j, t_b] - logits(x)[p_j, t_b]``.  ``tokens`` int64 [1, T] on the device."""
    pos = residue_positions(model, tokens[0].cpu())
    L, nA = len(pos), len(cols)
    pos_d = torch.tensor(pos, device=tokens.device)
    cols_d = torch.tensor(cols, device=tokens.device)
    J = torch.empty((L, nA, L, nA), dtype=torch.float32, device=tokens.device)
    with torch.no_grad():
        wt = model(tokens)["logits"][0].float()[pos_d][:, cols_d]
        for i, p in enumerate(pos):
            for a, t in enumerate(cols):
                copy = tokens.clone()
                copy[0, p] = t
                J[i, a] = model(copy)["logits"][0].float()[pos_d][:, cols_d] - wt
    return J


# ---- centring ---------------------------------------------------------------------------------------------------------------
def center_ref(J):
    """(Jc fp64, [m_1 .. m_4]): the four passes b, j, a, i on the fp64 copy of ``J`` with NO rounding in between; m_k is the
    largest magnitude after pass k."""
    x = J.double().clone()
    ms = []
    for axis in AXES:
        x = x - x.sum(dim=axis, keepdim=True) / x.shape[axis]
        ms.append(x.abs().max().item() if x.numel() else 0.0)
    return x, ms


def center_closed_form(J):
    """(P_i x P_a x P_j x P_b) J in fp64 with P = I - 11'/n written out as matrices: the closed form of the four passes."""
    x = J.double()
    L, nA = x.shape[0], x.shape[1]
    PL = torch.eye(L, dtype=torch.float64) - torch.full((L, L), 1.0 / L, dtype=torch.float64)
    PA = torch.eye(nA, dtype=torch.float64) - torch.full((nA, nA), 1.0 / nA, dtype=torch.float64)
    PL, PA = PL.to(x.device), PA.to(x.device)
    x = torch.einsum("pi,iajb->pajb", PL, x)  # one axis at a time: the Kronecker product applied factor by factor
    x = torch.einsum("qa,pajb->pqjb", PA, x)
    x = torch.einsum("rj,pqjb->pqrb", PL, x)
    return torch.einsum("sb,pqrb->pqrs", PA, x)


def center_bound(ms):
    """The per-element bound of the kernel's centred tensor against ``center_ref``: sum over the passes k = 1 .. 4 of
    2^(4 - k) * EPS * m_k.  Pass k rounds every element to fp32 once — an error of at most EPS times its magnitude, which is
    m_k up to the (second-order) error already made — and each of the 4 - k later projections I - 11'/n has an infinity norm of
    |1 - 1/n| + (n - 1)/n < 2, so it at most doubles an error.  The kernel's means are fp64 sums of at most a few thousand
    fp32 values: their error (n * 2^-53 relative) is far below one fp32 rounding and is not counted."""
    return sum(2.0 ** (4 - k) * EPS * m for k, m in enumerate(ms, start=1))


# ---- the coupling map and its correction ------------------------------------------------------------------------------------
def contacts_ref(Jc):
    """S fp64 [L, L] from ``Jc`` (any float dtype; taken in fp64): S[i, j] = ||0.5 (Jc[i, :, j, :] + Jc[j, :, i, :]')||_F."""
    x = Jc.double()
    sym = 0.5 * (x + x.permute(2, 3, 0, 1))
    return sym.pow(2).sum(dim=(1, 3)).sqrt()


def contacts_bound(S_ref):
    """[L, L] bound of the kernel's fp32 S against ``contacts_ref`` of the SAME fp32 tensor: the kernel adds the nA^2 <= 1024
    squares in fp64 (relative error below 1026 * 2^-53 < 2^-42 with the square root) and rounds to fp32 once (EPS): EPS * S with
    2^-10 of slack for the fp64 part."""
    return EPS * (1 + 2.0 ** -10) * S_ref


def apc_ref(S):
    """C fp64: diagonal of S zero, C = S - r c' / s (no correction when s == 0), diagonal zero."""
    x = S.double().clone()
    x.fill_diagonal_(0.0)
    r, c, s = x.sum(dim=1, keepdim=True), x.sum(dim=0, keepdim=True), x.sum()
    if s.item() != 0.0:
        x = x - r * c / s
    x.fill_diagonal_(0.0)
    return x


def apc_bound(S, C_ref):
    """[L, L] bound of the kernel's fp32 C against ``apc_ref`` of the SAME non-negative fp32 S: the kernel's sums, product and
    quotient are fp64 (relative error of r_i c_j / s below (3 L + 3) * 2^-53 < 2^-40 for L < 2^11, counted against |S| + |r c / s|)
    and the result is rounded to fp32 once (EPS * |C|, 2^-10 of slack)."""
    x = S.double().clone()
    x.fill_diagonal_(0.0)
    s = x.sum()
    t = x.sum(dim=1, keepdim=True) * x.sum(dim=0, keepdim=True) / s if s.item() != 0.0 else torch.zeros_like(x)
    return EPS * (1 + 2.0 ** -10) * C_ref.abs() + 2.0 ** -40 * (x.abs() + t.abs())


def contact_map_ref_and_bound(J_raw):
    """(C fp64, bound [L, L]) for the whole pipeline on the raw fp32 tensor: ``apc_ref(contacts_ref(center_ref(J)))`` with no
    rounding anywhere, and the bound of the engine's fp32 map against it.

    eps = ``center_bound``: every element of the engine's centred tensor is within eps, so is every element of the
    symmetrised nA x nA block E of a pair, and | ||M + E||_F - ||M||_F | <= ||E||_F <= nA * eps.  With the rounding of S
    (``contacts_bound``) every S is within d = nA * eps + EPS (1 + 2^-10) max S.  The sums then are within dr = (L - 1) d (rows,
    columns) and ds = L (L - 1) d (total); with s_low = s - ds > 0 the product term t = r_i c_j / s moves by at most
        dt = ((|c_j| + dr) dr + |r_i| dr) / s_low + |r_i c_j| ds / (s s_low),
    and the result is rounded once: bound = d + dt + EPS (1 + 2^-10) (|C| + d + dt).  The diagonal is exactly zero."""
    Jc, ms = center_ref(J_raw)
    nA, L = J_raw.shape[1], J_raw.shape[0]
    eps = center_bound(ms)
    S = contacts_ref(Jc)
    C = apc_ref(S)
    d = nA * eps + EPS * (1 + 2.0 ** -10) * S.max().item()
    x = S.clone()
    x.fill_diagonal_(0.0)
    r, c, s = x.sum(dim=1, keepdim=True), x.sum(dim=0, keepdim=True), x.sum().item()
    dr, ds = (L - 1) * d, L * (L - 1) * d
    s_low = s - ds
    assert s_low > 0.0, "the map is too small against its own error for a bound"
    dt = ((c.abs() + dr) * dr + r.abs() * dr) / s_low + (r * c).abs() * ds / (s * s_low)
    bound = d + dt + EPS * (1 + 2.0 ** -10) * (C.abs() + d + dt)
    bound.fill_diagonal_(0.0)
    return C, bound


def report(what, err, bound):
    """Prints max err / bound (where the bound is zero the error must be zero too), then asserts."""
    err, bound = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(bound, dtype=torch.float64)
    bound = bound.expand_as(err) if bound.dim() else bound
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                              torch.zeros_like(err)))
    worst = ratio.max().item() if ratio.numel() else 0.0
    print(f"\n{what}: max err / bound = {worst:.3f} (max err {err.max().item() if err.numel() else 0.0:.3e})")
    assert worst <= 1.0, (what, worst)
