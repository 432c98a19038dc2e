"""fp64 restatement of the linear pairwise head (csrc/pair_head.hip) and the fp32 error bound of its kernels.

The reference (examples/lm-design/utils/linear_projection.py:119-135 on the attention maps of esm/model/esm2.py:119-139,
cropped by linear_projection.py:76-82) is two 1 x 1 convolutions over the channels c = layer * H + head:

    out[b,i,j,o] = sum_c W[c,o] (P_c[b,i,j] + P_c[b,j,i]) + bias[o]   o <  n_sym   (conv1 on P + P^T)
    out[b,i,j,o] = sum_c W[c,o]  P_c[b,i,j]               + bias[o]   o >= n_sym   (conv2 on P)

``pair_head_on_maps`` states it on attention maps; ``pair_head_ref`` on (q, k, key_bias), one layer at a time like
``_contacts_ref.contact_ref``, with the operands the kernel takes: q_effective (natural domain, ``ops.to_log2_domain``), k as
rounded to the operand dtype; rows and columns of <pad> positions are zero; ``null_k`` [L,H,D] adds ESM-1's null key to the row
log-sum-exp (it has no column).  It hands back the fp64 natural lse for the kernel to take.

Bound (``PairRef.tol``, after ``_contacts_ref.ContactRef.tol``): |got - ref| <= 2 kappa mag + 4u (|ref| + 1) with
kappa = eps_p + (L*H + 8) u, eps_p the relative error of one recomputed probability, mag = sum_c |W[c,o]| (P_c[i,j] (+ P_c[j,i])).

Mutation knobs (for showing that the bound discriminates): ``drop`` = channels (l, h) left out, ``w_layer_shift`` = layer l
takes layer (l + shift) % L's weights, ``swap_blocks`` = the transpose term goes to the outputs >= n_sym instead of those below,
``no_transpose`` = the transpose term is left out."""
import math

import torch

U = 2.0 ** -24  # fp32 unit roundoff
LOG2E = 1.4426950408889634


def eps_p(sbound, T, D):
    """Relative error of one probability the kernel recomputes (``ContactRef.tol``): chained-MFMA score, fp32 lse, v_exp_f32."""
    return math.log(2.0) * ((D / 8 + 3) * U * sbound + U * (sbound + math.log2(max(T, 2)))) + 2 * U


class PairRef:
    """z fp64 [B,S,S,C_out]; mag the same shape; lse fp64 natural [L,B,H,T] (0 where a row has no key); sbound: max over
    layers of max_i |q_i| max_j |k_j| in the log2 domain."""

    def __init__(self, z, mag, lse, sbound, C, T, D):
        self.z, self.mag, self.lse, self.sbound, self.C, self.T, self.D = z, mag, lse, sbound, C, T, D

    def tol(self, extra_eps_p=0.0):
        kappa = eps_p(self.sbound, self.T, self.D) + extra_eps_p + (self.C + 8) * U
        return 2.0 * kappa * self.mag + 4 * U * (self.z.abs() + 1.0)


def _combine(A, M, bias, n_sym, swap_blocks, no_transpose):
    """A, M [B,S,S,C_out]: the plain sums and their magnitudes -> (z, mag) with the transpose term on the symmetric block."""
    C_out = A.shape[-1]
    sym = torch.zeros(C_out, dtype=torch.bool, device=A.device)
    if swap_blocks:
        sym[n_sym:] = True
    else:
        sym[:n_sym] = True
    if no_transpose:
        sym[:] = False
    z = A + A.transpose(1, 2) * sym.double()
    mag = M + M.transpose(1, 2) * sym.double()
    if bias is not None:
        z = z + bias.double().to(A.device)
    return z, mag


@torch.no_grad()
def pair_head_on_maps(attn, w, bias, n_sym, bos=1, eos=1, swap_blocks=False, no_transpose=False, drop=(), w_layer_shift=0):
    """attn [B,L,H,T,T] (any float dtype, taken to fp64); w [L*H, C_out]; bias [C_out] or None -> (z, mag) fp64 [B,S,S,C_out]."""
    B, L, H, T, _ = attn.shape
    S = T - bos - eos
    w3 = w.double().reshape(L, H, -1).to(attn.device)
    w3 = torch.stack([w3[(l + w_layer_shift) % L] for l in range(L)])
    for (l, h) in drop:
        w3[l, h] = 0.0
    A = torch.zeros(B, S, S, w3.shape[-1], dtype=torch.float64, device=attn.device)
    M = torch.zeros_like(A)
    for l in range(L):  # one layer at a time
        p = attn[:, l, :, bos:T - eos, bos:T - eos].double()
        A += torch.einsum("bhij,ho->bijo", p, w3[l])
        M += torch.einsum("bhij,ho->bijo", p.abs(), w3[l].abs())
    return _combine(A, M, bias, n_sym, swap_blocks, no_transpose)


@torch.no_grad()
def pair_head_ref(q_eff, k, w, bias, n_sym, key_bias=None, tokens=None, pad_idx=1, bos=1, eos=1, null_k=None, drop=(),
                  w_layer_shift=0, swap_blocks=False, no_transpose=False):
    """q_eff, k [L,B,H,T,D]; w [L*H, C_out]; bias [C_out] or None; key_bias [B,T] (0 / -inf) and / or tokens [B,T] mark <pad>.
    Returns a PairRef."""
    L, B, H, T, D = q_eff.shape
    dev = q_eff.device
    S = T - bos - eos
    pad = torch.zeros(B, T, dtype=torch.bool, device=dev)
    if key_bias is not None:
        pad |= key_bias.ne(0)
    if tokens is not None:
        pad |= tokens.eq(pad_idx)
    kb = torch.where(pad, float("-inf"), 0.0).double()
    keep = (~pad).double()
    mm = (keep[:, :, None] * keep[:, None, :])[:, bos:T - eos, bos:T - eos]  # [B,S,S]
    w3 = w.double().reshape(L, H, -1).to(dev)
    C_out = w3.shape[-1]
    drop = set(drop)
    A = torch.zeros(B, S, S, C_out, dtype=torch.float64, device=dev)
    M = torch.zeros_like(A)
    lse_all = torch.zeros(L, B, H, T, dtype=torch.float64, device=dev)
    sbound = 0.0
    for l in range(L):
        wl = w3[(l + w_layer_shift) % L].clone()
        for h in range(H):
            if (l, h) in drop:
                wl[h] = 0.0
        for bi in range(B):  # one [H, T, T] at a time
            qb, kv = q_eff[l, bi].double(), k[l, bi].double()
            sbound = max(sbound, LOG2E * qb.norm(dim=-1).max().item() * kv.norm(dim=-1).max().item())
            s = qb @ kv.transpose(-1, -2) + kb[bi][None, None, :]
            cols = s
            if null_k is not None:  # ESM-1: one more key in the softmax, no column in the map
                s0 = torch.einsum("htd,hd->ht", qb, null_k[l].double())
                sbound = max(sbound, LOG2E * qb.norm(dim=-1).max().item() * null_k[l].double().norm(dim=-1).max().item())
                cols = torch.cat([s, s0[..., None]], -1)
            lse = torch.logsumexp(cols, dim=-1)
            lse = torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse))  # a row with no key: masked below
            lse_all[l, bi] = lse
            p = torch.exp(s - lse[..., None])[:, bos:T - eos, bos:T - eos]
            p = torch.where(mm[bi].bool()[None], p, torch.zeros_like(p))
            A[bi] += torch.einsum("hij,ho->ijo", p, wl)
            M[bi] += torch.einsum("hij,ho->ijo", p, wl.abs())
    z, mag = _combine(A, M, bias, n_sym, swap_blocks, no_transpose)
    return PairRef(z, mag, lse_all, sbound, L * H, T, D)


def check_against_ref(got, ref, where="", extra_eps_p=0.0):
    """Every element of got fp32 [B,S,S,C_out] within the bound; returns the largest |got - ref| / tol."""
    assert tuple(got.shape) == tuple(ref.z.shape), (where, tuple(got.shape), tuple(ref.z.shape))
    g = got.double()
    assert torch.isfinite(g).all(), (where, "not finite")
    d = (g - ref.z).abs()
    tol = ref.tol(extra_eps_p)
    ratio = (d / tol).max().item()
    assert ratio <= 1.0, (where, "max |got - ref| / tol", ratio, "max |got - ref|", d.max().item())
    return ratio


def discrimination(ref, mutated):
    """max over elements of |z_mutated - z_ref| / tol: how many times the bound a mutation moves the output."""
    return ((mutated.z - ref.z).abs() / ref.tol()).max().item()


@torch.no_grad()
def distogram_energy_ref(logits, target, min_sep=0, inv_temp=1.0, eps=1e-8):
    """get_cce_loss (examples/lm-design/utils/loss.py:10-29) in fp64 on probs = softmax(inv_temp * logits): logits [B,S,S,n],
    target integer [S,S] (255 = ignore) -> (energy fp64 [B], count): mean of -log(p[target] + eps) over ALL ordered pairs with
    target < n and |i - j| >= min_sep; no such pair: 0."""
    B, S, _, n = logits.shape
    t = torch.as_tensor(target).long().to(logits.device)
    idx = torch.arange(S, device=logits.device)
    mask = (t < n) & ((idx[:, None] - idx[None, :]).abs() >= min_sep)
    probs = torch.softmax(logits.double() * inv_temp, -1)
    labels = torch.nn.functional.one_hot(t.clamp(max=n - 1), n).double()
    cce = -(labels[None] * torch.log(probs + eps)).sum(-1)  # [B,S,S]
    cnt = int(mask.sum())
    if cnt == 0:
        return torch.zeros(B, dtype=torch.float64, device=logits.device), 0
    return (cce * mask.double()[None]).sum((1, 2)) / cnt, cnt
