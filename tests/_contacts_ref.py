"""fp64 contact head that streams over channels, and the fp32 error bound of the fused contact kernels.

The reference (esm/modules.py:27-41, 338-357 on the attention maps of esm/model/esm2.py:119-139) needs every channel's
map only through

    A = sum_c w_c (P_c + P_c^T),   r_c = row sums of (P_c + P_c^T),   t_c = sum r_c,
    logit = A - sum_c (w_c / t_c) r_c r_c^T + bias

with P_c the softmax of channel c = (layer, head) with <pad>, <eos> and the cropped first / last position zeroed.  So a
reference can take the layers one at a time and never hold [B, L, H, T, T]: a 1920-channel case costs one layer's
[H, T, T] at a time.  The operands are the kernel's own: q_effective (natural domain, ``ops.to_log2_domain``), k as
rounded to the operand dtype.  The row log-sum-exp it hands back (``lse``) is the fp64 one, for the kernel to take.

Mutation knobs (for showing that the bound discriminates): ``drop`` = channels to leave out, ``w_layer_shift`` = use
layer (l + shift) % L's weights for layer l, ``apc_upto`` = only the first apc_upto channels in the apc term (what
skipping the final kernel's last 32-channel slab does)."""
import math

import torch

U = 2.0 ** -24  # fp32 unit roundoff
LOG2E = 1.4426950408889634


def residue_mask(tokens, pad_idx=1, eos_idx=2, bos=1, eos=1):
    """m[b, t] = 1 for a residue: not <pad>, not <eos> (when the layout appends one), inside the crop."""
    B, T = tokens.shape
    t = torch.arange(T, device=tokens.device)
    m = (t >= bos) & (t < T - eos) & tokens.ne(pad_idx)
    if eos:
        m &= tokens.ne(eos_idx)
    return m


class ContactRef:
    """z: fp64 logits [B,S,S]; mag: sum_c |w_c| (|a_c| + r_c r_c^T / t_c) [B,S,S] (the size of what the kernel sums);
    lse: fp64 natural row log-sum-exp [L,B,H,T]; sbound: max over layers of max_i |q_i| max_j |k_j| in the log2 domain
    (>= every |sum_d q_d k_d| the kernel forms)."""

    def __init__(self, z, mag, lse, sbound, C, T, D):
        self.z, self.mag, self.lse, self.sbound, self.C, self.T, self.D = z, mag, lse, sbound, C, T, D

    @property
    def prob(self):
        return torch.sigmoid(self.z)

    def tol(self):
        """Bound on |logit_kernel - logit_ref| per element, from the kernel's fp32 arithmetic:
          - score s = q.k over D products (exact in fp32) by chained MFMA: <= (D/8 + 3) u sbound;
          - lse rounded to fp32: <= u (sbound + log2 T);  2^x by v_exp_f32: 1 ulp.  So each P carries a relative
            error <= eps_p = ln2 ((D/8 + 3) u sbound + u (sbound + log2 T)) + 2u;
          - fp32 sums in any order over <= T keys (r_c), <= C channels (A, apc) and G groups: <= (T + C + 8) u of the
            sum of magnitudes;
        applied to mag = sum_c |w_c| (|a_c| + r_c r_c^T / t_c), plus the rounding of the bias add."""
        eps_p = math.log(2.0) * ((self.D / 8 + 3) * U * self.sbound + U * (self.sbound + math.log2(self.T))) + 2 * U
        kappa = eps_p + (self.T + self.C + 8) * U
        return 2.0 * kappa * self.mag + 4 * U * (self.z.abs() + 1.0)


@torch.no_grad()
def contact_ref(q_eff, k, tokens, w, b, key_bias=None, pad_idx=1, eos_idx=2, bos=1, eos=1, drop=(), w_layer_shift=0,
                apc_upto=None):
    """q_eff, k: [L, B, H, T, D] (any float dtype; the values are taken as they are); tokens [B, T]; w [L*H]; b scalar or
    [1]; key_bias [B, T] (0 / -inf) or None.  Returns a ContactRef."""
    L, B, H, T, D = q_eff.shape
    C = L * H
    dev = q_eff.device
    m = residue_mask(tokens, pad_idx, eos_idx, bos, eos).double()
    S = T - bos - eos
    mm = (m[:, :, None] * m[:, None, :])[:, bos:T - eos, bos:T - eos]  # [B,S,S]
    kb = torch.zeros(B, T, dtype=torch.float64, device=dev) if key_bias is None else key_bias.double()
    w = w.reshape(L, H).double().to(dev)
    bb = float(torch.as_tensor(b).double().reshape(-1)[0]) if b is not None else 0.0
    A = torch.zeros(B, S, S, dtype=torch.float64, device=dev)
    apc = torch.zeros_like(A)
    mag = torch.zeros_like(A)
    lse_all = torch.empty(L, B, H, T, dtype=torch.float64, device=dev)
    drop = set(drop)
    sbound = 0.0
    for l in range(L):
        wl = w[(l + w_layer_shift) % L]
        keep_h = torch.tensor([(l, h) not in drop for h in range(H)], dtype=torch.float64, device=dev)
        apc_h = keep_h.clone()
        if apc_upto is not None:
            apc_h *= (torch.arange(H, device=dev) + l * H < apc_upto).double()
        for bi in range(B):  # one [H, T, T] at a time
            qb = q_eff[l, bi].double()
            kbv = k[l, bi].double()
            sbound = max(sbound, LOG2E * qb.norm(dim=-1).max().item() * kbv.norm(dim=-1).max().item())
            s = qb @ kbv.transpose(-1, -2) + kb[bi][None, None, :]
            lse = torch.logsumexp(s, dim=-1)
            lse_all[l, bi] = lse
            p = torch.exp(s - lse[..., None])[:, bos:T - eos, bos:T - eos] * mm[bi]
            a = p + p.transpose(-1, -2)
            r = a.sum(-1)  # [H, S]
            t = r.sum(-1)  # [H]
            rr = r[:, :, None] * r[:, None, :]
            A[bi] += torch.einsum("h,hij->ij", wl * keep_h, a)
            apc[bi] += torch.einsum("h,hij->ij", wl * apc_h / t, rr)
            mag[bi] += torch.einsum("h,hij->ij", wl.abs() * keep_h, a + rr / t[:, None, None])
            del s, p, a, rr
    return ContactRef(A - apc + bb, mag, lse_all, sbound, C, T, D)


def kernel_lse(lse_nat):
    """What the kernel takes: fp32(lse * log2 e) from the fp64 natural lse (ops.contacts_fused does the conversion
    in fp64, so passing the fp64 lse hands the kernel exactly this)."""
    return (lse_nat.double() * LOG2E).float()


def check_against_ref(got, ref, where=""):
    """got: fp32 [B,S,S] maps of the kernel.  NaN exactly where the reference's 0/0 puts it; elsewhere the
    probabilities within p(1-p) tol + 4u, and the unsaturated logits (0.01 <= p_ref <= 0.99) within
    tol + 8u / (p (1 - p)) (the fp32 rounding of p seen through the logit)."""
    z = ref.z
    nan_ref = torch.isnan(z)
    assert torch.equal(torch.isnan(got), nan_ref), (where, "NaN pattern", torch.isnan(got).sum().item(),
                                                      nan_ref.sum().item())
    ok = ~nan_ref
    tol = ref.tol()[ok]
    p_ref = torch.sigmoid(z[ok])
    g = got[ok].double()
    assert torch.isfinite(g).all(), where
    dp = (g - p_ref).abs()
    ptol = p_ref * (1 - p_ref) * tol * 1.01 + 4 * U
    bad = dp > ptol
    assert not bad.any(), (where, "prob", dp.max().item(), (dp / ptol).max().item())
    uns = (p_ref >= 0.01) & (p_ref <= 0.99)
    if uns.any():
        gz = torch.log(g[uns] / (1 - g[uns]))
        pu = p_ref[uns]
        dz = (gz - z[ok][uns]).abs()
        ztol = tol[uns] + 8 * U / (pu * (1 - pu))
        assert not (dz > ztol).any(), (where, "logit", dz.max().item(), (dz / ztol).max().item())
    return (dp / ptol).max().item() if dp.numel() else 0.0


def discrimination(ref, mutated):
    """max over elements of |logit_mutated - logit_ref| / tol: how many times the bound a mutation moves the output."""
    ok = torch.isfinite(ref.z) & torch.isfinite(mutated.z)
    return ((mutated.z - ref.z).abs()[ok] / ref.tol()[ok]).max().item()
