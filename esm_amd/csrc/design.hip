// design.hip — Metropolis-Hastings design toward a target contact map on the device (esm_amd/design.py): the uniform single-site
// proposal of lm-design (examples/lm-design/utils/fixedbb.py), the structure term of the energy as the cross-entropy between
// the predicted contact map and a target map, the acceptance test and the Hastings correction of the LM proposal.  None of
// them is a hot loop: the layer stack in front of every acceptance is the time.  A step is propose -> esmk_op_substitute_rows ->
// esmk_forward_rows_contacts -> esmk_op_sum_target_rows -> contact energy -> accept on one stream, and every random number is
// addressed by (seed, chain id, step, purpose, 0): a chain proposes and accepts the same alone, in a batch and in any launch
// geometry.  No atomics; every sum is fp64 in an order fixed by the shape alone.
#include "common.h"
#include "kernels.h"
#include "philox.h"
#include <algorithm>

// Every fp64 result below is compared bit for bit with separately rounded operations: no fused multiply-adds in this file
#pragma clang fp contract(off)

namespace esmk {

// One lane per chain c: the words x, y of the generator at counter (chain_id[c], step, 2, 0).
//   site = pos[lo + mulhi32(x, len)], (lo, hi) = pos_off[c], pos_off[c + 1] clamped to [0, total], len = hi - lo; an empty list, or
//          a site outside [0, T), proposes nothing: site -1, old -1, token -1
//   old  = tokens[slot, site], slot = slot[c] (clamped to [0, B)) or c when slot is null
//   cand = the bits of `allowed` below V, minus old with force_new; token = the set bit number mulhi32(y, popcount(cand)) of cand
//          in ascending token order, -1 when there is none
// Integer arithmetic only.
__global__ __launch_bounds__(256) void propose_mutations_kernel(const int64_t* __restrict__ tokens, const int* __restrict__ slot,
                                                                const int* __restrict__ pos_off, const int* __restrict__ pos,
                                                                const int* __restrict__ chain_id, unsigned long long allowed,
                                                                int force_new, unsigned long long seed, int step,
                                                                int* __restrict__ site_out, int* __restrict__ old_out,
                                                                int* __restrict__ tok_out, int n_chain, int B, int T, int total,
                                                                int V) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t c = (size_t)blockIdx.x * 256 + threadIdx.x; c < (size_t)n_chain; c += stride) {
        const int lo = min(max(pos_off[c], 0), total), hi = min(max(pos_off[c + 1], 0), total);
        const int len = hi - lo;
        int site = -1, old = -1, tok = -1;
        if (len > 0) {
            const Philox4 w = philox4x32_10((unsigned)chain_id[c], (unsigned)step, kPurposeProposal, 0u, (unsigned)seed,
                                            (unsigned)(seed >> 32));
            const int p = pos[lo + (int)__umulhi(w.x, (unsigned)len)];
            if (p >= 0 && p < T) {
                site = p;
                const int b = slot != nullptr ? min(max(slot[c], 0), B - 1) : min((int)c, B - 1);
                old = (int)tokens[(size_t)b * T + p];
                unsigned long long cand = V < 64 ? allowed & ((1ull << V) - 1) : allowed;
                if (force_new && old >= 0 && old < V) cand &= ~(1ull << old);
                const int n_cand = __popcll(cand);
                if (n_cand > 0) {
                    int k = (int)__umulhi(w.y, (unsigned)n_cand);  // 0 .. n_cand - 1
                    for (; k > 0; --k) cand &= cand - 1;             // drop the k lowest set bits
                    tok = __ffsll((long long)cand) - 1;
                }
            }
        }
        site_out[c] = site;
        old_out[c] = old;
        tok_out[c] = tok;
    }
}

hipError_t launch_propose_mutations(const int64_t* tokens, const int* slot, const int* pos_off, const int* pos, const int* chain_id,
                                    unsigned long long allowed, int force_new, unsigned long long seed, int step, int* site_out,
                                    int* old_out, int* tok_out, int n_chain, int B, int T, int total, int V, hipStream_t st) {
    if (!tokens || !pos_off || !pos || !chain_id || !site_out || !old_out || !tok_out || n_chain <= 0 || B <= 0 || T <= 0 ||
        total < 0 || V <= 0 || V > 64)
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)std::min<size_t>(((size_t)n_chain + 255) / 256, 8192);
    hipLaunchKernelGGL(propose_mutations_kernel, dim3(blocks), dim3(256), 0, st, tokens, slot, pos_off, pos, chain_id, allowed,
                       force_new, seed, step, site_out, old_out, tok_out, n_chain, B, T, total, V);
    return hipGetLastError();
}

// The structure term of one chain per workgroup (grid-stride over the chains).  Element e = i * S + j of the chain's map counts
// when j - i >= min_sep (so i < j) and target[e] != 2.  p = the fp32 probability clamped to [2^-24, 1 - 2^-24] (both fp32
// values; a NaN becomes a bound), taken to fp64.
//   kind 0  term = log p on target contacts, nothing elsewhere; count = the target contacts that count
//   kind 1  term = log p on target contacts, log(1 - p) on the others; count = the pairs that count
// Lane t adds the terms of e = t, t + 256, ... in that order; the 64 lane sums of a wavefront are added in a butterfly, the four
// wavefront sums in wavefront order: the order of addition is a function of S, min_sep and the target alone.
// energy = -(sum / count), 0.0 when count == 0.
__global__ __launch_bounds__(256) void contact_energy_kernel(const float* __restrict__ contacts, const unsigned char* __restrict__ target,
                                                             double* __restrict__ energy_out, int* __restrict__ count_out, int B, int S,
                                                             int min_sep, int kind) {
    __shared__ double wave_sum[4];
    __shared__ int wave_count[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = S * S;  // S <= 32768
    for (int b = blockIdx.x; b < B; b += gridDim.x) {  // block uniform
        const float* p = contacts + (size_t)b * (size_t)n;
        double sum = 0.0;
        int count = 0;
        for (int e = tid; e < n; e += 256) {
            const int i = e / S, j = e - i * S;
            if (j - i < min_sep) continue;
            const unsigned char y = target[e];
            if (y == 2 || (kind == 0 && y != 1)) continue;
            const double q = (double)fminf(fmaxf(p[e], 0x1p-24f), 1.0f - 0x1p-24f);
            sum += log(y == 1 ? q : 1.0 - q);
            ++count;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sum += __shfl_xor(sum, o, 64);
            count += __shfl_xor(count, o, 64);
        }
        __syncthreads();  // the sums of the chain before this one have been read
        if (lane == 0) wave_sum[wave] = sum, wave_count[wave] = count;
        __syncthreads();
        if (tid == 0) {
            const double total = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
            const int cnt = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
            energy_out[b] = cnt > 0 ? -(total / (double)cnt) : 0.0;
            count_out[b] = cnt;
        }
    }
}

hipError_t launch_contact_energy(const float* contacts, const unsigned char* target, double* energy_out, int* count_out, int B, int S,
                                 int min_sep, int kind, hipStream_t st) {
    if (!contacts || !target || !energy_out || !count_out || B <= 0 || S <= 0 || S > 32768 || min_sep < 1 || kind < 0 || kind > 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(contact_energy_kernel, dim3((unsigned)std::min(B, 8192)), dim3(256), 0, st, contacts, target, energy_out,
                       count_out, B, S, min_sep, kind);
    return hipGetLastError();
}

// One lane per chain c, everything in fp64 with one rounding per operation (no contraction into fused multiply-adds).  The one
// acceptance kernel: esmk_op_mh_accept gives a scalar temperature and no third term, esmk_op_mh_accept_ex (replica exchange and
// the n-gram term, tempering.hip) a temperature per chain and e_extra.
//   e_lm  = -(lp_sum[c] / n_res[c]) (0 without lp_sum or with n_res[c] <= 0), e_c = e_contact[c] (0 without e_contact)
//   E'    = (w_contact * e_c + w_lm * e_lm) + w_extra * e_extra[c]; without e_extra the last addition is not made
//   dE    = E' - e_cur[c],  h = hastings[c] or 0
//   u     = (x >> 8) * 2^-24, x the first word of the generator at counter (chain_id[c], step, 3, 0)
//   inv_t = inv_t_tab[clamp(rung[c], 0, n_rung - 1)] (rung null: entry 0); inv_t_tab null: the scalar inv_t0 (no table to
//           allocate or upload for one temperature)
//   a     = -dE * inv_t + h;  accept iff tok[c] >= 0 and (a >= 0 or u < exp(a));  inv_t == +inf (greedy): accept iff tok[c] >= 0
//           and dE <= 0.  A NaN anywhere rejects.
// On acceptance tokens[slot, site[c]] = tok[c] (a site outside [0, T) writes no token), e_cur[c] = E', and the components
// e_contact_cur[c] = e_c, e_lm_cur[c] = e_lm, e_extra_cur[c] = e_extra[c] where those arrays are given.  accepted, u and E' are
// written for every chain.
__global__ __launch_bounds__(256) void mh_accept_kernel(int64_t* __restrict__ tokens, const int* __restrict__ slot,
                                                        const int* __restrict__ site, const int* __restrict__ tok,
                                                        const int* __restrict__ chain_id, const double* __restrict__ e_contact,
                                                        const double* __restrict__ lp_sum, const int* __restrict__ n_res,
                                                        const double* __restrict__ hastings, const double* __restrict__ e_extra,
                                                        double w_contact, double w_lm, double w_extra,
                                                        const double* __restrict__ inv_t_tab, double inv_t0,
                                                        const int* __restrict__ rung, int n_rung, unsigned long long seed, int step,
                                                        double* __restrict__ e_cur, double* __restrict__ e_contact_cur,
                                                        double* __restrict__ e_lm_cur, double* __restrict__ e_extra_cur,
                                                        unsigned char* __restrict__ accepted_out, double* __restrict__ u_out,
                                                        double* __restrict__ e_prop_out, int n_chain, int B, int T) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t c = (size_t)blockIdx.x * 256 + threadIdx.x; c < (size_t)n_chain; c += stride) {
        const double e_c = e_contact != nullptr ? e_contact[c] : 0.0;
        double e_lm = 0.0;
        if (lp_sum != nullptr && n_res != nullptr && n_res[c] > 0) e_lm = -(lp_sum[c] / (double)n_res[c]);
        const double a_c = w_contact * e_c, a_lm = w_lm * e_lm;
        double e_prop = a_c + a_lm;
        double e_x = 0.0;
        if (e_extra != nullptr) {
            e_x = e_extra[c];
            const double a_x = w_extra * e_x;
            e_prop = e_prop + a_x;
        }
        const double dE = e_prop - e_cur[c];
        const double h = hastings != nullptr ? hastings[c] : 0.0;
        const double u = (double)(philox_word0(seed, chain_id[c], step, kPurposeAcceptance, 0) >> 8) * 0x1p-24;
        double inv_temperature = inv_t0;
        if (inv_t_tab != nullptr) inv_temperature = inv_t_tab[rung != nullptr ? min(max(rung[c], 0), n_rung - 1) : 0];
        const int t = tok[c];
        bool accept;
        if (inv_temperature == (double)INFINITY) {
            accept = t >= 0 && dE <= 0.0;
        } else {
            const double scaled = -dE * inv_temperature;
            const double a = scaled + h;
            accept = t >= 0 && (a >= 0.0 || u < exp(a));
        }
        if (accept) {
            const int p = site[c];
            if (p >= 0 && p < T) {
                const int b = slot != nullptr ? min(max(slot[c], 0), B - 1) : min((int)c, B - 1);
                tokens[(size_t)b * T + p] = (int64_t)t;
            }
            e_cur[c] = e_prop;
            if (e_contact_cur != nullptr) e_contact_cur[c] = e_c;
            if (e_lm_cur != nullptr) e_lm_cur[c] = e_lm;
            if (e_extra_cur != nullptr && e_extra != nullptr) e_extra_cur[c] = e_x;
        }
        accepted_out[c] = accept ? 1 : 0;
        if (u_out != nullptr) u_out[c] = u;
        if (e_prop_out != nullptr) e_prop_out[c] = e_prop;
    }
}

hipError_t launch_mh_accept(int64_t* tokens, const int* slot, const int* site, const int* tok, const int* chain_id,
                            const double* e_contact, const double* lp_sum, const int* n_res, const double* hastings,
                            const double* e_extra, double w_contact, double w_lm, double w_extra, const double* inv_t_tab,
                            double inv_t0, const int* rung, int n_rung, unsigned long long seed, int step, double* e_cur,
                            double* e_contact_cur, double* e_lm_cur, double* e_extra_cur, unsigned char* accepted_out, double* u_out,
                            double* e_prop_out, int n_chain, int B, int T, hipStream_t st) {
    if (!tokens || !site || !tok || !chain_id || !e_cur || !accepted_out || n_chain <= 0 || B <= 0 || T <= 0 ||
        (lp_sum != nullptr && n_res == nullptr) || (inv_t_tab != nullptr ? n_rung <= 0 : !(inv_t0 >= 0.0)))
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)std::min<size_t>(((size_t)n_chain + 255) / 256, 8192);
    hipLaunchKernelGGL(mh_accept_kernel, dim3(blocks), dim3(256), 0, st, tokens, slot, site, tok, chain_id, e_contact, lp_sum, n_res,
                       hastings, e_extra, w_contact, w_lm, w_extra, inv_t_tab, inv_t0, rung, n_rung, seed, step, e_cur,
                       e_contact_cur, e_lm_cur, e_extra_cur, accepted_out, u_out, e_prop_out, n_chain, B, T);
    return hipGetLastError();
}

// h[c] = (double)inv_t_prop * ((double)lp[c, old[c]] - (double)lp[c, new[c]]): the log ratio of the reverse and the forward
// proposal of a draw from softmax(lp * inv_t_prop) over one candidate set in one context (their normalisers cancel).  Exact
// fp64 operations on fp32 inputs, one rounding each.  A token outside [0, V) on either side (nothing was proposed): h = 0.
__global__ __launch_bounds__(256) void hastings_rows_kernel(const float* __restrict__ lp, const int* __restrict__ old_tok,
                                                            const int* __restrict__ new_tok, float inv_t_prop,
                                                            double* __restrict__ h_out, int n, int V) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t c = (size_t)blockIdx.x * 256 + threadIdx.x; c < (size_t)n; c += stride) {
        const int a = old_tok[c], b = new_tok[c];
        double h = 0.0;
        if (a >= 0 && a < V && b >= 0 && b < V)
            h = (double)inv_t_prop * ((double)lp[c * V + a] - (double)lp[c * V + b]);
        h_out[c] = h;
    }
}

hipError_t launch_hastings_rows(const float* lp, const int* old_tok, const int* new_tok, float inv_t_prop, double* h_out, int n, int V,
                                hipStream_t st) {
    if (!lp || !old_tok || !new_tok || !h_out || n <= 0 || V <= 0) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)std::min<size_t>(((size_t)n + 255) / 256, 8192);
    hipLaunchKernelGGL(hastings_rows_kernel, dim3(blocks), dim3(256), 0, st, lp, old_tok, new_tok, inv_t_prop, h_out, n, V);
    return hipGetLastError();
}

}  // namespace esmk
