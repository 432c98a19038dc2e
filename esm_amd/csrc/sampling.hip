// sampling.hip — drawing sequences from the model on the device (esm_amd/sampling.py: Gibbs sweeps, mask in-painting): a
// counter-addressed random number generator, the per-chain shuffle of the designable positions, the draw of one token from
// a row of log-probabilities and the write-back into the token matrix.  None of them is a hot loop: the layer stack in
// front of every draw is the time.  A sampling step is mask (esmk_op_mask_rows_multi) -> esmk_forward_rows -> draw -> commit
// on one stream, and every random number is addressed by (seed, chain id, epoch or step, purpose, index): it depends on
// nothing else, so a chain draws the same tokens alone, in a batch, and in any launch geometry.
#include "common.h"
#include "kernels.h"
#include <algorithm>

namespace esmk {

// Plain Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): multipliers 0xD2511F53 /
// 0xCD9E8D57, the key bumped by 0x9E3779B9 / 0xBB67AE85 between the ten rounds.
struct Philox4 {
    unsigned x, y, z, w;
};
__host__ __device__ inline Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return Philox4{c0, c1, c2, c3};
}

constexpr unsigned kPurposePermutation = 0, kPurposeToken = 1;  // counter word 2

// First output word of the generator at counter (chain, epoch_or_step, purpose, index) under key (seed lo, seed hi).
__device__ inline unsigned philox_word0(unsigned long long seed, int chain, int epoch_or_step, unsigned purpose, int index) {
    return philox4x32_10((unsigned)chain, (unsigned)epoch_or_step, purpose, (unsigned)index, (unsigned)seed,
                         (unsigned)(seed >> 32)).x;
}

// perm_out[lo : hi] = a Fisher-Yates shuffle of pos_in[lo : hi], (lo, hi) = pos_off[c], pos_off[c + 1]: for i = len - 1 .. 1,
// j = mulhi32(word0(chain_id[c], epoch, 0, i), i + 1), swap elements i and j.  One lane per chain runs the loop (a list is at
// most T long), so the order of the swaps is fixed; the slices are disjoint, so no two lanes write the same element.  Integer
// arithmetic only.  The offsets are device data: clamped to [0, total], a pair with hi < lo is an empty list.
__global__ __launch_bounds__(256) void permute_positions_kernel(const int* __restrict__ pos_off, const int* __restrict__ pos_in,
                                                                const int* __restrict__ chain_id, int* __restrict__ perm_out,
                                                                int n_chain, int total, unsigned long long seed, int epoch) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t c = (size_t)blockIdx.x * 256 + threadIdx.x; c < (size_t)n_chain; c += stride) {
        const int lo = min(max(pos_off[c], 0), total), hi = min(max(pos_off[c + 1], 0), total);
        const int len = hi - lo;
        if (len <= 0) continue;
        const int chain = chain_id[c];
        int* p = perm_out + lo;
        for (int i = 0; i < len; ++i) p[i] = pos_in[lo + i];
        for (int i = len - 1; i >= 1; --i) {
            const int j = (int)__umulhi(philox_word0(seed, chain, epoch, kPurposePermutation, i), (unsigned)(i + 1));  // 0 .. i
            const int a = p[i], b = p[j];
            p[i] = b;
            p[j] = a;
        }
    }
}

hipError_t launch_permute_positions(const int* pos_off, const int* pos_in, const int* chain_id, int* perm_out, int n_chain,
                                    int total, unsigned long long seed, int epoch, hipStream_t st) {
    if (!pos_off || !pos_in || !chain_id || !perm_out || n_chain <= 0 || total <= 0) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)std::min<size_t>(((size_t)n_chain + 255) / 256, 8192);
    hipLaunchKernelGGL(permute_positions_kernel, dim3(blocks), dim3(256), 0, st, pos_off, pos_in, chain_id, perm_out, n_chain,
                       total, seed, epoch);
    return hipGetLastError();
}

// One token per row of log-probabilities [n, V], V <= 64: one wavefront per row, one vocabulary entry per lane.
//   u      = (word0(row_chain[i], step, 1, row_index[i]) >> 8) * 2^-24: exact in fp32, in [0, 1)
//   cand   = the bits of allowed_mask below V, minus the token exclude[i] (when that is inside [0, V))
//   inv_temperature > 0:  z_v = lp[v] * inv_temperature, m = max over cand of z, w_v = expf(z_v - m) on cand (0 elsewhere);
//          the running sum c_v = w_0 + ... + w_v is added in fp32 in ascending token order — every lane walks the lanes
//          0 .. 63 through a shuffle and adds the ones at or below itself, so lane v holds exactly the sequential sum and the
//          last lane the total; token = the first candidate with c_v > u * total, the last candidate if there is none;
//          logq = z_tok - m - log(total), taken in fp64 from the fp32 inputs and rounded to fp32 once
//   inv_temperature == 0: the candidate with the largest lp, ties to the lowest index; logq = 0
//   cand empty: token = -1, logq = 0
//   every candidate at -inf (no log_softmax of finite logits gives that): m = -inf, every w is NaN, no running sum exceeds
//          the threshold: token = the last candidate, logq = NaN.  Greedy takes the lowest candidate (all tie at -inf).
// Nothing depends on the row's place in the launch.  expf is the precise one.
__global__ __launch_bounds__(256) void sample_rows_kernel(const float* __restrict__ lp, const int* __restrict__ row_chain,
                                                          const int* __restrict__ row_index, const int* __restrict__ exclude,
                                                          unsigned long long allowed, float inv_temperature,
                                                          unsigned long long seed, int step, int* __restrict__ token_out,
                                                          float* __restrict__ logq_out, float* __restrict__ u_out, int n, int V) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;  // wave uniform
    const float u = (float)(philox_word0(seed, row_chain[row], step, kPurposeToken, row_index[row]) >> 8) * 0x1p-24f;
    unsigned long long cand = V < 64 ? allowed & ((1ull << V) - 1) : allowed;
    if (exclude != nullptr) {
        const int ex = exclude[row];
        if (ex >= 0 && ex < V) cand &= ~(1ull << ex);
    }
    const bool mine = (cand >> lane) & 1ull;  // lanes at or past V never are
    const float x = mine ? lp[(size_t)row * V + lane] : -INFINITY;
    int token = -1;
    float logq = 0.f;
    if (cand != 0ull) {  // wave uniform
        const float z = inv_temperature > 0.f ? x * inv_temperature : x;  // (-inf stays -inf: inv_temperature > 0)
        float m = z;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if (inv_temperature > 0.f) {
            const float w = mine ? expf(z - m) : 0.f;
            float cum = 0.f;
            for (int v = 0; v < V; ++v) {  // ascending token order, the same additions in every lane up to its own entry
                const float wv = __shfl(w, v, 64);
                if (v <= lane) cum += wv;
            }
            const float total = __shfl(cum, V - 1, 64);
            const float thr = u * total;
            const unsigned long long over = __ballot(mine && cum > thr);
            token = over != 0ull ? __ffsll((long long)over) - 1 : 63 - __clzll((long long)cand);
            // logq in fp64 from the fp32 inputs, rounded once: the fp32 chain z_tok - m - logf(total) lost up to 1.2 ulp of the
            // result (5.6e-7 at logq = -4.9).  Butterfly reductions: every lane ends with the same bits.
            const double zd = mine ? (double)x * (double)inv_temperature : -INFINITY;
            double md = zd;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) md = fmax(md, __shfl_xor(md, o, 64));
            double sd = mine ? exp(zd - md) : 0.0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sd += __shfl_xor(sd, o, 64);
            logq = (float)(__shfl(zd, token, 64) - md - log(sd));
        } else {
            const unsigned long long top = __ballot(mine && x == m);  // (a row of NaNs only: no lane; the last candidate)
            token = top != 0ull ? __ffsll((long long)top) - 1 : 63 - __clzll((long long)cand);
        }
    }
    if (lane == 0) {
        token_out[row] = token;
        logq_out[row] = logq;
        if (u_out != nullptr) u_out[row] = u;
    }
}

hipError_t launch_sample_rows(const float* lp, const int* row_chain, const int* row_index, const int* exclude,
                              unsigned long long allowed, float inv_temperature, unsigned long long seed, int step,
                              int* token_out, float* logq_out, float* u_out, int n, int V, hipStream_t st) {
    if (!lp || !row_chain || !row_index || !token_out || !logq_out || n <= 0 || V <= 0 || V > 64 || !(inv_temperature >= 0.f))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, lp, row_chain, row_index, exclude,
                       allowed, inv_temperature, seed, step, token_out, logq_out, u_out, n, V);
    return hipGetLastError();
}

// tokens[slot[i], pos[i]] = token[i] on int64 [B, T]: the write-back of a sampling step.  A row with token < 0 (an empty
// candidate set) or a position outside [0, T) writes nothing; a slot outside [0, B) is clamped.  The (slot, pos) pairs of a
// call are distinct by contract, so no two lanes write the same element.
__global__ __launch_bounds__(256) void commit_tokens_kernel(int64_t* __restrict__ tokens, const int* __restrict__ slot,
                                                            const int* __restrict__ pos, const int* __restrict__ token, int n,
                                                            int B, int T) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += stride) {
        const int t = token[i], p = pos[i];
        if (t < 0 || p < 0 || p >= T) continue;
        const int b = min(max(slot[i], 0), B - 1);
        tokens[(size_t)b * T + p] = (int64_t)t;
    }
}

hipError_t launch_commit_tokens(int64_t* tokens, const int* slot, const int* pos, const int* token, int n, int B, int T,
                                hipStream_t st) {
    if (!tokens || !slot || !pos || !token || n <= 0 || B <= 0 || T <= 0) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)std::min<size_t>(((size_t)n + 255) / 256, 8192);
    hipLaunchKernelGGL(commit_tokens_kernel, dim3(blocks), dim3(256), 0, st, tokens, slot, pos, token, n, B, T);
    return hipGetLastError();
}

}  // namespace esmk
