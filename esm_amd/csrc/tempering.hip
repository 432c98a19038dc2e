// tempering.hip — the two things lm-design has around its energy forward that design.hip left out (esm_amd/design.py): the n-gram
// term of the energy (examples/lm-design/utils/ngram.py: a KL divergence between the n-gram frequencies of a sequence and a
// background) and replica exchange — the swap of temperatures between the neighbouring rungs of a ladder; the acceptance with a
// temperature per chain and a third energy term is mh_accept_kernel of design.hip.  As in design.hip none of them is a hot loop, every random number is
// addressed by its counter alone, there are no atomics, and every fp64 sum has an order fixed by the shape alone.
#include "common.h"
#include "kernels.h"
#include "philox.h"
#include <algorithm>

// Every fp64 result below is compared bit for bit with separately rounded operations: no fused multiply-adds in this file
#pragma clang fp contract(off)

namespace esmk {

constexpr int kNgramMaxS = 32768;
constexpr int kNgramShare = 4;  // windows of a lane counted in one walk over the chain

// The key of window i of order n over the chain's codes in LDS: sum_k code[i + k] * A^(n - 1 - k), -1 when a code is negative.
__device__ inline int ngram_key(const signed char* codes, int i, int n, int A) {
    int key = 0;
    for (int k = 0; k < n; ++k) {
        const int c = codes[i + k];
        if (c < 0) return -1;
        key = key * A + c;
    }
    return key;
}

// One workgroup of 256 lanes per chain (grid-stride over the chains).  The chain's S codes (code[token], -1 for a token outside
// [0, V) or a code outside [0, A)) are staged in LDS once.  Per chosen order n, ascending, lane t owns the windows t, t + 256, ...
// < S - n + 1: for a valid window i it walks every window j in ascending order (one walk serves kNgramShare of the lane's
// windows; every lane reads the same LDS byte at the same time), counts the valid ones (total) and those with its key (c_i), and
// is no first window once a valid j < i has its key.  A first window adds p * log(p / q_n[key]), p = c_i / total, to the lane's
// sum in window order; the 64 lane sums of a wavefront are added in a butterfly, the four wavefront sums in wavefront
// order (a window that is no first window adds nothing, which leaves a sum as adding +0.0 would): the order of addition is a
// function of S and the order mask alone.  energy = (((0.0 + KL_a) + KL_b) + ...) over the chosen orders, ascending.
__global__ __launch_bounds__(256) void ngram_energy_kernel(const int64_t* __restrict__ tokens, const int* __restrict__ code,
                                                           NgramTables q, double* __restrict__ energy_out, int B, int T, int first,
                                                           int S, int V, int A, int order_mask) {
    __shared__ signed char codes[kNgramMaxS];
    __shared__ double wave_sum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {  // block uniform
        __syncthreads();  // the codes of the chain before this one have been read
        for (int i = tid; i < S; i += 256) {
            const int64_t tok = tokens[(size_t)b * T + first + i];
            int c = -1;
            if (tok >= 0 && tok < V) c = code[tok];
            codes[i] = (signed char)(c >= 0 && c < A ? c : -1);
        }
        __syncthreads();
        double energy = 0.0;
        for (int n = 1; n <= 4; ++n) {
            if (!((order_mask >> (n - 1)) & 1)) continue;
            const double* __restrict__ qn = q.q[n - 1];
            const int W = S - n + 1;  // windows; <= 0: none
            int top = 1;              // A^(n-1): the weight of a window's first code
            for (int k = 1; k < n; ++k) top *= A;
            double sum = 0.0;
            for (int i0 = tid; i0 < W; i0 += kNgramShare * 256) {  // the lane's next kNgramShare windows share one walk
                int key[kNgramShare], count[kNgramShare];
                bool is_first[kNgramShare], any = false;
#pragma unroll
                for (int m = 0; m < kNgramShare; ++m) {
                    const int i = i0 + m * 256;
                    key[m] = i < W ? ngram_key(codes, i, n, A) : -1;
                    count[m] = 0;
                    is_first[m] = key[m] >= 0;
                    any |= is_first[m];
                }
                if (!any) continue;
                // the walk: kj is the key of window j kept rolling (a negative code counts as 0 in it), run the number of
                // codes >= 0 in a row up to the window's last one: window j is valid iff run >= n
                int total = 0, kj = 0, run = 0;
                for (int k = 0; k < n - 1; ++k) {
                    const int c = codes[k];
                    run = c >= 0 ? run + 1 : 0;
                    kj = kj * A + max(c, 0);
                }
#pragma unroll 8  // one wavefront per SIMD: the LDS reads of eight windows are in flight together
                for (int j = 0; j < W; ++j) {
                    const int c = codes[j + n - 1];
                    run = c >= 0 ? run + 1 : 0;
                    kj = kj * A + max(c, 0);
                    if (run >= n) {
                        ++total;
#pragma unroll
                        for (int m = 0; m < kNgramShare; ++m) {
                            if (kj != key[m]) continue;
                            if (j < i0 + m * 256)
                                is_first[m] = false;
                            else
                                ++count[m];
                        }
                    }
                    kj -= max((int)codes[j], 0) * top;
                }
#pragma unroll
                for (int m = 0; m < kNgramShare; ++m) {  // in window order
                    if (!is_first[m]) continue;
                    const double p = (double)count[m] / (double)total;
                    const double ratio = p / qn[key[m]];
                    sum += p * log(ratio);
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
            __syncthreads();  // the sums of the order before this one have been read
            if (lane == 0) wave_sum[wave] = sum;
            __syncthreads();
            const double kl = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
            energy += kl;
        }
        if (tid == 0) energy_out[b] = energy;
    }
}

hipError_t launch_ngram_energy(const int64_t* tokens, const int* code, const NgramTables& q, double* energy_out, int B, int T,
                               int first, int S, int V, int A, int order_mask, hipStream_t st) {
    if (!tokens || !code || !energy_out || B <= 0 || T <= 0 || first < 0 || S <= 0 || S > kNgramMaxS || (long long)first + S > T ||
        V <= 0 || A <= 0 || A > 32 || (order_mask & 15) == 0 || (order_mask & ~15) != 0)
        return hipErrorInvalidValue;
    for (int n = 1; n <= 4; ++n)
        if (((order_mask >> (n - 1)) & 1) && !q.q[n - 1]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ngram_energy_kernel, dim3((unsigned)std::min(B, 8192)), dim3(256), 0, st, tokens, code, q, energy_out, B, T,
                       first, S, V, A, order_mask);
    return hipGetLastError();
}

// Swap round r of the ladders of K consecutive slots.  One lane per (ladder l, m), m < (K + 1) / 2, with the lower rung k = 2 m +
// (r & 1).  The lane scans the K rungs of its ladder for the slot x at rung k and the slot y at rung k + 1.
//   k + 1 < K: a = (inv_t[k] - inv_t[k + 1]) * (e_cur[x] - e_cur[y]), u = (word0 >> 8) * 2^-24 at counter (ladder_id[l], r, 4, k);
//              accept iff a >= 0 or u < exp(a) (a NaN rejects): rung[x] = k + 1, rung[y] = k.  accepted and u go to x and y.
//   k + 1 == K: the last rung has no partner in this round: accepted 0, u -1 for x.  Lane m == 0 of an odd round writes the same
//              for the slot at rung 0.
// The rungs a lane writes are those of its own pair, which no other lane of the round reads as anything but "not mine": plain
// stores, nothing races.  A ladder that holds no permutation of 0 .. K - 1 swaps only the pairs it finds.
__global__ __launch_bounds__(256) void replica_swap_kernel(int* __restrict__ rung, const double* __restrict__ e_cur,
                                                           const double* __restrict__ inv_t, const int* __restrict__ ladder_id,
                                                           unsigned long long seed, int round, unsigned char* __restrict__ accepted_out,
                                                           double* __restrict__ u_out, int n_ladder, int K) {
    const int per = (K + 1) / 2, odd = round & 1;
    const size_t n_lane = (size_t)n_ladder * per, stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_lane; i += stride) {
        const int l = (int)(i / per), m = (int)(i - (size_t)l * per);
        const int k = 2 * m + odd;
        const size_t base = (size_t)l * K;
        int x = -1, y = -1, s0 = -1;
        for (int s = 0; s < K; ++s) {
            const int v = rung[base + s];
            if (v == k) x = s;
            if (v == k + 1) y = s;
            if (v == 0) s0 = s;
        }
        if (m == 0 && odd && s0 >= 0) {
            accepted_out[base + s0] = 0;
            u_out[base + s0] = -1.0;
        }
        if (k + 1 < K) {
            if (x < 0 || y < 0) continue;
            const double d_t = inv_t[k] - inv_t[k + 1];
            const double d_e = e_cur[base + x] - e_cur[base + y];
            const double a = d_t * d_e;
            const double u = (double)(philox_word0(seed, ladder_id[l], round, kPurposeSwap, k) >> 8) * 0x1p-24;
            const bool accept = a >= 0.0 || u < exp(a);
            if (accept) {
                rung[base + x] = k + 1;
                rung[base + y] = k;
            }
            accepted_out[base + x] = accepted_out[base + y] = accept ? 1 : 0;
            u_out[base + x] = u_out[base + y] = u;
        } else if (k < K && x >= 0) {
            accepted_out[base + x] = 0;
            u_out[base + x] = -1.0;
        }
    }
}

hipError_t launch_replica_swap(int* rung, const double* e_cur, const double* inv_t, const int* ladder_id, unsigned long long seed,
                               int round, unsigned char* accepted_out, double* u_out, int n_ladder, int K, hipStream_t st) {
    if (!rung || !e_cur || !inv_t || !ladder_id || !accepted_out || !u_out || n_ladder <= 0 || K < 1 || K > 64 || round < 0)
        return hipErrorInvalidValue;
    const size_t n_lane = (size_t)n_ladder * ((K + 1) / 2);
    const unsigned blocks = (unsigned)std::min<size_t>((n_lane + 255) / 256, 8192);
    hipLaunchKernelGGL(replica_swap_kernel, dim3(blocks), dim3(256), 0, st, rung, e_cur, inv_t, ladder_id, seed, round, accepted_out,
                       u_out, n_ladder, K);
    return hipGetLastError();
}

}  // namespace esmk
