// philox.h — the counter-addressed random number generator of the sampling kernels (sampling.hip) and of the MSA row race
// (msa_select.hip).  A number is addressed by (seed, counter word 0, counter word 1, purpose, index) and depends on nothing
// else: not on a thread or block index, the batch or the launch geometry.
#pragma once
#include <hip/hip_runtime.h>

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

// counter word 2: 0 and 1 belong to the sampler (sampling.hip), 2 to the row race of an MSA subsample (msa_select.hip: counter
// (subsample, 0, 2, row)); a design chain (design.hip) draws its proposal at (chain, step, 2, 0) and its acceptance at (chain,
// step, 3, 0) — a chain and a subsample are never keyed by the same seed in one computation; a ladder of replicas
// (tempering.hip) draws the swap of its rungs k and k + 1 in swap round r at (ladder id, r, 4, k)
constexpr unsigned kPurposePermutation = 0, kPurposeToken = 1, kPurposeRace = 2;
constexpr unsigned kPurposeProposal = 2, kPurposeAcceptance = 3, kPurposeSwap = 4;

// First output word of the generator at counter (chain, epoch_or_step, purpose, index) under key (seed lo, seed hi).
__device__ inline unsigned philox_word0(unsigned long long seed, int chain, int epoch_or_step, unsigned purpose, int index) {
    return philox4x32_10((unsigned)chain, (unsigned)epoch_or_step, purpose, (unsigned)index, (unsigned)seed,
                         (unsigned)(seed >> 32)).x;
}

}  // namespace esmk
