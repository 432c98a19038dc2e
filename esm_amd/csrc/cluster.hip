// cluster.hip — range search and greedy incremental clustering on pooled embeddings (esm_amd/cluster.py).
//
// The similarities are the dense GEMM of the search (f16x3 images of esmk_op_align_rows), block of database rows by block; the
// kernels here stand behind it and on the graph it leaves:
//     range_rows_kernel       per row of a block of similarities: count, or write in ascending column order, the columns >= tau
//     cluster_mark_kernel     per out-list: an undecided node blocks, a new representative covers, its later-ranked neighbours
//     cluster_decide_kernel   per node: covered -> member, neither blocked nor covered -> representative
//     cluster_assign_kernel   per out-list of a representative: an integer atomic max of [order(score) | ~rank] per member
// No float atomics, no scratch memory; every store that two threads may make to one word stores the same value, and the
// integer maximum does not depend on the order of its operands: every result is the same bits run after run.
#include "common.h"
#include "engine_internal.h"

#include <string>

using namespace esmk;
using namespace esmk_host;

namespace {

// ---- range search -------------------------------------------------------------------------------------------------------
constexpr int kRangeThreads = 256;
constexpr int kRangeWaves = kRangeThreads / 64;
constexpr int kRangeLoads = 8;  // float4 loads a thread has in flight per round: a round covers 8192 columns
constexpr int kRangeMaxCols = 1 << 22;

struct RangeArgs {
    const float* S;
    int ldS, n_cols, id_base;
    const int* exclude;  // [n_rows] or null
    float thr;
    long long* counts;         // count pass: [n_rows], added to
    const long long* offsets;  // fill pass: [n_rows + 1]
    long long* cursor;         // fill pass: [n_rows], where the row's next pair goes; advanced
    int* ids;                  // [cap]
    float* scores;             // [cap]
    long long cap;
};

// One workgroup per row, one read of the row, kRangeLoads float4 per thread in flight.  A column passes when S >= thr as a
// float comparison (false for NaN, true for a tie and for -0.0 against +0.0), lies before n_cols and is not the excluded id.
// Count pass: the row's passing columns are added to counts[row] (the workgroup is the word's only writer: a plain add).
// Fill pass: within a round the float4 groups ascend with (load, wavefront, lane), so a pair's slot is the row's cursor plus
// the passing columns of the groups before it: ballots and prefix counts inside a wavefront, one LDS word per (load,
// wavefront), an exclusive scan of those 32 words by the first wavefront.  The order of the output is the order of the
// columns, whatever order wavefronts arrive in.  A round in which nothing passes (nearly every one) costs a single barrier.
// offsets and cursor are device data: the row's range is clamped into [0, cap] and the cursor into the range, and no pair is
// written at or behind the range's end.
template <bool FILL>
__global__ __launch_bounds__(kRangeThreads) void range_rows_kernel(const RangeArgs a) {
    __shared__ unsigned int s_tot[kRangeLoads * kRangeWaves];
    __shared__ unsigned int s_sum;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x;
    const float* sr = a.S + (size_t)row * a.ldS;
    const int n4 = (a.n_cols + 3) >> 2;
    const int ex = a.exclude ? a.exclude[row] : -1;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    long long cur = 0, end = 0;
    if (FILL) {
        const long long lo = min(max(a.offsets[row], 0ll), a.cap);
        end = min(max(a.offsets[row + 1], lo), a.cap);
        cur = min(max(a.cursor[row], lo), end);
    }
    unsigned int mine = 0;  // count pass: this thread's passing columns

    const float nan = __builtin_nanf("");
    for (int g0 = 0; g0 < n4; g0 += kRangeThreads * kRangeLoads) {  // uniform trip count
        f32x4 v[kRangeLoads];
#pragma unroll
        for (int u = 0; u < kRangeLoads; ++u) {
            const int g = g0 + u * kRangeThreads + tid;
            v[u] = g < n4 ? *reinterpret_cast<const f32x4*>(sr + 4 * (size_t)g) : f32x4{nan, nan, nan, nan};
        }
        unsigned int bits = 0;  // bit 4 u + e: column e of load u passes
#pragma unroll
        for (int u = 0; u < kRangeLoads; ++u) {
            const int c0 = 4 * (g0 + u * kRangeThreads + tid);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool ok = c0 + e < a.n_cols && v[u][e] >= a.thr && a.id_base + c0 + e != ex;
                bits |= (ok ? 1u : 0u) << (4 * u + e);
            }
        }
        if (!FILL) {
            mine += (unsigned)__popc(bits);
            continue;
        }
        if (!__syncthreads_or(bits != 0)) continue;  // uniform
        unsigned int pre[kRangeLoads];  // the passing columns of this load in the lanes below
#pragma unroll
        for (int u = 0; u < kRangeLoads; ++u) {
            unsigned int p = 0, t = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned long long m = __ballot((bits >> (4 * u + e)) & 1u);
                p += (unsigned)__popcll(m & below);
                t += (unsigned)__popcll(m);
            }
            pre[u] = p;
            if (lane == 0) s_tot[u * kRangeWaves + wave] = t;
        }
        __syncthreads();
        if (wave == 0) {  // exclusive scan of the 32 (load, wavefront) totals, in that order
            const unsigned int x = lane < kRangeLoads * kRangeWaves ? s_tot[lane] : 0u;
            unsigned int incl = x;
#pragma unroll
            for (int d = 1; d < kRangeLoads * kRangeWaves; d <<= 1) {
                const unsigned int y = __shfl_up(incl, d, 64);
                if (lane >= d) incl += y;
            }
            if (lane < kRangeLoads * kRangeWaves) s_tot[lane] = incl - x;
            if (lane == kRangeLoads * kRangeWaves - 1) s_sum = incl;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kRangeLoads; ++u) {
            if (((bits >> (4 * u)) & 15u) == 0) continue;
            long long p = cur + s_tot[u * kRangeWaves + wave] + pre[u];
            const int c0 = 4 * (g0 + u * kRangeThreads + tid);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if ((bits >> (4 * u + e)) & 1u) {
                    if (p < end) {
                        a.ids[p] = a.id_base + c0 + e;
                        a.scores[p] = v[u][e];
                    }
                    ++p;
                }
            }
        }
        cur = min(cur + (long long)s_sum, end);
        // (the next round's barrier stands between these reads of s_tot / s_sum and its writes)
    }
    if (!FILL) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d, 64);
        if (lane == 0) s_tot[wave] = mine;
        __syncthreads();
        if (tid == 0) {
            unsigned int total = 0;
#pragma unroll
            for (int w = 0; w < kRangeWaves; ++w) total += s_tot[w];
            a.counts[row] += (long long)total;
        }
    } else if (tid == 0) {
        a.cursor[row] = cur;
    }
}

// ---- greedy incremental clustering ------------------------------------------------------------------------------------------
// A node is undecided, a representative that has not yet covered its out-list (new), a representative that has, or covered.
// A round is a mark launch and a decide launch.  Mark reads `state` and writes only `blocked` and `covered`; decide reads
// those and writes `state`: nothing a launch reads changes under it, so a round's outcome and the number of rounds are fixed.
//   mark    an undecided u sets blocked[w] = 1, a new representative u sets covered[w] = 1, for every w of out(u) with
//           rank(w) > rank(u): plain stores of the value 1.
//   decide  a new representative becomes an old one (it has covered); an undecided node with covered set becomes a member;
//           one that is neither covered nor blocked becomes a new representative; blocked is cleared.
// Why this is the sequential loop (walk the nodes by rank; an uncovered node becomes a representative and covers the undecided
// nodes of its out-list): a representative only ever covers later ranks, and an undecided earlier u with w in out(u) blocks
// w.  So when w is decided every earlier u with w in out(u) is decided already, and each of them that is a representative
// has covered w in the mark launch that followed its own decision (w could not be decided in the round that decided u: u
// was undecided when that round began, and blocked it).  By induction over rank, w becomes a member exactly when an earlier
// representative lists it and a representative otherwise.  The undecided node of the lowest rank is never blocked, so every
// round decides at least one node.
constexpr int kUndecided = 0, kRepNew = 1, kRep = 2, kCovered = 3;
constexpr int kClusterThreads = 256;

// `1 << lanes_log2` lanes walk one out-list, interleaved (consecutive lanes read consecutive ids).  offsets and ids are device
// data: a list's range is clamped into [0, nnz] and an id outside [0, n) is skipped.
__global__ __launch_bounds__(kClusterThreads) void cluster_mark_kernel(const long long* __restrict__ offsets, const int* __restrict__ ids,
                                                                       int n, long long nnz, const int* __restrict__ rank,
                                                                       const int* __restrict__ state, int* __restrict__ blocked,
                                                                       int* __restrict__ covered, int lanes_log2) {
    const size_t t = (size_t)blockIdx.x * kClusterThreads + threadIdx.x;
    const size_t u = t >> lanes_log2;
    const int lanes = 1 << lanes_log2, sub = (int)(t & (size_t)(lanes - 1));
    if (u >= (size_t)n) return;
    const int st = state[u];
    if (st != kUndecided && st != kRepNew) return;
    int* __restrict__ flag = st == kUndecided ? blocked : covered;
    const long long lo = min(max(offsets[u], 0ll), nnz), hi = min(max(offsets[u + 1], lo), nnz);
    const int ru = rank[u];
    for (long long i = lo + sub; i < hi; i += lanes) {
        const int w = ids[i];
        if ((unsigned)w < (unsigned)n && rank[w] > ru) flag[w] = 1;
    }
}

__global__ __launch_bounds__(kClusterThreads) void cluster_decide_kernel(int* __restrict__ state, int* __restrict__ blocked,
                                                                         const int* __restrict__ covered, int n,
                                                                         int* __restrict__ remaining) {
    const size_t u = (size_t)blockIdx.x * kClusterThreads + threadIdx.x;
    int left = 0;
    if (u < (size_t)n) {
        const int st = state[u];
        if (st == kRepNew) {
            state[u] = kRep;
        } else if (st == kUndecided) {
            if (covered[u]) state[u] = kCovered;
            else if (!blocked[u]) state[u] = kRepNew;
            else left = 1;
        }
        blocked[u] = 0;
    }
    const int c = __syncthreads_count(left);
    if (threadIdx.x == 0 && c > 0) atomicAdd(remaining, c);  // an integer sum: the same whatever the order
}

// (the map of search.hip's top-k: an unsigned integer that ascends with the total order of the IEEE bits)
ESMK_DEV unsigned int float_order(float v) {
    const unsigned int b = __builtin_bit_cast(unsigned int, v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// key[w] = max over the representatives u with w in out(u) and rank(u) < rank(w) of [o | ~rank(u)], o = order(S[u][w]) for
// "nearest" and 0 for "first": the largest score, ties to the lower rank / the lowest rank.  key starts at 0, which no
// candidate equals (~rank >= 2^31 for rank < 2^31).
__global__ __launch_bounds__(kClusterThreads) void cluster_assign_kernel(const long long* __restrict__ offsets, const int* __restrict__ ids,
                                                                         const float* __restrict__ scores, int n, long long nnz,
                                                                         const int* __restrict__ rank, const int* __restrict__ state,
                                                                         int nearest, unsigned long long* __restrict__ key,
                                                                         int lanes_log2) {
    const size_t t = (size_t)blockIdx.x * kClusterThreads + threadIdx.x;
    const size_t u = t >> lanes_log2;
    const int lanes = 1 << lanes_log2, sub = (int)(t & (size_t)(lanes - 1));
    if (u >= (size_t)n) return;
    const int st = state[u];
    if (st != kRepNew && st != kRep) return;
    const long long lo = min(max(offsets[u], 0ll), nnz), hi = min(max(offsets[u + 1], lo), nnz);
    const int ru = rank[u];
    const unsigned long long low = (unsigned long long)(0xFFFFFFFFu - (unsigned)ru);
    for (long long i = lo + sub; i < hi; i += lanes) {
        const int w = ids[i];
        if ((unsigned)w < (unsigned)n && rank[w] > ru)
            atomicMax(&key[w], ((unsigned long long)(nearest ? float_order(scores[i]) : 0u) << 32) | low);
    }
}

bool misaligned(const void* p, size_t a) { return ((size_t)p & (a - 1)) != 0; }

// the checks the three graph entries share; blocks of the launch in *blocks
int check_graph(const std::string& w, const void* offsets, const void* ids, int n, long long nnz, const void* rank, const void* state,
                int lanes, unsigned* blocks, int* lanes_log2) {
    if (!offsets || !rank || !state) return fail(w + ": null argument");
    if (n < 1 || n > ESMK_MAX_ROWS) return fail(w + ": need 1 <= n <= 2^24");
    if (nnz < 0) return fail(w + ": nnz must not be negative");
    if (nnz > 0 && !ids) return fail(w + ": null ids with nnz > 0");
    if (lanes < 1 || lanes > 64 || (lanes & (lanes - 1)) != 0) return fail(w + ": lanes must be a power of two, 1 .. 64");
    if (misaligned(offsets, 8) || misaligned(ids, 4) || misaligned(rank, 4) || misaligned(state, 4))
        return fail(w + ": offsets must be 8-byte aligned, ids, rank and state 4-byte aligned");
    int lg = 0;
    while ((1 << lg) < lanes) ++lg;
    *lanes_log2 = lg;
    *blocks = (unsigned)((((size_t)n << lg) + kClusterThreads - 1) / kClusterThreads);
    return 0;
}

}  // namespace

extern "C" {

int esmk_op_range_rows(const float* S_dev, int ldS, int n_rows, int n_cols, int id_base, const int32_t* exclude_dev, float threshold,
                       int fill, int64_t* counts_dev, const int64_t* offsets_dev, int64_t* cursor_dev, int32_t* ids_dev,
                       float* scores_dev, long long cap, void* stream) {
    const std::string w("esmk_op_range_rows");
    if (!S_dev) return fail(w + ": null argument");
    if (!fill && !counts_dev) return fail(w + ": null counts in the count pass");
    if (fill && (!offsets_dev || !cursor_dev || !ids_dev || !scores_dev)) return fail(w + ": null offsets, cursor, ids or scores in the fill pass");
    if (n_cols < 1 || n_cols > kRangeMaxCols) return fail(w + ": n_cols must be 1 .. 2^22");
    if (n_rows < 0 || n_rows > ESMK_MAX_ROWS) return fail(w + ": need 0 <= n_rows <= 2^24");
    if (ldS < n_cols || ldS % 4 != 0) return fail(w + ": ldS must be a multiple of 4 that is >= n_cols");
    if (id_base < 0 || (long long)id_base + n_cols > 0x7fffffffLL) return fail(w + ": need 0 <= id_base and id_base + n_cols <= 2^31 - 1");
    if (fill && cap < 0) return fail(w + ": cap must not be negative");
    if (misaligned(S_dev, 16) || misaligned(exclude_dev, 4) || misaligned(counts_dev, 8) || misaligned(offsets_dev, 8) ||
        misaligned(cursor_dev, 8) || misaligned(ids_dev, 4) || misaligned(scores_dev, 4))
        return fail(w + ": S must be 16-byte aligned, counts, offsets and cursor 8-byte aligned, exclude, ids and scores 4-byte aligned");
    if (n_rows == 0) return 0;
    RangeArgs a;
    a.S = S_dev, a.ldS = ldS, a.n_cols = n_cols, a.id_base = id_base, a.exclude = exclude_dev, a.thr = threshold;
    a.counts = (long long*)counts_dev, a.offsets = (const long long*)offsets_dev, a.cursor = (long long*)cursor_dev;
    a.ids = ids_dev, a.scores = scores_dev, a.cap = cap;
    if (fill)
        hipLaunchKernelGGL(range_rows_kernel<true>, dim3((unsigned)n_rows), dim3(kRangeThreads), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(range_rows_kernel<false>, dim3((unsigned)n_rows), dim3(kRangeThreads), 0, (hipStream_t)stream, a);
    ESMK_TRY(hipGetLastError());
    return 0;
}

int esmk_op_cluster_mark(const int64_t* offsets_dev, const int32_t* ids_dev, int n, long long nnz, const int32_t* rank_dev,
                         const int32_t* state_dev, int32_t* blocked_dev, int32_t* covered_dev, int lanes, void* stream) {
    const std::string w("esmk_op_cluster_mark");
    unsigned blocks = 0;
    int lg = 0;
    if (int rc = check_graph(w, offsets_dev, ids_dev, n, nnz, rank_dev, state_dev, lanes, &blocks, &lg)) return rc;
    if (!blocked_dev || !covered_dev) return fail(w + ": null argument");
    if (misaligned(blocked_dev, 4) || misaligned(covered_dev, 4)) return fail(w + ": blocked and covered must be 4-byte aligned");
    hipLaunchKernelGGL(cluster_mark_kernel, dim3(blocks), dim3(kClusterThreads), 0, (hipStream_t)stream, (const long long*)offsets_dev,
                       ids_dev, n, nnz, rank_dev, state_dev, blocked_dev, covered_dev, lg);
    ESMK_TRY(hipGetLastError());
    return 0;
}

int esmk_op_cluster_decide(int32_t* state_dev, int32_t* blocked_dev, const int32_t* covered_dev, int n, int32_t* remaining_dev,
                           void* stream) {
    const std::string w("esmk_op_cluster_decide");
    if (!state_dev || !blocked_dev || !covered_dev || !remaining_dev) return fail(w + ": null argument");
    if (n < 1 || n > ESMK_MAX_ROWS) return fail(w + ": need 1 <= n <= 2^24");
    if (misaligned(state_dev, 4) || misaligned(blocked_dev, 4) || misaligned(covered_dev, 4) || misaligned(remaining_dev, 4))
        return fail(w + ": state, blocked, covered and remaining must be 4-byte aligned");
    hipLaunchKernelGGL(cluster_decide_kernel, dim3((unsigned)((n + kClusterThreads - 1) / kClusterThreads)), dim3(kClusterThreads), 0,
                       (hipStream_t)stream, state_dev, blocked_dev, covered_dev, n, remaining_dev);
    ESMK_TRY(hipGetLastError());
    return 0;
}

int esmk_op_cluster_assign(const int64_t* offsets_dev, const int32_t* ids_dev, const float* scores_dev, int n, long long nnz,
                           const int32_t* rank_dev, const int32_t* state_dev, int nearest, uint64_t* key_dev, int lanes, void* stream) {
    const std::string w("esmk_op_cluster_assign");
    unsigned blocks = 0;
    int lg = 0;
    if (int rc = check_graph(w, offsets_dev, ids_dev, n, nnz, rank_dev, state_dev, lanes, &blocks, &lg)) return rc;
    if (!key_dev) return fail(w + ": null argument");
    if (nearest && nnz > 0 && !scores_dev) return fail(w + ": null scores with nearest");
    if (misaligned(key_dev, 8) || misaligned(scores_dev, 4)) return fail(w + ": key must be 8-byte aligned, scores 4-byte aligned");
    hipLaunchKernelGGL(cluster_assign_kernel, dim3(blocks), dim3(kClusterThreads), 0, (hipStream_t)stream, (const long long*)offsets_dev,
                       ids_dev, scores_dev, n, nnz, rank_dev, state_dev, nearest ? 1 : 0, (unsigned long long*)key_dev, lg);
    ESMK_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
