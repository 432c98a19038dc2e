// search.hip — protein search on pooled embeddings (esm_amd/search.py).
//
// One vector per protein (the mean of its residue rows), a cosine top-k against the whole database, the aligner on the
// survivors.  The similarities are the existing dense GEMM over the f16x3 images of esmk_op_align_rows; the kernels here stand
// around it, one launch each, no global atomics, nothing that depends on the order lanes arrive in:
//     pool_rows_kernel    per (segment, column): the mean of the segment's listed rows, summed in fp64 in list order
//     topk_merge_kernel   per row of a block of similarities: the k best of the block and of a running list, in one read
#include "common.h"
#include "engine_internal.h"

#include <string>

using namespace esmk;
using namespace esmk_host;

namespace {

// ---- pooling ------------------------------------------------------------------------------------------------------------
// One thread per (segment, float4 of E).  Segment s owns rows[seg_off[s] .. seg_off[s + 1]) of the list, whose length is
// seg_off[n_seg]; offsets and row indices are device data, hence the clamps.  The sum runs in list order in fp64 and is
// divided and rounded once: a segment's vector depends on its own rows alone.
__global__ __launch_bounds__(256) void pool_rows_kernel(const float* __restrict__ x, int ldx, int N, const int* __restrict__ rows,
                                                        const int* __restrict__ seg_off, int n_seg, float* __restrict__ out, int E) {
    const int e4 = E >> 2;
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (size_t)n_seg * e4) return;
    const int s = (int)(id / e4), c = (int)(id - (size_t)s * e4) << 2;
    const int total = max(seg_off[n_seg], 0);
    const int lo = min(max(seg_off[s], 0), total), hi = min(max(seg_off[s + 1], lo), total);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int r = lo; r < hi; ++r) {
        const int row = min(max(rows ? rows[r] : r, 0), N - 1);
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + (size_t)row * ldx + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += (double)v[e];
    }
    f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
    if (hi > lo) {
        const double n = (double)(hi - lo);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (float)(acc[e] / n);
    }
    *reinterpret_cast<f32x4*>(out + (size_t)s * E + c) = o;
}

// ---- streaming top-k ----------------------------------------------------------------------------------------------------
// A candidate (value, id) is the 64-bit key [order(value) | ~id]: order() maps the IEEE bits to an unsigned integer that
// ascends with the total order (-inf < ... < -0.0 < +0.0 < ... < +inf), so "key descending" is "value descending, ties to the
// lower id", and keys are unique per id.  An unused slot (-inf, -1) is the key [order(-inf) | 0], below every real candidate
// (ids are >= 0, so ~id >= 2^31); it decodes to (-inf, -1) again.
constexpr int kTopkThreads = 1024;
constexpr int kTopkCap = 8192;              // candidate keys in LDS (64 KiB)
constexpr int kTopkLoads = 8;               // float4 loads a thread has in flight per round
constexpr int kTopkStep = 4 * kTopkThreads; // columns one load of the workgroup covers
constexpr int kTopkMaxK = 1024;
constexpr int kTopkMaxCols = 1 << 22;
static_assert(kTopkMaxK + kTopkStep <= kTopkCap, "a compacted list plus one step of columns must fit the candidate buffer");

ESMK_DEV unsigned int topk_order(float v) {
    const unsigned int b = __builtin_bit_cast(unsigned int, v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
ESMK_DEV float topk_value(unsigned int o) {
    return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
ESMK_DEV unsigned long long topk_key(float v, int id) {
    return ((unsigned long long)topk_order(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)id);
}
constexpr unsigned long long kTopkPad = (unsigned long long)0x007FFFFFu << 32;  // [order(-inf) | ~(-1)]

struct TopkArgs {
    const float* S;
    int ldS, n_cols, id_base;
    const int* exclude;  // [n_rows] or null
    int k;
    float* val;  // [n_rows, k] the running list, in and out
    int* id;
    int first;
};

// One workgroup per row, one read of the row.  Keys above the running threshold `thr` are appended to the candidate buffer
// (ballot and prefix count, one LDS counter update per wavefront); when the buffer could not hold another step of columns it
// is sorted, cut to the k best, and thr becomes the k-th key: from then on few columns pass.  The slot a key lands in depends
// on the order wavefronts arrive in, the sorted result does not (unique keys).  A round loads kTopkLoads float4 per thread
// before it looks at any; if its appends overflow the buffer they are dropped as a whole and the round is redone load by load
// with compactions in between (the first round, and rows that keep ascending).
__global__ __launch_bounds__(kTopkThreads) void topk_merge_kernel(const TopkArgs a) {
    __shared__ unsigned long long cand[kTopkCap];
    __shared__ unsigned int s_fill;
    const int tid = threadIdx.x, lane = tid & 63;
    const int row = blockIdx.x;
    const float* sr = a.S + (size_t)row * a.ldS;
    const int n4 = (a.n_cols + 3) >> 2;
    const int ex = a.exclude ? a.exclude[row] : -1;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    unsigned long long thr = kTopkPad;  // only keys above it are candidates
    float thr_val = topk_value((unsigned int)(kTopkPad >> 32));  // its value: -inf until k candidates stand
    unsigned int fill = 0;              // the keys in cand: the same in every thread

    auto append = [&](bool ok, unsigned long long key) {
        const unsigned long long m = __ballot(ok);
        if (m == 0) return;  // wave uniform
        unsigned int base = 0;
        if (lane == 0) base = atomicAdd(&s_fill, (unsigned)__popcll(m));
        base = __shfl(base, 0, 64);
        const unsigned int p = base + (unsigned)__popcll(m & below);
        if (ok && p < (unsigned)kTopkCap) cand[p] = key;
    };
    // the four columns of float4 group g (a group behind the row's end is passed as NaNs: no candidates)
    auto append4 = [&](const f32x4& v, int g) {
        // Once a threshold stands, nearly every group ends here: a value below the threshold's value is no candidate (the
        // float comparison is false for NaN, true for a tie and for -0.0 against +0.0, which the keys below decide)
        const bool maybe = (v[0] >= thr_val) | (v[1] >= thr_val) | (v[2] >= thr_val) | (v[3] >= thr_val);
        if (__ballot(maybe) == 0) return;  // wave uniform
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int col = 4 * g + e;
            const int id = a.id_base + col;
            const unsigned long long key = topk_key(v[e], id);
            append(col < a.n_cols && v[e] == v[e] && id != ex && key > thr, key);
        }
    };
    // bitonic sort, descending, of the `fill` keys padded with unused slots to a power of two; then the k best stay.
    // Called by every thread, after a barrier behind the last append.
    auto compact = [&]() {
        unsigned int P = 2;
        while (P < fill) P <<= 1;
        for (unsigned int i = fill + tid; i < P; i += kTopkThreads) cand[i] = kTopkPad;
        for (unsigned int size = 2; size <= P; size <<= 1) {
            for (unsigned int stride = size >> 1; stride > 0; stride >>= 1) {
                __syncthreads();
                for (unsigned int t = tid; t < (P >> 1); t += kTopkThreads) {
                    const unsigned int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                    const unsigned long long x = cand[lo], y = cand[hi];
                    const bool desc = (lo & size) == 0;
                    if ((x < y) == desc) {
                        cand[lo] = y;
                        cand[hi] = x;
                    }
                }
            }
        }
        __syncthreads();
        if (fill >= (unsigned)a.k) {
            fill = (unsigned)a.k;
            thr = cand[a.k - 1];
            thr_val = topk_value((unsigned int)(thr >> 32));
        }
        __syncthreads();  // (thr has been read before a later append overwrites the slot)
        if (tid == 0) s_fill = fill;
        __syncthreads();
    };

    if (tid == 0) s_fill = 0;
    __syncthreads();
    if (!a.first) {  // the used slots of the running list
        float v = 0.f;
        int id = -1;
        if (tid < a.k) {
            v = a.val[(size_t)row * a.k + tid];
            id = a.id[(size_t)row * a.k + tid];
        }
        append(id >= 0 && v == v, topk_key(v, id));
        __syncthreads();
        fill = min(s_fill, (unsigned)kTopkCap);
        __syncthreads();
    }

    const float nan = __builtin_nanf("");
    for (int g0 = 0; g0 < n4; g0 += kTopkThreads * kTopkLoads) {  // uniform trip count
        f32x4 v[kTopkLoads];
#pragma unroll
        for (int u = 0; u < kTopkLoads; ++u) {
            const int g = g0 + u * kTopkThreads + tid;
            v[u] = g < n4 ? *reinterpret_cast<const f32x4*>(sr + 4 * (size_t)g) : f32x4{nan, nan, nan, nan};
        }
#pragma unroll
        for (int u = 0; u < kTopkLoads; ++u) append4(v[u], g0 + u * kTopkThreads + tid);
        __syncthreads();
        const unsigned int total = s_fill;
        __syncthreads();  // (everyone has read the counter before the next round adds to it)
        if (total <= (unsigned)kTopkCap) {
            fill = total;
            continue;
        }
        // overflow: the round's appends are dropped, and the round runs again one load at a time
        if (tid == 0) s_fill = fill;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kTopkLoads; ++u) {
            if (fill + (unsigned)kTopkStep > (unsigned)kTopkCap) compact();  // fill <= k afterwards: the step fits
            append4(v[u], g0 + u * kTopkThreads + tid);
            __syncthreads();
            fill = s_fill;
            __syncthreads();
        }
    }
    compact();
    for (int r = tid; r < a.k; r += kTopkThreads) {
        const unsigned long long key = (unsigned)r < fill ? cand[r] : kTopkPad;
        a.val[(size_t)row * a.k + r] = topk_value((unsigned int)(key >> 32));
        a.id[(size_t)row * a.k + r] = (int)(0xFFFFFFFFu - (unsigned int)key);
    }
}

bool misaligned(const void* p, size_t a) { return ((size_t)p & (a - 1)) != 0; }

}  // namespace

extern "C" {

int esmk_op_pool_rows(const float* x_dev, int ldx, int N, const int32_t* rows_dev, const int32_t* seg_off_dev, int n_seg,
                      float* out_dev, int E, void* stream) {
    const std::string w("esmk_op_pool_rows");
    if (!x_dev || !seg_off_dev || !out_dev) return fail(w + ": null argument");
    if (E <= 0 || E % 4 != 0) return fail(w + ": E must be a positive multiple of 4");
    if (N <= 0 || N > ESMK_MAX_ROWS) return fail(w + ": need 0 < N <= 2^24");
    if (n_seg < 0 || n_seg > ESMK_MAX_ROWS) return fail(w + ": need 0 <= n_seg <= 2^24");
    if (ldx < E || ldx % 4 != 0) return fail(w + ": ldx must be a multiple of 4 that is >= E");
    if (misaligned(x_dev, 16) || misaligned(out_dev, 16)) return fail(w + ": x and out must be 16-byte aligned");
    const size_t total = (size_t)n_seg * (E / 4);
    if ((total + 255) / 256 > 0x7fffffffULL) return fail(w + ": n_seg * E exceeds the grid");
    if (n_seg == 0) return 0;
    hipLaunchKernelGGL(pool_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x_dev, ldx, N,
                       rows_dev, seg_off_dev, n_seg, out_dev, E);
    ESMK_TRY(hipGetLastError());
    return 0;
}

int esmk_op_topk_merge(const float* S_dev, int ldS, int n_rows, int n_cols, int id_base, const int32_t* exclude_dev, int k,
                       float* val_dev, int32_t* id_dev, int first, void* stream) {
    const std::string w("esmk_op_topk_merge");
    if (!S_dev || !val_dev || !id_dev) return fail(w + ": null argument");
    if (k < 1 || k > kTopkMaxK) return fail(w + ": k must be 1 .. 1024");
    if (n_cols < 1 || n_cols > kTopkMaxCols) return fail(w + ": n_cols must be 1 .. 2^22");
    if (n_rows < 0 || n_rows > ESMK_MAX_ROWS) return fail(w + ": need 0 <= n_rows <= 2^24");
    if (ldS < n_cols || ldS % 4 != 0) return fail(w + ": ldS must be a multiple of 4 that is >= n_cols");
    if (id_base < 0 || (long long)id_base + n_cols > 0x7fffffffLL) return fail(w + ": need 0 <= id_base and id_base + n_cols <= 2^31 - 1");
    if (misaligned(S_dev, 16) || misaligned(val_dev, 4) || misaligned(id_dev, 4) || misaligned(exclude_dev, 4))
        return fail(w + ": S must be 16-byte aligned, the lists and exclude 4-byte aligned");
    if (n_rows == 0) return 0;
    TopkArgs a;
    a.S = S_dev, a.ldS = ldS, a.n_cols = n_cols, a.id_base = id_base, a.exclude = exclude_dev, a.k = k;
    a.val = val_dev, a.id = id_dev, a.first = first ? 1 : 0;
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)n_rows), dim3(kTopkThreads), 0, (hipStream_t)stream, a);
    ESMK_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
