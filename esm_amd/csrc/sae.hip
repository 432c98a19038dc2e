// sae.hip — reading the residual stream in the basis of a sparse autoencoder (esm_amd/sae.py).
//
// For a captured representation row x (fp32 [E]):  u = sub(mul(input_scale, x), b_dec);  z[f] = <w_enc[f], u> + b_enc[f];
// feature f is ACTIVE iff z[f] > threshold[f] (thresholds >= 0: a NaN is never active, +inf is).  The product is the existing
// dense GEMM over the f16x3 operand images (hi | hi | lo rows against hi | lo | hi weights, fp32 store epilogue); the kernels
// here are what stands around it, one launch each, no global atomics, nothing that depends on the order lanes arrive in:
//     image_rows_kernel       (elementwise.hip) gather the scored rows, form u, write the hi | hi | lo image the GEMM reads
//     sae_topk_kernel         per row: count the actives and select the k best, value descending, ties to the lower index
//     sae_segment_max_kernel  per (sequence, feature): the largest activation over the sequence's rows and where it was
//     sae_decode_kernel       x^ = inv_scale (b_dec + sum_r values[r] w_dec[indices[r]]), one rounded product and add per term
#include "common.h"
#include "engine_internal.h"

#include <cmath>
#include <string>

using namespace esmk;
using namespace esmk_host;

namespace {

// The candidates of a row that the selection sorts in LDS.  A row with more actives goes through the radix select first.
constexpr int kSaeCand = 1024;
constexpr int kSaeMaxK = 256;
constexpr int kSaeMaxF = 65536;

// An active value is a positive float (thresholds are >= 0), so its bits order as an unsigned integer; with the complement of
// the index below them the key is unique per feature and "key descending" is "value descending, ties to the lower index".
ESMK_DEV unsigned long long sae_key(float v, int f) {
    return ((unsigned long long)__builtin_bit_cast(unsigned int, v) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)f);
}

// ---- top-k --------------------------------------------------------------------------------------------------------------
struct SaeTopkArgs {
    const float* z;
    int ldz;
    const float* thr;  // [F] or null: thr0 for every feature
    float thr0;
    int F, k, k_sae;  // k_sae > 0: a top-k autoencoder that keeps k_sae features of a row (k <= k_sae)
    int* idx;
    float* val;
    int* n_active;
    unsigned long long* cutoff;  // [n] or null: the key of the k_sae-th feature where a row has more actives, else 0
    int* path;                   // [n] or null: 0 = the LDS path, d > 0 = the radix select ran d digit passes
};

// One workgroup per row.  The row is walked in float4 groups, group g by thread g % 256 in round g / 256: 16-byte loads,
// coalesced over the wavefront.  Actives are compacted by ballot and prefix count, one LDS counter update per wavefront and
// component; the slot a key lands in depends on the order wavefronts arrive in, the sorted result does not (unique keys).
__global__ __launch_bounds__(256) void sae_topk_kernel(const SaeTopkArgs a) {
    __shared__ unsigned long long cand[kSaeCand];
    __shared__ unsigned int hist[256];
    __shared__ unsigned int s_fill, s_bucket, s_above;
    const int tid = threadIdx.x, lane = tid & 63;
    const int row = blockIdx.x;
    const float* zr = a.z + (size_t)row * a.ldz;
    const int F4 = a.F >> 2, rounds = (F4 + 255) >> 8;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));

    // every active key >= low goes into cand while there is room; s_fill counts them all
    auto compact = [&](unsigned long long low) {
        for (int it = 0; it < rounds; ++it) {  // uniform trip count: every lane takes part in the ballots
            const int g = it * 256 + tid;
            const bool in = g < F4;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f}, t = f32x4{a.thr0, a.thr0, a.thr0, a.thr0};
            if (in) {
                v = *reinterpret_cast<const f32x4*>(zr + 4 * g);
                if (a.thr) t = *reinterpret_cast<const f32x4*>(a.thr + 4 * g);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned long long key = sae_key(v[e], 4 * g + e);
                const bool act = in && v[e] > t[e] && key >= low;
                const unsigned long long m = __ballot(act);
                if (m == 0) continue;  // wave uniform
                unsigned int base = 0;
                if (lane == 0) base = atomicAdd(&s_fill, (unsigned)__popcll(m));
                base = __shfl(base, 0, 64);
                const unsigned int p = base + (unsigned)__popcll(m & below);
                if (act && p < (unsigned)kSaeCand) cand[p] = key;
            }
        }
    };

    if (tid == 0) s_fill = 0;
    __syncthreads();
    compact(0ull);
    __syncthreads();
    const unsigned int count = s_fill;  // the row's actives
    const int ksel = a.k_sae > 0 ? a.k_sae : a.k;
    unsigned int nc = count;
    int passes = 0;
    if (count > (unsigned)kSaeCand) {
        // radix select over the row in global memory: 8-bit digits of the key from the high one down; after digit d the
        // keys that share `prefix` above d hold the ksel-th key at place `remaining`.  It stops as soon as the keys at or
        // above the prefix fit the candidate buffer (after the last digit they are exactly ksel).
        unsigned long long prefix = 0;
        unsigned int remaining = (unsigned)ksel, above = 0;
        for (int d = 7; d >= 0; --d) {
            const int shift = 8 * d;
            hist[tid] = 0;
            __syncthreads();
            for (int it = 0; it < rounds; ++it) {
                const int g = it * 256 + tid;
                if (g >= F4) break;
                const f32x4 v = *reinterpret_cast<const f32x4*>(zr + 4 * g);
                const f32x4 t = a.thr ? *reinterpret_cast<const f32x4*>(a.thr + 4 * g) : f32x4{a.thr0, a.thr0, a.thr0, a.thr0};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (!(v[e] > t[e])) continue;
                    const unsigned long long key = sae_key(v[e], 4 * g + e);
                    const bool same = d == 7 || (key >> (shift + 8)) == (prefix >> (shift + 8));
                    if (same) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
                }
            }
            __syncthreads();
            if (tid == 0) {
                unsigned int acc = 0;
                int b = 255;
                for (; b > 0; --b) {
                    if (acc + hist[b] >= remaining) break;
                    acc += hist[b];
                }
                s_bucket = (unsigned)b;
                s_above = acc;
            }
            __syncthreads();
            const unsigned int b = s_bucket, acc = s_above, inb = hist[b];
            prefix |= (unsigned long long)b << shift;
            above += acc;
            remaining -= acc;
            ++passes;
            __syncthreads();  // hist and the two scalars have been read
            if (above + inb <= (unsigned)kSaeCand) break;
        }
        if (tid == 0) s_fill = 0;
        __syncthreads();
        compact(prefix);
        __syncthreads();
        nc = min(s_fill, (unsigned)kSaeCand);
    }
    // bitonic sort, descending, of the nc candidates padded with zero keys (below every active key) to a power of two
    unsigned int P = 2;
    while (P < nc) P <<= 1;
    for (unsigned int i = nc + tid; i < P; i += 256) cand[i] = 0ull;
    for (unsigned int size = 2; size <= P; size <<= 1) {
        for (unsigned int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (unsigned int t = tid; t < (P >> 1); t += 256) {
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
    const unsigned int kept = min(nc, (unsigned)ksel);
    for (int r = tid; r < a.k; r += 256) {
        const bool have = (unsigned)r < kept;
        const unsigned long long key = have ? cand[r] : 0ull;
        a.idx[(size_t)row * a.k + r] = have ? (int)(0xFFFFFFFFu - (unsigned)key) : -1;
        a.val[(size_t)row * a.k + r] = have ? __builtin_bit_cast(float, (unsigned int)(key >> 32)) : 0.f;
    }
    if (tid == 0) {
        a.n_active[row] = (int)(a.k_sae > 0 ? min(count, (unsigned)a.k_sae) : count);
        if (a.cutoff) a.cutoff[row] = (a.k_sae > 0 && count > (unsigned)a.k_sae) ? cand[a.k_sae - 1] : 0ull;
        if (a.path) a.path[row] = passes;
    }
}

// ---- per-sequence maximum -----------------------------------------------------------------------------------------------
// One thread per (sequence, feature); the chunk holds rows [row0, row0 + n) of the call's row list, sequence b owns the rows
// [seg_start[b], seg_start[b + 1]) of that list (device data, hence the clamps).  Rows are walked in ascending position and a
// row replaces the stored value only if it is strictly greater: the lowest position wins ties, and a sequence split between
// two chunks (launches in order on one stream) merges to what one launch gives.
__global__ __launch_bounds__(256) void sae_segment_max_kernel(const float* __restrict__ z, int ldz, const float* __restrict__ thr,
                                                              float thr0, const unsigned long long* __restrict__ cutoff,
                                                              const int* __restrict__ rows, const int* __restrict__ seg_start,
                                                              int row0, int n, int F, int nfb, float* __restrict__ pmax,
                                                              int* __restrict__ parg) {
    const int b = blockIdx.x / nfb;
    const int f = (blockIdx.x - b * nfb) * 256 + threadIdx.x;
    if (f >= F) return;
    const int lo = min(max(seg_start[b] - row0, 0), n), hi = min(max(seg_start[b + 1] - row0, 0), n);
    if (lo >= hi) return;
    const float t = thr ? thr[f] : thr0;
    const size_t o = (size_t)b * F + f;
    float cur = pmax[o];
    int arg = parg[o];
    for (int r = lo; r < hi; ++r) {
        const float v = z[(size_t)r * ldz + f];
        bool act = v > t;
        if (cutoff) {
            const unsigned long long c = cutoff[r];
            act = act && (c == 0ull || sae_key(v, f) >= c);
        }
        if (act && v > cur) {
            cur = v;
            arg = rows[2 * r + 1];
        }
    }
    pmax[o] = cur;
    parg[o] = arg;
}

// ---- decode -------------------------------------------------------------------------------------------------------------
// One thread per (row, float4 of E); the sum runs rank by rank from r = 0; indices outside [0, F) (-1: an unused slot) are skipped
__global__ __launch_bounds__(256) void sae_decode_kernel(const int* __restrict__ idx, const float* __restrict__ val, int k,
                                                         const float* __restrict__ w_dec, const float* __restrict__ b_dec,
                                                         float inv_scale, float* __restrict__ out, int n, int E, int F) {
    const int e4 = E >> 2;
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (size_t)n * e4) return;
    const int row = (int)(id / e4), c = (int)(id - (size_t)row * e4) << 2;
    f32x4 acc = b_dec ? *reinterpret_cast<const f32x4*>(b_dec + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < k; ++r) {
        const int f = idx[(size_t)row * k + r];
        if (f < 0 || f >= F) continue;
        const float v = val[(size_t)row * k + r];
        const f32x4 w = *reinterpret_cast<const f32x4*>(w_dec + (size_t)f * E + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = add_rn(acc[e], mul_rn(v, w[e]));
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = mul_rn(inv_scale, acc[e]);
    *reinterpret_cast<f32x4*>(out + (size_t)row * E + c) = acc;
}

bool misaligned(const void* p, size_t a) { return ((size_t)p & (a - 1)) != 0; }

}  // namespace

extern "C" {

int esmk_op_sae_cand(void) { return kSaeCand; }

int esmk_op_sae_rows(const float* x_dev, int ldx, int N, const int32_t* rows_dev, int n, const float* b_dec_dev, float input_scale,
                     void* image_dev, int ld_image, int E, void* stream) {
    const std::string w("esmk_op_sae_rows");
    if (!x_dev || !image_dev) return fail(w + ": null argument");
    if (E <= 0 || E % 4 != 0) return fail(w + ": E must be a positive multiple of 4");
    if (N <= 0 || N > ESMK_MAX_ROWS || n < 0 || n > ESMK_MAX_ROWS) return fail(w + ": need 0 < N <= 2^24 and 0 <= n <= 2^24");
    if (!rows_dev && n > N) return fail(w + ": without a row list the first n rows are taken, n must not exceed N");
    if (ldx < E || ldx % 4 != 0) return fail(w + ": ldx must be a multiple of 4 that is >= E");
    const int Ep = (E + 63) / 64 * 64;
    if (ld_image < 3 * Ep || ld_image % 4 != 0) return fail(w + ": ld_image must be a multiple of 4 that is >= 3 * (E rounded up to 64)");
    if (misaligned(x_dev, 16) || misaligned(b_dec_dev, 16) || misaligned(image_dev, 8)) return fail(w + ": x and b_dec must be 16-byte aligned, the image 8-byte aligned");
    if (!(input_scale == input_scale) || std::isinf(input_scale)) return fail(w + ": input_scale must be finite");
    if (n == 0) return 0;
    ESMK_TRY(launch_image_rows(x_dev, ldx, N, rows_dev, n, b_dec_dev, input_scale, /*cosine=*/0, /*b_side=*/0, /*zero_negative=*/0,
                               image_dev, ld_image, E, (hipStream_t)stream));
    return 0;
}

int esmk_op_sae_topk(const float* z_dev, int ldz, const float* threshold_dev, float threshold, int n, int F, int k, int k_sae,
                     int32_t* indices_dev, float* values_dev, int32_t* n_active_dev, uint64_t* cutoff_dev, int32_t* path_dev,
                     void* stream) {
    const std::string w("esmk_op_sae_topk");
    if (!z_dev || !indices_dev || !values_dev || !n_active_dev) return fail(w + ": null argument");
    if (F <= 0 || F > kSaeMaxF || F % 4 != 0) return fail(w + ": F must be a multiple of 4 in 4 .. 65536");
    if (k < 1 || k > kSaeMaxK) return fail(w + ": k must be 1 .. 256");
    if (k_sae < 0 || k_sae > kSaeMaxK || (k_sae > 0 && k > k_sae)) return fail(w + ": k_sae must be 0 (no limit) or k .. 256");
    if (n < 0 || n > ESMK_MAX_ROWS) return fail(w + ": need 0 <= n <= 2^24");
    if (ldz < F || ldz % 4 != 0) return fail(w + ": ldz must be a multiple of 4 that is >= F");
    if (misaligned(z_dev, 16) || misaligned(threshold_dev, 16) || misaligned(cutoff_dev, 8)) return fail(w + ": z and threshold must be 16-byte aligned, cutoff 8-byte aligned");
    if (!threshold_dev && !(threshold >= 0.f)) return fail(w + ": the threshold must not be negative or NaN");
    if (n == 0) return 0;
    SaeTopkArgs a;
    a.z = z_dev, a.ldz = ldz, a.thr = threshold_dev, a.thr0 = threshold, a.F = F, a.k = k, a.k_sae = k_sae;
    a.idx = indices_dev, a.val = values_dev, a.n_active = n_active_dev, a.cutoff = (unsigned long long*)cutoff_dev, a.path = path_dev;
    hipLaunchKernelGGL(sae_topk_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, a);
    ESMK_TRY(hipGetLastError());
    return 0;
}

int esmk_op_sae_segment_max(const float* z_dev, int ldz, const float* threshold_dev, float threshold, const uint64_t* cutoff_dev,
                            const int32_t* rows_dev, const int32_t* seg_start_dev, int row0, int n, int F, int B,
                            float* protein_max_dev, int32_t* protein_argmax_dev, void* stream) {
    const std::string w("esmk_op_sae_segment_max");
    if (!z_dev || !rows_dev || !seg_start_dev || !protein_max_dev || !protein_argmax_dev) return fail(w + ": null argument");
    if (F <= 0 || F > kSaeMaxF) return fail(w + ": F must be 1 .. 65536");
    if (B <= 0 || B > ESMK_MAX_ROWS) return fail(w + ": need 0 < B <= 2^24");
    if (n < 0 || n > ESMK_MAX_ROWS || row0 < 0 || row0 > ESMK_MAX_ROWS) return fail(w + ": need 0 <= n, row0 <= 2^24");
    if (ldz < F) return fail(w + ": ldz must be >= F");
    if (misaligned(cutoff_dev, 8)) return fail(w + ": cutoff must be 8-byte aligned");
    if (!threshold_dev && !(threshold >= 0.f)) return fail(w + ": the threshold must not be negative or NaN");
    const int nfb = (F + 255) / 256;
    if ((long long)nfb * B > 0x7fffffffLL) return fail(w + ": B * ceil(F / 256) exceeds the grid");
    if (n == 0) return 0;
    hipLaunchKernelGGL(sae_segment_max_kernel, dim3((unsigned)(nfb * B)), dim3(256), 0, (hipStream_t)stream, z_dev, ldz, threshold_dev,
                       threshold, (const unsigned long long*)cutoff_dev, rows_dev, seg_start_dev, row0, n, F, nfb, protein_max_dev,
                       protein_argmax_dev);
    ESMK_TRY(hipGetLastError());
    return 0;
}

int esmk_op_sae_decode(const int32_t* indices_dev, const float* values_dev, int n, int k, const float* w_dec_dev,
                       const float* b_dec_dev, float inv_scale, float* out_dev, int E, int F, void* stream) {
    const std::string w("esmk_op_sae_decode");
    if (!indices_dev || !values_dev || !w_dec_dev || !out_dev) return fail(w + ": null argument");
    if (E <= 0 || E % 4 != 0) return fail(w + ": E must be a positive multiple of 4");
    if (F <= 0 || F > kSaeMaxF) return fail(w + ": F must be 1 .. 65536");
    if (k < 1 || k > kSaeMaxK) return fail(w + ": k must be 1 .. 256");
    if (n < 0 || n > ESMK_MAX_ROWS) return fail(w + ": need 0 <= n <= 2^24");
    if (misaligned(w_dec_dev, 16) || misaligned(b_dec_dev, 16) || misaligned(out_dev, 16)) return fail(w + ": w_dec, b_dec and out must be 16-byte aligned");
    if (((size_t)n * (E / 4) + 255) / 256 > 0x7fffffffULL) return fail(w + ": n * E exceeds the grid");
    if (n == 0) return 0;
    const size_t total = (size_t)n * (E / 4);
    hipLaunchKernelGGL(sae_decode_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, indices_dev,
                       values_dev, k, w_dec_dev, b_dec_dev, inv_scale, out_dev, n, E, F);
    ESMK_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
