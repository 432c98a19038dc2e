// jacobian.hip — the categorical Jacobian of a masked language model (esm_amd/jacobian.py): every candidate residue put at
// every position of ONE protein, the change of the logits at every other position recorded as J[i, a, j, b] fp32
// [L, nA, L, nA] (400 L^2 floats for the 20 standard residues: 1.7 GB at L = 1022).  copy_rows_kernel (scoring.hip) builds the substituted
// copies; the kernels here scatter the logit differences of a chunk of copies into J, centre J along its four axes IN PLACE (one tensor, never
// two), reduce it to the [L, L] coupling map and correct that by its average product.  The layer stack between the first two
// is the time; these are bandwidth kernels.  No atomics anywhere: every sum runs in a fixed order in fp64, so no result
// depends on the launch geometry or on how the copies were chunked.  All indices into J are 64 bit.
#include "engine_internal.h"

#include <algorithm>
#include <stdint.h>

namespace esmk {

// out[c, j, b] = logits[c * L + j, cols[b]] - wt[j, cols[b]]: the fp32 difference of two fp32 logits, copy c of the chunk against
// the wild type.  out is the slice of J that starts at the chunk's first copy; one element per lane, the stores contiguous.
// Columns are device data, clamped to [0, V).
__global__ __launch_bounds__(256) void jacobian_scatter_kernel(const float* __restrict__ logits, const float* __restrict__ wt,
                                                               const int* __restrict__ cols, float* __restrict__ out,
                                                               size_t total, int L, int nA, int V) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const size_t r = e / nA;  // row c * L + j of the chunk's logits
        const int b = (int)(e - r * nA), j = (int)(r % L);
        const int col = min(max(cols[b], 0), V - 1);
        out[e] = logits[r * V + col] - wt[(size_t)j * V + col];
    }
}

hipError_t launch_jacobian_scatter(const float* logits, const float* wt, const int* cols, float* out, int n_copies, int L, int nA,
                                   int V, hipStream_t st) {
    if (!logits || !wt || !cols || !out || n_copies <= 0 || L <= 0 || nA <= 0 || V <= 0) return hipErrorInvalidValue;
    const size_t total = (size_t)n_copies * L * nA;
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(jacobian_scatter_kernel, dim3(blocks), dim3(256), 0, st, logits, wt, cols, out, total, L, nA, V);
    return hipGetLastError();
}

// ---- centring: x -= mean along one axis, four passes (b, j, a, i) -----------------------------------------------------------
// Every pass: the mean is the fp64 sum of the fp32 values in ascending index order, divided by n; every element becomes
// (float)((double)x - mean).  One lane owns one whole line of the axis, so the order of the additions is fixed.

// The contiguous axis b: a line is n <= 32 adjacent floats, held in registers between the sum and the store (one read, one
// write of J).  VEC4: n % 4 == 0 and J 16-byte aligned, so every line starts on a 16-byte boundary.
template <bool VEC4>
__global__ __launch_bounds__(256) void center_rows_kernel(float* __restrict__ J, size_t rows, int n) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += stride) {
        float* p = J + r * n;
        float v[32];
        if (VEC4) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (4 * q < n) x = *reinterpret_cast<const float4*>(p + 4 * q);
                v[4 * q] = x.x, v[4 * q + 1] = x.y, v[4 * q + 2] = x.z, v[4 * q + 3] = x.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 32; ++k) v[k] = k < n ? p[k] : 0.f;
        }
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 32; ++k)
            if (k < n) s += (double)v[k];
        const double mean = s / (double)n;
#pragma unroll
        for (int k = 0; k < 32; ++k) v[k] = (float)((double)v[k] - mean);
        if (VEC4) {
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (4 * q < n) *reinterpret_cast<float4*>(p + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < 32; ++k)
                if (k < n) p[k] = v[k];
        }
    }
}

// A strided axis: J seen as [outer, n, inner] with inner contiguous.  A lane owns VEC adjacent lines (outer index o, inner
// indices x .. x + VEC - 1) and walks them along the axis; adjacent lanes own adjacent inner indices, so every load and store
// of a wavefront is a contiguous run (broken only where the lanes pass from one outer index to the next: the j pass, inner =
// nA).  The lines are read twice — once for the sums, once for the subtraction — and written once.  VEC == 4: inner % 4 == 0
// and J 16-byte aligned.
template <int VEC>
__global__ __launch_bounds__(256) void center_axis_kernel(float* __restrict__ J, size_t units, int n, size_t inner) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < units; u += stride) {
        const size_t f = u * VEC, o = f / inner, x = f - o * inner;
        float* p = J + o * (size_t)n * inner + x;
        double s[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) s[q] = 0.0;
#pragma unroll 8
        for (int k = 0; k < n; ++k) {
            if constexpr (VEC == 4) {
                const float4 v = *reinterpret_cast<const float4*>(p + (size_t)k * inner);
                s[0] += (double)v.x, s[1] += (double)v.y, s[2] += (double)v.z, s[3] += (double)v.w;
            } else {
                s[0] += (double)p[(size_t)k * inner];
            }
        }
#pragma unroll
        for (int q = 0; q < VEC; ++q) s[q] /= (double)n;
#pragma unroll 8
        for (int k = 0; k < n; ++k) {
            if constexpr (VEC == 4) {
                float4* at = reinterpret_cast<float4*>(p + (size_t)k * inner);
                float4 v = *at;
                v.x = (float)((double)v.x - s[0]), v.y = (float)((double)v.y - s[1]);
                v.z = (float)((double)v.z - s[2]), v.w = (float)((double)v.w - s[3]);
                *at = v;
            } else {
                float* at = p + (size_t)k * inner;
                *at = (float)((double)*at - s[0]);
            }
        }
    }
}

static unsigned center_blocks(size_t work) { return (unsigned)std::min<size_t>((work + 255) / 256, (size_t)1 << 20); }

static void launch_center_axis(float* J, size_t outer, int n, size_t inner, bool aligned, hipStream_t st) {
    if (aligned && inner % 4 == 0) {
        const size_t units = outer * inner / 4;
        hipLaunchKernelGGL(center_axis_kernel<4>, dim3(center_blocks(units)), dim3(256), 0, st, J, units, n, inner);
    } else {
        const size_t units = outer * inner;
        hipLaunchKernelGGL(center_axis_kernel<1>, dim3(center_blocks(units)), dim3(256), 0, st, J, units, n, inner);
    }
}

hipError_t launch_jacobian_center(float* J, int L, int nA, hipStream_t st) {
    if (!J || L <= 0 || nA <= 0 || nA > 32) return hipErrorInvalidValue;
    const bool aligned = ((uintptr_t)J & 15) == 0;
    const size_t l = (size_t)L, a = (size_t)nA;
    const size_t rows = l * a * l;
    if (aligned && nA % 4 == 0)  // axis b
        hipLaunchKernelGGL(center_rows_kernel<true>, dim3(center_blocks(rows)), dim3(256), 0, st, J, rows, nA);
    else
        hipLaunchKernelGGL(center_rows_kernel<false>, dim3(center_blocks(rows)), dim3(256), 0, st, J, rows, nA);
    launch_center_axis(J, l * a, L, a, aligned, st);       // axis j: [L nA, L, nA]
    launch_center_axis(J, l, nA, l * a, aligned, st);      // axis a: [L, nA, L nA]
    launch_center_axis(J, 1, L, a * l * a, aligned, st);   // axis i: [1, L, nA L nA]
    return hipGetLastError();
}

// ---- the coupling map -------------------------------------------------------------------------------------------------------
// S[i, j] = S[j, i] = sqrt(sum over (a, b) of (0.5 (Jc[i, a, j, b] + Jc[j, b, i, a]))^2) for i <= j: one wavefront (a workgroup
// of 64) per pair, so both halves of S carry the same bits.  X[a][b] = Jc[i, a, j, b] and Y[b][a] = Jc[j, b, i, a] are nA runs
// of nA adjacent floats each; Y is read as it lies in memory and turned round in LDS (row stride nA | 1: the transposed reads
// of a wavefront fall into different banks), which is the one thing here that needs LDS.  Lane l adds the terms e = l, l + 64,
// ... (e = a nA + b) in fp64 in that order (the square and the addition one fused multiply-add), then a butterfly over the 64
// lanes adds the partial sums in a fixed tree; the square root is taken in fp64 and rounded to fp32 once.
__global__ __launch_bounds__(64) void jacobian_contacts_kernel(const float* __restrict__ Jc, float* __restrict__ S, int L, int nA) {
    __shared__ float yt[32 * 33];
    const int lane = threadIdx.x, ld = nA | 1, n2 = nA * nA;
    const size_t pairs = (size_t)L * L, run = (size_t)L * nA;
    for (size_t p = blockIdx.x; p < pairs; p += gridDim.x) {  // workgroup uniform: every lane reaches the barriers
        const int i = (int)(p / L), j = (int)(p - (size_t)i * L);
        if (i > j) continue;
        const float* X = Jc + ((size_t)i * run + j) * nA;
        const float* Y = Jc + ((size_t)j * run + i) * nA;
        __syncthreads();  // the reads of the pair before this one are done
        for (int e = lane; e < n2; e += 64) {
            const int b = e / nA, a = e - b * nA;
            yt[b * ld + a] = Y[(size_t)b * run + a];
        }
        __syncthreads();
        double acc = 0.0;
        for (int e = lane; e < n2; e += 64) {
            const int a = e / nA, b = e - a * nA;
            const double m = 0.5 * ((double)X[(size_t)a * run + b] + (double)yt[b * ld + a]);
            acc = fma(m, m, acc);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) {
            const float s = (float)sqrt(acc);
            S[(size_t)i * L + j] = s;
            S[(size_t)j * L + i] = s;
        }
    }
}

hipError_t launch_jacobian_contacts(const float* Jc, float* S, int L, int nA, hipStream_t st) {
    if (!Jc || !S || L <= 0 || nA <= 0 || nA > 32) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)std::min<size_t>((size_t)L * L, (size_t)1 << 22);
    hipLaunchKernelGGL(jacobian_contacts_kernel, dim3(blocks), dim3(64), 0, st, Jc, S, L, nA);
    return hipGetLastError();
}

// ---- average product correction ---------------------------------------------------------------------------------------------
// C[i, j] = S[i, j] - r_i c_j / s with the diagonal of S taken as zero: r (row sums), c (column sums) and s (their total) in
// fp64, in work[0 : L], work[L : 2 L] and work[2 L].  Row sums: one wavefront per row, lane l adds the columns l, l + 64, ...
// in that order, then the butterfly.  Column sums: one lane per column walks the rows in ascending order (adjacent lanes read
// adjacent floats).  The total: one wavefront over r, the same way.
__global__ __launch_bounds__(256) void apc_row_sums_kernel(const float* __restrict__ S, double* __restrict__ r, int L) {
    const int lane = threadIdx.x & 63;
    for (size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < (size_t)L; row += (size_t)gridDim.x * 4) {  // wave uniform
        double acc = 0.0;
        for (int j = lane; j < L; j += 64)
            if ((size_t)j != row) acc += (double)S[row * L + j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) r[row] = acc;
    }
}

__global__ __launch_bounds__(256) void apc_col_sums_kernel(const float* __restrict__ S, double* __restrict__ c, int L) {
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < (size_t)L; j += (size_t)gridDim.x * 256) {
        double acc = 0.0;
#pragma unroll 8
        for (int i = 0; i < L; ++i)
            if ((size_t)i != j) acc += (double)S[(size_t)i * L + j];
        c[j] = acc;
    }
}

__global__ __launch_bounds__(64) void apc_total_kernel(const double* __restrict__ r, double* __restrict__ total, int L) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < L; i += 64) acc += r[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (threadIdx.x == 0) *total = acc;
}

// in place: the diagonal becomes zero; s == 0 (S is zero off the diagonal, there is nothing to correct) leaves the rest as it is
__global__ __launch_bounds__(256) void apc_apply_kernel(float* __restrict__ S, const double* __restrict__ r,
                                                        const double* __restrict__ c, const double* __restrict__ total, int L) {
    const double s = *total;
    const size_t n = (size_t)L * L, stride = (size_t)gridDim.x * 256;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
        const size_t i = e / L, j = e - i * L;
        float v = S[e];
        if (i == j)
            v = 0.f;
        else if (s != 0.0)
            v = (float)((double)v - r[i] * c[j] / s);
        S[e] = v;
    }
}

hipError_t launch_apc(float* S, double* work, int L, hipStream_t st) {
    if (!S || !work || L <= 0) return hipErrorInvalidValue;
    double *r = work, *c = work + L, *total = work + 2 * (size_t)L;
    hipLaunchKernelGGL(apc_row_sums_kernel, dim3((unsigned)std::min((L + 3) / 4, 65536)), dim3(256), 0, st, S, r, L);
    hipLaunchKernelGGL(apc_col_sums_kernel, dim3((unsigned)std::min((L + 255) / 256, 65536)), dim3(256), 0, st, S, c, L);
    hipLaunchKernelGGL(apc_total_kernel, dim3(1), dim3(64), 0, st, r, total, L);
    const size_t n = (size_t)L * L;
    hipLaunchKernelGGL(apc_apply_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 65536)), dim3(256), 0, st, S, r, c, total, L);
    return hipGetLastError();
}

}  // namespace esmk

// ---- the C ABI (include/esmk.h): validation before any HIP call, then the launchers ---------------------------------------
using namespace esmk;
using namespace esmk_host;

namespace {
constexpr long long kMaxJacobian = 1LL << 40;  // elements of J

// L, nA and the size of J; `copies` (L * nA) against the row limit of the engine
int bad_jacobian_shape(const std::string& w, int L, int nA) {
    if (L <= 0 || nA <= 0) return fail(w + ": L and nA must be positive");
    if (nA > 32) return fail(w + ": nA must be in 1 .. 32");
    const long long copies = (long long)L * nA;
    if (copies > ESMK_MAX_ROWS) return fail(w + ": L*nA exceeds 2^24 copies");
    if (copies * copies >= kMaxJacobian) return fail(w + ": L*nA*L*nA must stay below 2^40 elements");
    return 0;
}
}  // namespace

extern "C" {

int esmk_op_substitute_rows(const int64_t* tokens_dev, const int32_t* src_row_dev, const int32_t* pos_dev, const int32_t* tok_dev,
                            int64_t* out_dev, int B, int T, int n, int V, void* stream) {
    if (!tokens_dev || !pos_dev || !tok_dev || !out_dev) return fail("esmk_op_substitute_rows: null argument");
    if (B <= 0 || T <= 0 || n <= 0 || V <= 0) return fail("esmk_op_substitute_rows: B, T, n and V must be positive");
    if ((long long)B * T > ESMK_MAX_ROWS || (long long)n * T > ESMK_MAX_ROWS)
        return fail("esmk_op_substitute_rows: B*T or n*T exceeds 2^24 rows");
    ESMK_TRY(launch_copy_rows(tokens_dev, src_row_dev, /*start=*/nullptr, /*pos_off=*/nullptr, pos_dev, tok_dev, out_dev, B, T, n, T,
                              /*total=*/0, V, /*head_tok=*/-1, /*tail_tok=*/-1, /*mask_idx=*/0, (hipStream_t)stream));
    return 0;
}

int esmk_op_jacobian_scatter(const float* logits_dev, const float* wt_dev, const int32_t* cols_dev, float* out_dev, int n_copies,
                             int L, int nA, int V, void* stream) {
    if (!logits_dev || !wt_dev || !cols_dev || !out_dev) return fail("esmk_op_jacobian_scatter: null argument");
    if (n_copies <= 0 || V <= 0) return fail("esmk_op_jacobian_scatter: n_copies and V must be positive");
    if (int rc = bad_jacobian_shape("esmk_op_jacobian_scatter", L, nA)) return rc;
    if ((long long)n_copies > (long long)L * nA) return fail("esmk_op_jacobian_scatter: more copies than L*nA");
    if ((long long)n_copies * L > ESMK_MAX_ROWS) return fail("esmk_op_jacobian_scatter: n_copies*L exceeds 2^24 rows");
    ESMK_TRY(launch_jacobian_scatter(logits_dev, wt_dev, cols_dev, out_dev, n_copies, L, nA, V, (hipStream_t)stream));
    return 0;
}

int esmk_op_jacobian_center(float* J_dev, int L, int nA, void* stream) {
    if (!J_dev) return fail("esmk_op_jacobian_center: null argument");
    if (int rc = bad_jacobian_shape("esmk_op_jacobian_center", L, nA)) return rc;
    ESMK_TRY(launch_jacobian_center(J_dev, L, nA, (hipStream_t)stream));
    return 0;
}

int esmk_op_jacobian_contacts(const float* Jc_dev, float* S_out_dev, int L, int nA, void* stream) {
    if (!Jc_dev || !S_out_dev) return fail("esmk_op_jacobian_contacts: null argument");
    if (int rc = bad_jacobian_shape("esmk_op_jacobian_contacts", L, nA)) return rc;
    ESMK_TRY(launch_jacobian_contacts(Jc_dev, S_out_dev, L, nA, (hipStream_t)stream));
    return 0;
}

int esmk_op_apc(float* S_dev, double* work_dev, int L, void* stream) {
    if (!S_dev || !work_dev) return fail("esmk_op_apc: null argument");
    if (L <= 0) return fail("esmk_op_apc: L must be positive");
    if (L > ESMK_MAX_ROWS) return fail("esmk_op_apc: L exceeds 2^24 rows");
    ESMK_TRY(launch_apc(S_dev, work_dev, L, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
