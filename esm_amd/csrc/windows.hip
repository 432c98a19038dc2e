// windows.hip — the small kernels of windowed scoring and embedding (esm_amd/windows.py): proteins longer than the model's
// window are run as model-sized window copies built on the device (copy_rows_kernel, scoring.hip), and the per-window outputs
// are stitched back into full-length outputs.  None of them is a hot loop: the layer stack between them is the time.  All index lists are device
// data the host never saw: every index is clamped, nothing is read or written out of bounds; plain vector stores, no atomics.
#include "common.h"
#include "kernels.h"
#include <algorithm>

namespace esmk {

// out[r, :] = (sum_k w[k] x[src[k], :]) / sum_k w[k] over k in [off[r], off[r + 1]), ascending: the stitch of per-window rows
// into full-length rows.  One lane per 4 neighbouring output elements (16 bytes of fp32), no exchange between lanes: every
// element is accumulated in fp32 in list order by one lane, so the result does not depend on the launch geometry.  A list
// of ONE entry copies the row (converted to fp32) exactly — the owner stitch — and an empty list gives zeros.  src is clamped
// to [0, N), the offsets to [0, total] (hi < lo: an empty list).  Weights are positive by contract.
template <typename T>
__global__ __launch_bounds__(256) void blend_rows_kernel(const T* __restrict__ x, const int* __restrict__ off,
                                                         const int* __restrict__ src, const float* __restrict__ w,
                                                         float* __restrict__ out, int N, int E4, int n_out, int total) {
    const size_t count = (size_t)n_out * E4;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < count; e += stride) {
        const int r = (int)(e / E4), c = (int)(e - (size_t)r * E4);
        const int lo = min(max(off[r], 0), total), hi = min(max(off[r + 1], 0), total);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        float wsum = 0.f;
        for (int k = lo; k < hi; ++k) {
            const int row = min(max(src[k], 0), N - 1);
            const T* p = x + ((size_t)row * E4 + c) * 4;
            f32x4 v;
            if constexpr (sizeof(T) == 4) {
                v = *reinterpret_cast<const f32x4*>(p);
            } else {
                const typename Op<T>::v4 q = *reinterpret_cast<const typename Op<T>::v4*>(p);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = (float)q[i];
            }
            if (hi - lo == 1) {
                acc = v;
                wsum = 1.f;
            } else {
                const float wk = w[k];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] += wk * v[i];
                wsum += wk;
            }
        }
        if (hi - lo > 1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = acc[i] / wsum;
        }
        reinterpret_cast<f32x4*>(out)[e] = acc;
    }
}

hipError_t launch_blend_rows(const void* x, int x_dtype, const int* off, const int* src, const float* w, float* out, int N, int E,
                             int n_out, int total, hipStream_t st) {
    if (!x || !off || !src || !w || !out || N <= 0 || E <= 0 || E % 4 != 0 || n_out <= 0 || total < 0) return hipErrorInvalidValue;
    const size_t count = (size_t)n_out * (E / 4);
    const dim3 grid((unsigned)std::min<size_t>((count + 255) / 256, 16384));
    if (x_dtype == ESMK_DT_F32)
        hipLaunchKernelGGL(blend_rows_kernel<float>, grid, dim3(256), 0, st, (const float*)x, off, src, w, out, N, E / 4, n_out, total);
    else if (x_dtype == ESMK_DT_F16)
        hipLaunchKernelGGL(blend_rows_kernel<_Float16>, grid, dim3(256), 0, st, (const _Float16*)x, off, src, w, out, N, E / 4, n_out,
                           total);
    else if (x_dtype == ESMK_DT_BF16)
        hipLaunchKernelGGL(blend_rows_kernel<__bf16>, grid, dim3(256), 0, st, (const __bf16*)x, off, src, w, out, N, E / 4, n_out,
                           total);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

// out[i, j] (body coordinates, [Lb, Lb]) = maps[w, i - s_w, j - s_w] of the window w that owns the pair: among the windows
// that hold both residues (s_w <= i, j < s_w + R, s_w = start[w] - body_lo) the one with the least |2 s_w + R - 1 - (i + j)|,
// a tie going to the lower start; NaN where no window holds both.  n_w is small: each lane walks the window list.  The
// starts are device data: a window is read only through indices checked to lie in [0, R), whatever its start.
__global__ __launch_bounds__(256) void stitch_contacts_kernel(const float* __restrict__ maps, const int* __restrict__ start,
                                                              float* __restrict__ out, int n_w, int R, int Lb, int body_lo) {
    const size_t count = (size_t)Lb * Lb;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < count; e += stride) {
        const long long i = (long long)(e / Lb), j = (long long)(e - (size_t)i * Lb);
        long long best_key = 0, best_s = 0;
        int best = -1;
        for (int w = 0; w < n_w; ++w) {
            const long long s = (long long)start[w] - body_lo;
            if (i < s || i >= s + R || j < s || j >= s + R) continue;
            long long key = 2 * s + R - 1 - (i + j);
            key = key < 0 ? -key : key;
            if (best < 0 || key < best_key || (key == best_key && s < best_s)) {
                best = w;
                best_key = key;
                best_s = s;
            }
        }
        out[e] = best < 0 ? __builtin_nanf("") : maps[((size_t)best * R + (size_t)(i - best_s)) * R + (size_t)(j - best_s)];
    }
}

hipError_t launch_stitch_contacts(const float* maps, const int* start, float* out, int n_w, int R, int Lb, int body_lo,
                                  hipStream_t st) {
    if (!maps || !start || !out || n_w <= 0 || R <= 0 || Lb <= 0) return hipErrorInvalidValue;
    const size_t count = (size_t)Lb * Lb;
    const unsigned blocks = (unsigned)std::min<size_t>((count + 255) / 256, 16384);
    hipLaunchKernelGGL(stitch_contacts_kernel, dim3(blocks), dim3(256), 0, st, maps, start, out, n_w, R, Lb, body_lo);
    return hipGetLastError();
}

}  // namespace esmk
