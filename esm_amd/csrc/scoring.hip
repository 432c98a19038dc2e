// scoring.hip — the three small kernels of variant scoring (esmk_forward_rows, include/esmk.h): the masked batch of the
// masked-marginal strategy built on the device, the row gather that lets the head of the model run on the selected rows
// only, and the log-softmax over the vocabulary.  None of them is a hot loop: the layer stack in front of them is the time.
#include "common.h"
#include "kernels.h"
#include <algorithm>

namespace esmk {

// out[i, :] = tokens[src_row[i], :] with position pos[i] replaced by mask_idx — the clone-and-assign of the reference's
// masked-marginal loop for a whole chunk of positions at once.  src_row == nullptr: every row comes from tokens[0].  A
// source row outside [0, B) is clamped; a position outside [0, T) masks nothing.
__global__ __launch_bounds__(256) void mask_rows_kernel(const int64_t* __restrict__ tokens, const int* __restrict__ src_row,
                                                        const int* __restrict__ pos, int64_t* __restrict__ out, int B, int T,
                                                        int n, int64_t mask_idx) {
    const size_t total = (size_t)n * T;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const int i = (int)(e / T), t = (int)(e - (size_t)i * T);
        const int b = src_row ? min(max(src_row[i], 0), B - 1) : 0;
        out[e] = t == pos[i] ? mask_idx : tokens[(size_t)b * T + t];
    }
}

hipError_t launch_mask_rows(const int64_t* tokens, const int* src_row, const int* pos, int64_t* out, int B, int T, int n,
                            int mask_idx, hipStream_t st) {
    if (B <= 0 || T <= 0 || n <= 0) return hipErrorInvalidValue;
    const size_t total = (size_t)n * T;
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(mask_rows_kernel, dim3(blocks), dim3(256), 0, st, tokens, src_row, pos, out, B, T, n, (int64_t)mask_idx);
    return hipGetLastError();
}

// out[i, :] = x[clamp(sel[i], 0, N - 1), :]: fp32 rows of E values, E % 4 == 0, 16 bytes per lane.  The clamp makes an index
// the host never saw (it is device data) read a valid row instead of faulting.
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ x, const int* __restrict__ sel,
                                                          float* __restrict__ out, int N, int E4, int n) {
    const size_t total = (size_t)n * E4;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const int i = (int)(e / E4), c = (int)(e - (size_t)i * E4);
        const int r = min(max(sel[i], 0), N - 1);
        reinterpret_cast<f32x4*>(out)[e] = reinterpret_cast<const f32x4*>(x)[(size_t)r * E4 + c];
    }
}

hipError_t launch_gather_rows(const float* x, const int* sel, float* out, int N, int E, int n, hipStream_t st) {
    if (N <= 0 || n <= 0 || E <= 0 || E % 4 != 0) return hipErrorInvalidValue;
    const size_t total = (size_t)n * (E / 4);
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks), dim3(256), 0, st, x, sel, out, N, E / 4, n);
    return hipGetLastError();
}

// torch.log_softmax(logits, -1) of [n, V] fp32 rows, V <= 64: one wavefront per row, one vocabulary entry per lane.  The row
// maximum and the sum of exp(x - max) are butterfly reductions over the 64 lanes (every lane ends with the same value, the
// same bits whatever the row's place in the launch); lanes past V carry -inf / 0.  expf and logf are the precise ones.
// target != nullptr: tgt_out[i] = the log-probability at column clamp(target[i], 0, V - 1) — the register of that lane, so
// it is the entry of the full output bit for bit.
__global__ __launch_bounds__(256) void log_softmax_rows_kernel(const float* __restrict__ logits, float* __restrict__ out,
                                                               const int* __restrict__ target, float* __restrict__ tgt_out,
                                                               int n, int V) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;  // wave uniform
    const float x = lane < V ? logits[(size_t)row * V + lane] : -INFINITY;
    float mx = x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const float sum = wave_sum(lane < V ? expf(x - mx) : 0.f);
    const float lp = (x - mx) - logf(sum);
    if (lane < V) out[(size_t)row * V + lane] = lp;
    if (target != nullptr) {
        const float t = __shfl(lp, min(max(target[row], 0), V - 1), 64);
        if (lane == 0) tgt_out[row] = t;
    }
}

hipError_t launch_log_softmax_rows(const float* logits, float* out, const int* target, float* tgt_out, int n, int V,
                                   hipStream_t st) {
    if (n <= 0 || V <= 0 || V > 64 || (target != nullptr && tgt_out == nullptr)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(log_softmax_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, logits, out, target, tgt_out,
                       n, V);
    return hipGetLastError();
}

}  // namespace esmk
