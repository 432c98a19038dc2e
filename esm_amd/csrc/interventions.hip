// interventions.hip — writes into the fp32 residual stream between two layers: activation patching,
// steering, ablation.  What a forward hook on model.layers[k] does to the reference (it returns a changed output and every
// later layer sees it) is one launch of stream_edit_kernel per edit here, between ffn_stage and the capture of
// representation k (engine.hip, stream_edit_stage).
#include "common.h"
#include "kernels.h"
#include "../../include/esmk.h"

#include <algorithm>

namespace esmk {

namespace {

// The arithmetic of an edit is stated operation by operation (include/esmk.h): mul_rn / add_rn / sub_rn (common.h) round
// products and sums one at a time, so numpy float32 reproduces x' bit for bit.
ESMK_DEV double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

}  // namespace

// One wavefront per edited row, grid-stride over the edit's rows (the row list, or all N rows under the token selector);
// no atomics, and nothing depends on the block or thread index beyond which row a wave owns.  The row stays in registers
// (lane l holds the f32x4 chunks l, l + 64, ... as rowstats_kernel does) from its load to the last store.
//
// Fold outputs (a.y != null): the row's mean, rstd and y = T(x' - mean) are computed by the statements of rowstats_kernel
// (elementwise.hip) — the same lane layout, pairwise partial sum, two-pass variance and wave_sum, under the same
// compiler flags — so they are the bits esmk_op_rowstats gives on x' (tests/test_stream_edit_ops_gpu.py holds this).
template <typename T, int NCH>
__global__ __launch_bounds__(256) void stream_edit_kernel(const StreamEditArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * 4;
    const int count = a.rows ? a.n_rows : a.N;
    const int E = a.E, e4 = E >> 2;
    for (int i = wave; i < count; i += nwaves) {
        int row = i;
        if (a.rows) {
            row = a.rows[i];
            if (row < 0 || row >= a.N) continue;  // listed rows outside [0, N) are skipped
        } else {
            const int64_t tok = a.tokens[i];
            if (tok < 0 || tok >= 64 || !((a.token_set >> tok) & 1ull)) continue;
        }
        const float* sr = nullptr;
        if (a.src) {
            sr = a.src;
            if (a.src_ld != 0) {
                const int si = a.src_index ? a.src_index[i] : i;  // (i is the row itself under the token selector)
                if (si < 0 || si >= a.n_src) continue;            // no source row: the row is left alone
                sr = a.src + (size_t)si * a.src_ld;
            }
        }
        float* xr = a.x + (size_t)row * E;
        f32x4 v[NCH];
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = lane + 64 * k;
            v[k] = c < e4 ? reinterpret_cast<const f32x4*>(xr)[c] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (a.op == ESMK_EDIT_PROJECT) {
            // c = gain <x, s> / <s, s>, both dot products in fp64 from the fp32 inputs: lane-strided partials in chunk
            // order, then the butterfly; rounded once to fp32
            f32x4 s[NCH];
            double dxs = 0.0, dss = 0.0;
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                const int c = lane + 64 * k;
                s[k] = c < e4 ? reinterpret_cast<const f32x4*>(sr)[c] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    dxs += (double)v[k][e] * (double)s[k][e];
                    dss += (double)s[k][e] * (double)s[k][e];
                }
            }
            dxs = wave_sum_f64(dxs);
            dss = wave_sum_f64(dss);
            if (dss == 0.0) continue;  // no direction: the row is left unchanged, in every buffer
            const float coef = (float)((double)a.gain * dxs / dss);
#pragma unroll
            for (int k = 0; k < NCH; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e) v[k][e] = sub_rn(v[k][e], mul_rn(coef, s[k][e]));
        } else if (sr) {  // x' = keep x + gain s
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                const int c = lane + 64 * k;
                const f32x4 s = c < e4 ? reinterpret_cast<const f32x4*>(sr)[c] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) v[k][e] = add_rn(mul_rn(a.keep, v[k][e]), mul_rn(a.gain, s[e]));
            }
        } else {  // x' = keep x
#pragma unroll
            for (int k = 0; k < NCH; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e) v[k][e] = mul_rn(a.keep, v[k][e]);
        }
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = lane + 64 * k;
            if (c < e4) reinterpret_cast<f32x4*>(xr)[c] = v[k];
        }
        if (a.y == nullptr) continue;
        // the edited row re-enters the LayerNorm-fold chain the way layer 0 does: rowstats_kernel's statements on x'
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) t += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
        const float mean = wave_sum(t) / (float)E;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = lane + 64 * k;
            if (c < e4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[k][e] -= mean;
                    q += v[k][e] * v[k][e];
                }
            }
        }
        const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)E + 1e-5f);
        if (lane == 0) {
            a.mean[row] = mean;
            a.rstd[row] = rstd;
        }
        T* yr = (T*)a.y + (size_t)row * a.ldy;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = lane + 64 * k;
            if (c < e4) {  // columns [E, ldy) are not written
                typename Op<T>::v4 pk;
#pragma unroll
                for (int e = 0; e < 4; ++e) pk[e] = Op<T>::from(v[k][e]);
                *reinterpret_cast<typename Op<T>::v4*>(yr + c * 4) = pk;
            }
        }
    }
}

hipError_t launch_stream_edit(const StreamEditArgs& a, int operand_dtype, hipStream_t st) {
    if (!a.x || a.N <= 0 || a.E <= 0 || a.E % 4 != 0 || a.E > 5120) return hipErrorInvalidValue;
    if (a.op != ESMK_EDIT_AXPBY && a.op != ESMK_EDIT_PROJECT) return hipErrorInvalidValue;
    if (a.op == ESMK_EDIT_PROJECT && !a.src) return hipErrorInvalidValue;
    if (a.rows ? a.n_rows < 0 : a.tokens == nullptr) return hipErrorInvalidValue;
    if (a.src && a.src_ld != 0 && (a.src_ld < a.E || a.src_ld % 4 != 0 || a.n_src <= 0)) return hipErrorInvalidValue;
    if (a.y && (!a.mean || !a.rstd || a.ldy < a.E || a.ldy % 4 != 0)) return hipErrorInvalidValue;
    const int count = a.rows ? a.n_rows : a.N;
    if (count == 0) return hipSuccess;
    // memory bound: at most 8 workgroups per CU, the rest of the rows by the grid stride
    const unsigned blocks = (unsigned)std::min((count + 3) / 4, 2048);
#define ESMK_SE(TT, NN) hipLaunchKernelGGL((stream_edit_kernel<TT, NN>), dim3(blocks), dim3(256), 0, st, a)
#define ESMK_SE_T(TT)                 \
    if (a.E <= 512) ESMK_SE(TT, 2);   \
    else if (a.E <= 1280) ESMK_SE(TT, 5);  \
    else if (a.E <= 2560) ESMK_SE(TT, 10); \
    else ESMK_SE(TT, 20);
    if (operand_dtype == ESMK_DT_BF16) { ESMK_SE_T(__bf16) } else { ESMK_SE_T(_Float16) }
#undef ESMK_SE_T
#undef ESMK_SE
    return hipGetLastError();
}

}  // namespace esmk
