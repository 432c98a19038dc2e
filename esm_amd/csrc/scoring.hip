// scoring.hip — the small kernels of variant scoring (esmk_forward_rows, include/esmk.h): the masked batch of the
// masked-marginal strategy built on the device (one position per copy, or a list of positions per copy for multi-mutant
// variants), the row gather that lets the head of the model run on the selected rows only, the log-softmax over the
// vocabulary and the per-variant sum of log p(mt) - log p(wt).  None of them is a hot loop: the layer stack in front of
// them is the time.
#include "common.h"
#include "kernels.h"
#include <algorithm>

namespace esmk {

// Every token copy with listed positions overwritten, in one kernel: the masked batch of the masked-marginal strategy
// (esmk_op_mask_rows: the clone-and-assign of the reference's loop for a whole chunk of positions at once), the joint mask of a
// multi-mutant variant (esmk_op_mask_rows_multi), the substituted copies of the categorical Jacobian (esmk_op_substitute_rows)
// and the window copies of a protein longer than the model's window (esmk_op_window_rows).
// Copy i, column c, holds tokens[clamp(src_row[i]), clamp(start[i] + c - h)], h = 1 if head_tok >= 0 else 0; column 0 is
// head_tok when head_tok >= 0 and column Tw - 1 is tail_tok when tail_tok >= 0 (a wrapped window: a fragment tokenised as
// the alphabet tokenises the substring; both negative: a raw token slice).  The entries of pos[pos_off[i] : pos_off[i + 1]] are
// token coordinates of the SOURCE row: entry p becomes mask_idx at column p - start[i] + h where that is a body column (not
// an overridden one) of the copy; any other entry masks nothing.  One workgroup per copy, copies strided over the grid; the
// row is written, then (behind the barrier, so that the mask lands on top of the copy) the lanes stride over the copy's list.
// A source row outside [0, B) and a source column outside [0, T) are clamped, the offsets to [0, total] (hi < lo: an empty
// list, a plain copy), a repeated entry stores the same value twice.  Columns are computed in 64 bits: no start overflows.
// What the three plain forms leave out is null: src_row (every copy comes from tokens[0]), start (0: with Tw = T and no head or
// tail a position is its own column, and one outside [0, T) masks nothing), pos_off (the list of copy i is pos[i] alone), and
// tok, the replacement token per copy in place of mask_idx: a tok[i] outside [0, V) substitutes nothing.
__global__ __launch_bounds__(256) void copy_rows_kernel(const int64_t* __restrict__ tokens, const int* __restrict__ src_row,
                                                        const int* __restrict__ start, const int* __restrict__ pos_off,
                                                        const int* __restrict__ pos, const int* __restrict__ tok,
                                                        int64_t* __restrict__ out, int B, int T, int n, int Tw, int total, int V,
                                                        int64_t head_tok, int64_t tail_tok, int64_t mask_idx) {
    const int h = head_tok >= 0 ? 1 : 0;
    const int body_end = tail_tok >= 0 ? Tw - 1 : Tw;  // body columns: [h, body_end)
    for (int i = blockIdx.x; i < n; i += gridDim.x) {  // workgroup uniform: every lane reaches the barrier
        const int b = src_row ? min(max(src_row[i], 0), B - 1) : 0;
        const long long s = (start ? (long long)start[i] : 0ll) - h;  // source column of copy column 0
        const int64_t* in = tokens + (size_t)b * T;
        int64_t* o = out + (size_t)i * Tw;
        // the list's bounds, the replacement and the lane's first entry are read in front of the copy: their latency passes
        // under it instead of standing behind the barrier
        int lo = i, hi = i + 1;
        if (pos_off) lo = min(max(pos_off[i], 0), total), hi = min(max(pos_off[i + 1], 0), total);
        int64_t v = mask_idx;
        if (tok) {
            v = tok[i];
            if (v < 0 || v >= V) hi = lo;
        }
        int j = lo + (int)threadIdx.x;
        long long at = j < hi ? (long long)pos[j] - s : -1;  // the copy column of entry j; -1 is no body column
#pragma unroll 4
        for (int c = threadIdx.x; c < Tw; c += 256) {
            const long long t = min(max(s + c, 0ll), (long long)T - 1);
            int64_t x = in[t];
            if (c == Tw - 1 && tail_tok >= 0) x = tail_tok;
            if (c == 0 && head_tok >= 0) x = head_tok;
            o[c] = x;
        }
        __syncthreads();
        while (j < hi) {
            if (at >= h && at < body_end) o[at] = v;
            j += 256;
            if (j < hi) at = (long long)pos[j] - s;
        }
    }
}

hipError_t launch_copy_rows(const int64_t* tokens, const int* src_row, const int* start, const int* pos_off, const int* pos,
                            const int* tok, int64_t* out, int B, int T, int n, int Tw, int total, int V, int head_tok, int tail_tok,
                            int mask_idx, hipStream_t st) {
    if (!tokens || !pos || !out || B <= 0 || T <= 0 || n <= 0 || Tw <= 0 || (pos_off && total < 0) || (tok && V <= 0))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(copy_rows_kernel, dim3((unsigned)std::min(n, 8192)), dim3(256), 0, st, tokens, src_row, start, pos_off, pos,
                       tok, out, B, T, n, Tw, total, V, (int64_t)head_tok, (int64_t)tail_tok, (int64_t)mask_idx);
    return hipGetLastError();
}

// The packed counterpart of esmk_op_mask_rows_multi (esmk_forward_packed_rows): copy i is the first seg_len[i] tokens of
// tokens[src_row[i]], written to out[seg_start[i] : seg_start[i] + seg_len[i]] of ONE row space of `rows` rows, with every
// position of pos[pos_off[i] : pos_off[i + 1]] replaced by mask_idx; the gap behind the copy — up to seg_start[i + 1], or to
// `rows` behind the last copy — is filled with pad_idx (esmk_forward_packed wants pad_idx in gap rows; nothing is assumed
// about what `out` held).  One workgroup per copy, copies strided over the grid: copy and gap fill, barrier, then the mask
// on top.  The copies' row ranges are disjoint by contract, so no two workgroups write the same row.  The lists are device
// data the host never saw: a source row outside [0, B) is clamped, seg_len to [0, T], the written range to [0, rows), the
// offsets to [0, total] (hi < lo: an empty list), a position outside [0, seg_len) masks nothing, and a repeated position
// stores the same value twice.
__global__ __launch_bounds__(256) void mask_rows_packed_kernel(const int64_t* __restrict__ tokens, const int* __restrict__ src_row,
                                                               const int* __restrict__ seg_start, const int* __restrict__ seg_len,
                                                               const int* __restrict__ pos_off, const int* __restrict__ pos,
                                                               int64_t* __restrict__ out, int B, int T, int n, int total, int rows,
                                                               int64_t mask_idx, int64_t pad_idx) {
    for (int i = blockIdx.x; i < n; i += gridDim.x) {  // workgroup uniform: every lane reaches the barrier
        const int b = min(max(src_row[i], 0), B - 1);
        const int64_t* in = tokens + (size_t)b * T;
        const int start = min(max(seg_start[i], 0), rows);
        const int len = min(min(max(seg_len[i], 0), T), rows - start);
        const int end = i + 1 < n ? min(max(seg_start[i + 1], start), rows) : rows;  // the gap's end; below start + len: no gap
        int64_t* o = out + start;
        for (int t = threadIdx.x; t < len; t += 256) o[t] = in[t];
        for (int r = start + len + (int)threadIdx.x; r < end; r += 256) out[r] = pad_idx;
        __syncthreads();
        const int lo = min(max(pos_off[i], 0), total), hi = min(max(pos_off[i + 1], 0), total);
        for (int j = lo + (int)threadIdx.x; j < hi; j += 256) {
            const int p = pos[j];
            if (p >= 0 && p < len) o[p] = mask_idx;
        }
    }
}

hipError_t launch_mask_rows_packed(const int64_t* tokens, const int* src_row, const int* seg_start, const int* seg_len,
                                   const int* pos_off, const int* pos, int64_t* out, int B, int T, int n, int total, int rows,
                                   int mask_idx, int pad_idx, hipStream_t st) {
    if (!tokens || !src_row || !seg_start || !seg_len || !pos_off || !pos || !out || B <= 0 || T <= 0 || n <= 0 || total < 0 ||
        rows <= 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_rows_packed_kernel, dim3((unsigned)std::min(n, 8192)), dim3(256), 0, st, tokens, src_row, seg_start,
                       seg_len, pos_off, pos, out, B, T, n, total, rows, (int64_t)mask_idx, (int64_t)pad_idx);
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

// out[v] = sum over r in [var_off[v], var_off[v + 1]), ascending, of (lp[r, mt[r]] - lp[r, wt[r]]): the masked-marginal score of
// variant v from its rows of log-probabilities.  Each term is the fp32 difference (the bits score_mutations gives a single
// mutant), the terms are added in fp64 in index order by ONE lane per variant: the result does not depend on the launch
// geometry, which a sum through atomics (torch.index_add_ on the device) would.  Columns are clamped to [0, V), offsets to
// [0, n_rows]; an empty range (hi <= lo) gives 0.0.
__global__ __launch_bounds__(256) void score_rows_kernel(const float* __restrict__ lp, const int* __restrict__ wt,
                                                         const int* __restrict__ mt, const int* __restrict__ var_off,
                                                         double* __restrict__ out, int n_rows, int n_var, int V) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < (size_t)n_var; v += stride) {
        const int lo = min(max(var_off[v], 0), n_rows), hi = min(max(var_off[v + 1], 0), n_rows);
        double sum = 0.0;
        for (int r = lo; r < hi; ++r) {
            const float* row = lp + (size_t)r * V;
            const float term = row[min(max(mt[r], 0), V - 1)] - row[min(max(wt[r], 0), V - 1)];
            sum += (double)term;
        }
        out[v] = sum;
    }
}

hipError_t launch_score_rows(const float* lp, const int* wt, const int* mt, const int* var_off, double* out, int n_rows,
                             int n_var, int V, hipStream_t st) {
    if (!lp || !wt || !mt || !var_off || !out || n_rows <= 0 || n_var <= 0 || V <= 0) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)std::min<size_t>(((size_t)n_var + 255) / 256, 8192);
    hipLaunchKernelGGL(score_rows_kernel, dim3(blocks), dim3(256), 0, st, lp, wt, mt, var_off, out, n_rows, n_var, V);
    return hipGetLastError();
}

// out[s] = sum over r in [off[s], off[s + 1]), ascending, of lp[r, target[r]]: the pseudo-log-likelihood of sequence s from its
// rows of log-probabilities.  The terms are fp32, added in fp64 in index order by ONE lane per sequence, as score_rows_kernel
// adds a variant's: no atomics, a result that does not depend on the launch geometry.  target is clamped to [0, V), the
// offsets to [0, n_rows]; an empty range (hi <= lo) gives 0.0.
__global__ __launch_bounds__(256) void sum_target_rows_kernel(const float* __restrict__ lp, const int* __restrict__ target,
                                                              const int* __restrict__ off, double* __restrict__ out, int n_rows,
                                                              int n_seq, int V) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t s = (size_t)blockIdx.x * 256 + threadIdx.x; s < (size_t)n_seq; s += stride) {
        const int lo = min(max(off[s], 0), n_rows), hi = min(max(off[s + 1], 0), n_rows);
        double sum = 0.0;
        for (int r = lo; r < hi; ++r) sum += (double)lp[(size_t)r * V + min(max(target[r], 0), V - 1)];
        out[s] = sum;
    }
}

hipError_t launch_sum_target_rows(const float* lp, const int* target, const int* off, double* out, int n_rows, int n_seq, int V,
                                  hipStream_t st) {
    if (!lp || !target || !off || !out || n_rows <= 0 || n_seq <= 0 || V <= 0) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)std::min<size_t>(((size_t)n_seq + 255) / 256, 8192);
    hipLaunchKernelGGL(sum_target_rows_kernel, dim3(blocks), dim3(256), 0, st, lp, target, off, out, n_rows, n_seq, V);
    return hipGetLastError();
}

}  // namespace esmk
