// pair_head.hip — linear pairwise heads on the attention maps WITHOUT the [B,L,H,T,T] attention tensor.
//
// Reference: examples/lm-design/utils/linear_projection.py:85-135 (LinearProjectionDistogramModel): two 1 x 1 convolutions
// over the L*H attention channels, conv1 on the symmetrised maps P + P^T (distance and omega bins), conv2 on the maps as they
// are (theta and phi bins); only the first / last position is cropped (linear_projection.py:76-82), no <eos> mask, no APC.
// With W [L*H][C_out] = the two weight matrices side by side (n_sym columns of conv1, then n_asym of conv2):
//     Z[b,i,j,o]   = sum_{c ascending} W[c,o] P_c[b,i,j]                 (fp32 FMA chain, one writer per element)
//     out[b,i,j,o] = Z[b,i,j,o] + Z[b,j,i,o] + bias[o]   for o < n_sym,     Z[b,i,j,o] + bias[o]   for the rest
// P_c is recomputed from the layer's q, k (operand dtype, log2 domain) and row log-sum-exp, as contacts.hip does: the engine
// keeps every layer's q / k / lse in a stacked [L,B,H,T,slots] / [L,B,H,T] stash and ONE launch after the last layer walks the
// L*H channels of a pair tile with the tile's accumulators resident in registers (a per-layer
// read-modify-write of a [T,T,64] fp32 accumulator would move more bytes than the forward).
//
// Form: vector FMA.  A workgroup of 8 waves owns a 32 x 32 pair tile; wave w = (query half, key half, output half) owns a
// 16 x 16 sub-tile times 32 outputs: S = q k^T by v_mfma_f32_16x16x32 (2 instructions per head at 64 slots, 4 at 128),
// P = exp2(S - lse) in the four result registers, then 4 pairs x 32 outputs of v_pk_fma_f32 — 128 accumulator VGPRs.  The
// weight row W[c, 32 og .. 32 og + 32) is wave uniform (c is the loop variable), so it comes from scalar loads and costs no
// vector register.  The two waves of an output pair recompute S and P (2 MFMAs, 4 exp2 against 64 packed FMAs).  Rows and
// columns of <pad> tokens (key_bias != 0, as attn_probs_rows reads it, or the token) and of positions past T are exact zeros by a select,
// so a sequence's map never depends on the batch it ran in.  The ESM-1 null key is in lse and has no column.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace esmk {

namespace {

// grid: B * ceil(T/32)^2, key tile fastest.  q, k [L,B,H,T,HD]; lse [L,B,H,T] (log2 domain); key_bias, tokens [B,T] or null;
// w64 [L*H][64] (columns >= C_out zero); out [B,S,S,C_out] receives Z
template <typename T, int HD>
__global__ __launch_bounds__(512) void pair_head_accum_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                              const float* __restrict__ lse,
                                                              const float* __restrict__ key_bias,
                                                              const int64_t* __restrict__ tokens,
                                                              const float* __restrict__ w64, float* __restrict__ out, int L,
                                                              int B, int H, int Tlen, int C_out, int bos, int S, int pad_idx) {
    using V8 = typename Op<T>::v8;
    constexpr int KS = HD / 32;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int og = wave >> 2;  // outputs [32 og, 32 og + 32)
    if (32 * og >= C_out) return;  // no barrier below: waves are independent
    const int nt = (Tlen + 31) >> 5;
    // XCD-remapped: the tiles of one sequence, which read the same q / k rows channel after channel, share an L2
    int id = xcd_remap(blockIdx.x, gridDim.x);
    const int tj = id % nt;
    id /= nt;
    const int ti = id % nt;
    const int b = id / nt;
    const int q0 = ti * 32 + 16 * (wave & 1), k0 = tj * 32 + 16 * ((wave >> 1) & 1);
    // sub-tiles with no pair inside the crop [bos, bos + S) x [bos, bos + S)
    if (q0 >= bos + S || q0 + 16 <= bos || k0 >= bos + S || k0 + 16 <= bos) return;

    const int lm = lane & 15, lq = lane >> 4;
    const int qa = min(q0 + lm, Tlen - 1);  // row of this lane's A fragment
    const int kr = min(k0 + lm, Tlen - 1);  // row of its B fragment = the key of its results
    const int key = k0 + lm;
    // a <pad> position: a key bias that is not 0 (attn_probs_rows), or the token itself where tokens are given
    auto is_pad = [&](int t) -> bool {
        const size_t o = (size_t)b * Tlen + t;
        return (key_bias != nullptr && key_bias[o] != 0.f) || (tokens != nullptr && tokens[o] == pad_idx);
    };
    const bool keepk = key < Tlen && !is_pad(kr);
    bool keep[4];
    int qd[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = q0 + 4 * lq + r;  // query of result register r
        qd[r] = min(qi, Tlen - 1);
        keep[r] = keepk && qi < Tlen && !is_pad(qd[r]);
    }

    f32x2 acc[4][16];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int o = 0; o < 16; ++o) acc[r][o] = f32x2{0.f, 0.f};

    // channel c = layer * H + head: its rows start at ((layer * B + b) * H + head) * T; `base` walks them without a division
    const size_t step_h = (size_t)Tlen, step_l = ((size_t)(B - 1) * H + 1) * (size_t)Tlen;
    auto load = [&](V8 (&qf)[KS], V8 (&kf)[KS], float (&ls)[4], size_t base) {
        const T* qp = q + (base + qa) * HD + 8 * lq;
        const T* kp = k + (base + kr) * HD + 8 * lq;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qf[ks] = *reinterpret_cast<const V8*>(qp + 32 * ks);
            kf[ks] = *reinterpret_cast<const V8*>(kp + 32 * ks);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) ls[r] = lse[base + qd[r]];
    };
    // P of one channel in the four result registers: D[query 4 lq + r][key lm]; a select, not a multiply, zeroes <pad> rows
    // and columns (the lse of a <pad> row is not its own: attention.hip)
    auto probs = [&](const V8 (&qf)[KS], const V8 (&kf)[KS], const float (&ls)[4], float (&p)[4]) {
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) s = Op<T>::mma16(qf[ks], kf[ks], s);
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = keep[r] ? __builtin_amdgcn_exp2f(s[r] - ls[r]) : 0.f;
    };
    // Three stages in flight: the FMAs of channel c, P of channel c + 1 (its MFMA -> exp2 chain interleaves with the FMAs), the
    // operand loads of channel c + 2.  The loads are pinned in front of the arithmetic: left to the scheduler they sink to
    // their first use (fewer live registers) and every channel waits a full memory latency in front of its MFMA.
    const int C = L * H;
    size_t base = (size_t)b * H * (size_t)Tlen;  // channel 0
    int hcount = 0;                              // head of the channel `base` points at
    auto advance = [&](bool go) {  // to the next channel if `go` (scalar selects: the loop body stays one basic block)
        const bool wrap = hcount + 1 >= H;
        base += go ? (wrap ? step_l : step_h) : (size_t)0;
        hcount = go ? (wrap ? 0 : hcount + 1) : hcount;
    };
    // two operand sets used in turn (no register copies: a copy would wait for the load it copies)
    V8 qa_[KS], ka_[KS], qb_[KS], kb_[KS];
    float la_[4], lb_[4], p[4];
    load(qa_, ka_, la_, base);
    probs(qa_, ka_, la_, p);  // channel 0
    advance(C > 1);
    load(qa_, ka_, la_, base);  // channel min(1, C - 1)
    // one channel: X holds the operands of channel c + 1, Y receives those of channel c + 2
    auto channel = [&](int c, V8 (&xq)[KS], V8 (&xk)[KS], float (&xl)[4], V8 (&yq)[KS], V8 (&yk)[KS], float (&yl)[4]) {
        advance(c + 2 < C);
        load(yq, yk, yl, base);  // channel min(c + 2, C - 1)
        const float* wr = w64 + (size_t)c * 64 + 32 * og;  // wave uniform: scalar loads
        f32x2 wv[16];
#pragma unroll
        for (int o = 0; o < 16; ++o) wv[o] = f32x2{wr[2 * o], wr[2 * o + 1]};
        __builtin_amdgcn_sched_barrier(0);
        float pn[4];
        probs(xq, xk, xl, pn);  // channel min(c + 1, C - 1)
#pragma unroll
        for (int o = 0; o < 16; ++o)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r][o] = __builtin_elementwise_fma(wv[o], f32x2{p[r], p[r]}, acc[r][o]);
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = pn[r];
    };
    int c = 0;
    if (C & 1) {  // an odd count: one channel in front, so that the loop below runs whole pairs and has no branch inside
        channel(0, qa_, ka_, la_, qb_, kb_, lb_);
        for (c = 1; c < C; c += 2) {
            channel(c, qb_, kb_, lb_, qa_, ka_, la_);
            channel(c + 1, qa_, ka_, la_, qb_, kb_, lb_);
        }
    } else {
        for (; c < C; c += 2) {
            channel(c, qa_, ka_, la_, qb_, kb_, lb_);
            channel(c + 1, qb_, kb_, lb_, qa_, ka_, la_);
        }
    }

    const int nv = min(32, C_out - 32 * og);  // outputs of this wave that exist (wave uniform)
    const int j = key - bos;
    if (j < 0 || j >= S) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = q0 + 4 * lq + r - bos;
        if (i < 0 || i >= S) continue;
        float* o = out + (((size_t)b * S + i) * S + j) * C_out + 32 * og;
        if ((C_out & 3) == 0) {  // 16-byte aligned rows
#pragma unroll
            for (int o4 = 0; o4 < 8; ++o4)
                if (4 * o4 < nv)
                    *reinterpret_cast<f32x4*>(o + 4 * o4) =
                        f32x4{acc[r][2 * o4][0], acc[r][2 * o4][1], acc[r][2 * o4 + 1][0], acc[r][2 * o4 + 1][1]};
        } else {
#pragma unroll
            for (int oo = 0; oo < 32; ++oo)
                if (oo < nv) o[oo] = acc[r][oo >> 1][oo & 1];
        }
    }
}

// In place on out [B,S,S,C_out] holding Z: element e = (b, i, j, o).  o >= n_sym: + bias.  o < n_sym: the thread of i <= j
// writes Z[i,j] + Z[j,i] + bias to both places (the same fp32 sum: addition commutes), the thread of i > j does nothing.
__global__ __launch_bounds__(256) void pair_head_final_kernel(float* __restrict__ out, const float* __restrict__ bias, int S,
                                                              int C_out, int n_sym, size_t total) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int o = (int)(e % C_out);
    size_t p = e / C_out;
    const int j = (int)(p % S);
    p /= S;
    const int i = (int)(p % S);
    const size_t b = p / S;
    const float bb = bias != nullptr ? bias[o] : 0.f;
    if (o >= n_sym) {
        out[e] += bb;
        return;
    }
    if (i > j) return;
    const size_t et = ((b * S + j) * S + i) * C_out + o;
    const float v = (out[e] + out[et]) + bb;
    out[e] = v;
    out[et] = v;
}

// w [C][C_out] -> w64 [C][64], zero beyond C_out
__global__ __launch_bounds__(256) void pair_head_pad_w_kernel(const float* __restrict__ w, float* __restrict__ w64, int C,
                                                              int C_out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)C * 64) return;
    const int o = (int)(e & 63);
    w64[e] = o < C_out ? w[(e >> 6) * C_out + o] : 0.f;
}

// The distogram term of one chain per workgroup (grid-stride over the chains), everything in fp64.  Element e = i * S + j of
// the chain counts when |i - j| >= min_sep and target[e] < n_bins (255 = ignore): term = -log(softmax(inv_temp * z)[target]
// + 1e-8), z = the n_bins logits at pair_logits[b,i,j,first ..] (utils/loss.py:10-29 with lm_design.py:254-280's mask: ALL
// ordered pairs that qualify).  Lane t adds the terms of e = t, t + 256, ... in that order; the 64 lane sums of a wavefront
// are added in a butterfly, the four wavefront sums in wavefront order: the order is a function of S, min_sep and the
// target alone.  energy = sum / count, 0.0 when count == 0.
__global__ __launch_bounds__(256) void distogram_energy_kernel(const float* __restrict__ logits, int ld, int first, int n_bins,
                                                               const unsigned char* __restrict__ target,
                                                               double* __restrict__ energy_out, int* __restrict__ count_out,
                                                               int B, int S, int min_sep, double inv_temp) {
    __shared__ double wave_sum[4];
    __shared__ int wave_count[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = S * S;  // S <= 32768
    for (int b = blockIdx.x; b < B; b += gridDim.x) {  // block uniform
        const float* z = logits + (size_t)b * (size_t)n * ld + first;
        double sum = 0.0;
        int count = 0;
        for (int e = tid; e < n; e += 256) {
            const int i = e / S, j = e - i * S;
            if (abs(i - j) < min_sep) continue;
            const int y = target[e];
            if (y >= n_bins) continue;
            const float* ze = z + (size_t)e * ld;
            double m = inv_temp * (double)ze[0];
            for (int t = 1; t < n_bins; ++t) m = fmax(m, inv_temp * (double)ze[t]);
            double den = 0.0;
            for (int t = 0; t < n_bins; ++t) den += exp(inv_temp * (double)ze[t] - m);
            const double pr = exp(inv_temp * (double)ze[y] - m) / den;
            sum += -log(pr + 1e-8);
            ++count;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sum += __shfl_xor(sum, o, 64);
            count += __shfl_xor(count, o, 64);
        }
        __syncthreads();  // the sums of the chain before this one have been read
        if (lane == 0) wave_sum[wave] = sum, wave_count[wave] = count;
        __syncthreads();
        if (tid == 0) {
            const double total = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
            const int cnt = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
            energy_out[b] = cnt > 0 ? total / (double)cnt : 0.0;
            count_out[b] = cnt;
        }
    }
}

template <typename T>
hipError_t launch_accum(int head_dim, unsigned grid, hipStream_t st, const void* q, const void* k, const float* lse,
                        const float* key_bias, const int64_t* tokens, const float* w64, float* out, int L, int B, int H, int T_,
                        int C_out, int bos, int S, int pad_idx) {
    if (head_dim == 128)
        hipLaunchKernelGGL((pair_head_accum_kernel<T, 128>), dim3(grid), dim3(512), 0, st, (const T*)q, (const T*)k, lse, key_bias,
                           tokens, w64, out, L, B, H, T_, C_out, bos, S, pad_idx);
    else
        hipLaunchKernelGGL((pair_head_accum_kernel<T, 64>), dim3(grid), dim3(512), 0, st, (const T*)q, (const T*)k, lse, key_bias,
                           tokens, w64, out, L, B, H, T_, C_out, bos, S, pad_idx);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_pair_head_pad_w(const float* w, float* w64, int C, int C_out, hipStream_t st) {
    if (!w || !w64 || C <= 0 || C_out <= 0 || C_out > 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pair_head_pad_w_kernel, dim3((unsigned)(((size_t)C * 64 + 255) / 256)), dim3(256), 0, st, w, w64, C, C_out);
    return hipGetLastError();
}

hipError_t launch_pair_head(const void* q, const void* k, const float* lse, const float* key_bias, const int64_t* tokens,
                            const float* w64, const float* bias, float* out, int L, int B, int H, int T, int head_dim, int n_sym,
                            int n_asym, int pad_idx, int prepend_bos, int append_eos, int operand_dtype, hipStream_t st) {
    const int bos = prepend_bos ? 1 : 0, eos = append_eos ? 1 : 0;
    const int S = T - bos - eos, C_out = n_sym + n_asym;
    if (!q || !k || !lse || !w64 || !out || L <= 0 || B <= 0 || H <= 0 || S <= 0 || n_sym < 0 || n_asym < 0 || C_out <= 0 ||
        C_out > 64 || (head_dim != 64 && head_dim != 128))
        return hipErrorInvalidValue;
    const long long nt = (T + 31) / 32, grid = (long long)B * nt * nt;
    const size_t total = (size_t)B * S * S * C_out;
    if (grid > 0x7fffffffLL || (total + 255) / 256 > 0x7fffffffULL) return hipErrorInvalidValue;
    hipError_t e = operand_dtype == ESMK_DT_BF16
                       ? launch_accum<__bf16>(head_dim, (unsigned)grid, st, q, k, lse, key_bias, tokens, w64, out, L, B, H, T, C_out,
                                              bos, S, pad_idx)
                       : launch_accum<_Float16>(head_dim, (unsigned)grid, st, q, k, lse, key_bias, tokens, w64, out, L, B, H, T,
                                                C_out, bos, S, pad_idx);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pair_head_final_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, out, bias, S, C_out, n_sym,
                       total);
    return hipGetLastError();
}

hipError_t launch_distogram_energy(const float* logits, int ld, int first, int n_bins, const unsigned char* target,
                                   double* energy_out, int* count_out, int B, int S, int min_sep, double inv_temp,
                                   hipStream_t st) {
    if (!logits || !target || !energy_out || !count_out || B <= 0 || S <= 0 || S > 32768 || min_sep < 0 || n_bins <= 0 ||
        n_bins > 255 || first < 0 || first + n_bins > ld)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(distogram_energy_kernel, dim3((unsigned)std::min(B, 8192)), dim3(256), 0, st, logits, ld, first, n_bins,
                       target, energy_out, count_out, B, S, min_sep, inv_temp);
    return hipGetLastError();
}

}  // namespace esmk
