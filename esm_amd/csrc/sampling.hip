// sampling.hip — drawing sequences from the model on the device (esm_amd/sampling.py: Gibbs sweeps, mask in-painting): a
// counter-addressed random number generator, the per-chain shuffle of the designable positions, the draw of one token from
// a row of log-probabilities and the write-back into the token matrix.  None of them is a hot loop: the layer stack in
// front of every draw is the time.  A sampling step is mask (esmk_op_mask_rows_multi) -> esmk_forward_rows -> draw -> commit
// on one stream, and every random number is addressed by (seed, chain id, epoch or step, purpose, index): it depends on
// nothing else, so a chain draws the same tokens alone, in a batch, and in any launch geometry.  Confidence-ordered unmasking
// (inpaint(order=...)) replaces the shuffle by a score per row and a per-chain choice of the best rows: esmk_forward_rows on
// every remaining <mask> row -> sample_rows_kernel (top-k / nucleus filter, draw, score) -> select_rows_kernel -> commit.
#include "common.h"
#include "kernels.h"
#include "philox.h"
#include <algorithm>

namespace esmk {

// perm_out[lo : hi] = a Fisher-Yates shuffle of pos_in[lo : hi], (lo, hi) = pos_off[c], pos_off[c + 1]: for i = len - 1 .. 1,
// j = mulhi32(word0(chain_id[c], epoch, 0, i), i + 1), swap elements i and j.  One lane per chain runs the loop (a list is at
// most T long), so the order of the swaps is fixed; the slices are disjoint, so no two lanes write the same element.  Integer
// arithmetic only.  The offsets are device data: clamped to [0, total], a pair with hi < lo is an empty list.
__global__ __launch_bounds__(256) void permute_positions_kernel(const int* __restrict__ pos_off, const int* __restrict__ pos_in,
                                                                const int* __restrict__ chain_id, int* __restrict__ perm_out,
                                                                int n_chain, int total, unsigned long long seed, int epoch) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t c = (size_t)blockIdx.x * 256 + threadIdx.x; c < (size_t)n_chain; c += stride) {
        const int lo = min(max(pos_off[c], 0), total), hi = min(max(pos_off[c + 1], 0), total);
        const int len = hi - lo;
        if (len <= 0) continue;
        const int chain = chain_id[c];
        int* p = perm_out + lo;
        for (int i = 0; i < len; ++i) p[i] = pos_in[lo + i];
        for (int i = len - 1; i >= 1; --i) {
            const int j = (int)__umulhi(philox_word0(seed, chain, epoch, kPurposePermutation, i), (unsigned)(i + 1));  // 0 .. i
            const int a = p[i], b = p[j];
            p[i] = b;
            p[j] = a;
        }
    }
}

hipError_t launch_permute_positions(const int* pos_off, const int* pos_in, const int* chain_id, int* perm_out, int n_chain,
                                    int total, unsigned long long seed, int epoch, hipStream_t st) {
    if (!pos_off || !pos_in || !chain_id || !perm_out || n_chain <= 0 || total <= 0) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)std::min<size_t>(((size_t)n_chain + 255) / 256, 8192);
    hipLaunchKernelGGL(permute_positions_kernel, dim3(blocks), dim3(256), 0, st, pos_off, pos_in, chain_id, perm_out, n_chain,
                       total, seed, epoch);
    return hipGetLastError();
}

// v ranks before w in a best-first order of fp32 values: the larger value first, equal values by the lower index, NaN behind
// everything (-inf included), among NaNs the lower index first.  Comparison logic only: a total order on (value, index).
__device__ inline bool ranks_before(float xv, int v, float xw, int w) {
    if (xv != xv) return xw != xw && v < w;
    if (xw != xw) return true;
    return xv > xw || (xv == xw && v < w);
}

// One token per row of log-probabilities [n, V], V <= 64: one wavefront per row, one vocabulary entry per lane.  The one
// statement of the draw: esmk_op_sample_rows is this kernel with both filters off and no score, esmk_op_sample_rows_ex all of it.
//   u      = (word0(row_chain[i], step, 1, row_index[i]) >> 8) * 2^-24: exact in fp32, in [0, 1)
//   cand   = the bits of allowed_mask below V, minus the token exclude[i] (when that is inside [0, V))
//   z_v    = lp[v] * inv_temperature (greedy, inv_temperature == 0: lp[v]), m = max over cand of z, w_v = expf(z_v - m) on cand
//          (0 elsewhere); expf is the precise one
//   rank   of candidate v = the number of candidates that rank before it by the fp32 INPUT lp (ranks_before; inv_temperature
//          > 0, so that is the order of the tempered values): every lane counts over a shuffle of the 64 lanes
//   E_r    = the fp32 sum of the weights of the ranks before r, added in rank order: the wave walks the ranks 0, 1, ... (the
//          lane holding rank r is found by a ballot, its weight broadcast) and every lane adds the ones before its own rank;
//          W = the same sum over all candidates
//   kept   = rank 0, and every rank r with (top_k == 0 || r < top_k) && (top_p >= 1 || E_r < top_p * W).  Both filters off
//          (top_k == 0, top_p == 1): kept = cand without any of this arithmetic
//   draw   (inv_temperature > 0) over the kept set: the running sum c_v = w_0 + ... + w_v is added in fp32 in ascending token
//          order — every lane walks the lanes 0 .. 63 through a shuffle and adds the ones at or below itself, so lane v holds
//          exactly the sequential sum and the last lane the total; token = the first kept token with c_v > u * total, the last
//          kept one if there is none; logq = z_tok - m - log(total) relative to the kept set, taken in fp64 from the fp32
//          inputs and rounded to fp32 once
//   greedy (inv_temperature == 0): the argmax of lp over cand, ties to the lowest index, whatever the filters say (it is rank
//          0: always kept); logq = 0; kept and score are computed with z = lp
//   score  over cand, before filtering, in fp64 from the fp32 inputs, rounded to fp32 once: kind 1 = max log q = -log(sum of
//          exp(z - m)), kind 2 = sum of q log q (terms with q == 0 count as 0), q = softmax(z); cand empty: -inf
//   cand empty: token = -1, logq = 0
//   every candidate at -inf (no log_softmax of finite logits gives that): m = -inf, every w is NaN, no running sum exceeds
//          the threshold: token = the last kept candidate, logq = NaN; kept = rank 0 alone when top_p < 1 (no comparison with
//          NaN holds).  Greedy takes the lowest candidate (all tie at -inf).
// Nothing depends on the row's place in the launch.  EX = false leaves the filters, the score and the kept set out of the
// compiled code (the launcher takes it when none of them is asked for): the same statements, so the same bits.
template <bool EX>
__global__ __launch_bounds__(256) void sample_rows_kernel(const float* __restrict__ lp, const int* __restrict__ row_chain,
                                                          const int* __restrict__ row_index, const int* __restrict__ exclude,
                                                          unsigned long long allowed, float inv_temperature,
                                                          unsigned long long seed, int step, int top_k, float top_p,
                                                          int score_kind, int* __restrict__ token_out,
                                                          float* __restrict__ logq_out, float* __restrict__ u_out,
                                                          float* __restrict__ score_out,
                                                          unsigned long long* __restrict__ kept_out, int n, int V) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;  // wave uniform
    const float u = (float)(philox_word0(seed, row_chain[row], step, kPurposeToken, row_index[row]) >> 8) * 0x1p-24f;
    unsigned long long cand = V < 64 ? allowed & ((1ull << V) - 1) : allowed;
    if (exclude != nullptr) {
        const int ex = exclude[row];
        if (ex >= 0 && ex < V) cand &= ~(1ull << ex);
    }
    const bool mine = (cand >> lane) & 1ull;  // lanes at or past V never are
    const float x = mine ? lp[(size_t)row * V + lane] : -INFINITY;
    const float scale = inv_temperature > 0.f ? inv_temperature : 1.f;
    int token = -1;
    float logq = 0.f, score = -INFINITY;
    unsigned long long kept = cand;
    if (cand != 0ull) {  // wave uniform
        const float z = inv_temperature > 0.f ? x * inv_temperature : x;  // (-inf stays -inf: inv_temperature > 0)
        float m = z;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        const float w = mine ? expf(z - m) : 0.f;
        if (EX && (top_k != 0 || top_p < 1.f)) {  // wave uniform
            int rank = 0;
            for (int v = 0; v < V; ++v) {
                const float xv = __shfl(x, v, 64);
                if (((cand >> v) & 1ull) && ranks_before(xv, v, x, lane)) ++rank;
            }
            const int n_cand = __popcll(cand);
            float before = 0.f, all = 0.f;  // E of this lane's rank; W
            for (int r = 0; r < n_cand; ++r) {  // rank order, the same additions in every lane up to its own rank
                const unsigned long long at = __ballot(mine && rank == r);  // exactly one lane: the order is total
                const float wr = __shfl(w, __ffsll((long long)at) - 1, 64);
                if (r < rank) before += wr;
                all += wr;
            }
            const bool keep = mine && (rank == 0 || ((top_k == 0 || rank < top_k) && (top_p >= 1.f || before < top_p * all)));
            kept = __ballot(keep);
        }
        const bool held = (kept >> lane) & 1ull;
        if (inv_temperature > 0.f) {
            const float wk = held ? w : 0.f;
            float cum = 0.f;
            for (int v = 0; v < V; ++v) {  // ascending token order, the same additions in every lane up to its own entry
                const float wv = __shfl(wk, v, 64);
                if (v <= lane) cum += wv;
            }
            const float total = __shfl(cum, V - 1, 64);
            const float thr = u * total;
            const unsigned long long over = __ballot(held && cum > thr);
            token = over != 0ull ? __ffsll((long long)over) - 1 : 63 - __clzll((long long)kept);
            // logq in fp64 from the fp32 inputs, rounded once: the fp32 chain z_tok - m - logf(total) lost up to 1.2 ulp of the
            // result (5.6e-7 at logq = -4.9).  Butterfly reductions: every lane ends with the same bits.
            const double zd = held ? (double)x * (double)inv_temperature : -INFINITY;
            double md = zd;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) md = fmax(md, __shfl_xor(md, o, 64));
            double sd = held ? exp(zd - md) : 0.0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sd += __shfl_xor(sd, o, 64);
            logq = (float)(__shfl(zd, token, 64) - md - log(sd));
        } else {
            const unsigned long long top = __ballot(mine && x == m);  // (a row of NaNs only: no lane; the last candidate)
            token = top != 0ull ? __ffsll((long long)top) - 1 : 63 - __clzll((long long)cand);
        }
        if (EX && score_kind != 0) {  // butterfly reductions: every lane ends with the same bits
            const double zd = mine ? (double)x * (double)scale : -INFINITY;
            double md = zd;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) md = fmax(md, __shfl_xor(md, o, 64));
            const double ed = mine ? exp(zd - md) : 0.0;
            double sd = ed;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sd += __shfl_xor(sd, o, 64);
            const double ls = log(sd);
            if (score_kind == 1) {
                score = (float)(-ls);
            } else {
                const double q = ed / sd;
                double h = (mine && q > 0.0) ? q * (zd - md - ls) : 0.0;
                if (mine && q != q) h = q;  // a row without a distribution: NaN, as logq
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o, 64);
                score = (float)h;
            }
        }
    }
    if (lane == 0) {
        token_out[row] = token;
        logq_out[row] = logq;
        if (u_out != nullptr) u_out[row] = u;
        if (EX && score_out != nullptr && score_kind != 0) score_out[row] = score;
        if (EX && kept_out != nullptr) kept_out[row] = kept;
    }
}

hipError_t launch_sample_rows(const float* lp, const int* row_chain, const int* row_index, const int* exclude,
                              unsigned long long allowed, float inv_temperature, unsigned long long seed, int step, int top_k,
                              float top_p, int score_kind, int* token_out, float* logq_out, float* u_out, float* score_out,
                              unsigned long long* kept_out, int n, int V, hipStream_t st) {
    if (!lp || !row_chain || !row_index || !token_out || !logq_out || n <= 0 || V <= 0 || V > 64 || !(inv_temperature >= 0.f) ||
        top_k < 0 || top_k > 64 || !(top_p > 0.f && top_p <= 1.f) || score_kind < 0 || score_kind > 2 ||
        (score_kind != 0 && !score_out))
        return hipErrorInvalidValue;
    const bool ex = top_k != 0 || top_p < 1.f || score_kind != 0 || kept_out != nullptr;
    hipLaunchKernelGGL(ex ? sample_rows_kernel<true> : sample_rows_kernel<false>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, lp,
                       row_chain, row_index, exclude, allowed, inv_temperature, seed, step, top_k, top_p, score_kind, token_out,
                       logq_out, u_out, score_out, kept_out, n, V);
    return hipGetLastError();
}

// Per chain c (rows [row_off[c], row_off[c+1]) of score, offsets clamped to [0, n], hi < lo: empty) the k_c = clamp(sel_off[c+1] -
// sel_off[c], 0, len_c) rows with the largest score, best first (ranks_before: ties to the lower row, NaN below everything),
// as row indices into sel_out[sel_off[c] ..]; the other rows of the chain in ascending row order into rest_out[rest_off[c] ..],
// at most rest_off[c+1] - rest_off[c] of them.  One workgroup per chain, grid-stride over the chains.
//   pass 1  every thread counts, for each of its rows, the rows of the chain that rank before it (rank counting: len^2 / 256
//           comparisons per thread, no sort, no scratch; every thread reads the same score at the same time); a row of rank
//           r < k_c is written to sel_out[sel_off[c] + r], and the row of rank k_c - 1 leaves its (score, row) in LDS
//   pass 2  a row is selected exactly when it does not rank behind that threshold row, so the rest list is an ordered
//           compaction of a pure comparison: tiles of 256 rows in ascending order, a ballot per wavefront, the four
//           wavefront counts and the running base through LDS
// Comparison logic and integer arithmetic only; no atomics; nothing outside the slices is written, and no element outside
// [0, n_sel) / [0, n_rest) whatever the offsets hold.
__global__ __launch_bounds__(256) void select_rows_kernel(const float* __restrict__ score, const int* __restrict__ row_off,
                                                          const int* __restrict__ sel_off, const int* __restrict__ rest_off,
                                                          int* __restrict__ sel_out, int* __restrict__ rest_out, int n_chain,
                                                          int n, int n_sel, int n_rest) {
    __shared__ float thr_score;
    __shared__ int thr_row;
    __shared__ int wave_count[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int c = blockIdx.x; c < n_chain; c += gridDim.x) {  // block uniform
        __syncthreads();  // thr_* of the chain before this one has been read by everyone
        const int lo = min(max(row_off[c], 0), n), hi = min(max(row_off[c + 1], 0), n);
        const int len = max(hi - lo, 0);
        if (len == 0) continue;
        const long long s0 = sel_off[c];
        const int k = (int)min(max((long long)sel_off[c + 1] - s0, 0ll), (long long)len);
        for (int i = tid; i < len; i += 256) {
            const float xi = score[lo + i];
            int rank = 0;
            for (int j = 0; j < len; ++j) rank += ranks_before(score[lo + j], j, xi, i) ? 1 : 0;
            if (rank < k) {
                const long long at = s0 + rank;
                if (at >= 0 && at < (long long)n_sel) sel_out[at] = lo + i;
                if (rank == k - 1) thr_score = xi, thr_row = i;
            }
        }
        if (n_rest <= 0 || len == k) continue;  // block uniform: no rest list, or nothing left for it
        __syncthreads();
        const float ts = k > 0 ? thr_score : 0.f;
        const int tr = k > 0 ? thr_row : 0;
        const long long r0 = rest_off[c];
        const long long room = (long long)rest_off[c + 1] - r0;
        int base = 0;  // rows of the rest list in front of this tile (block uniform)
        for (int t0 = 0; t0 < len; t0 += 256) {
            const int i = t0 + tid;
            const bool left = i < len && k > 0 ? ranks_before(ts, tr, score[lo + i], i) : i < len;  // behind the threshold row
            const unsigned long long b = __ballot(left);
            if (lane == 0) wave_count[wave] = __popcll(b);
            __syncthreads();
            int at = base + __popcll(b & ((1ull << lane) - 1));
            for (int q = 0; q < wave; ++q) at += wave_count[q];
            if (left && at < room) {
                const long long dst = r0 + at;
                if (dst >= 0 && dst < (long long)n_rest) rest_out[dst] = lo + i;
            }
            base += wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
            __syncthreads();  // wave_count is rewritten by the next tile
        }
    }
}

hipError_t launch_select_rows(const float* score, const int* row_off, const int* sel_off, const int* rest_off, int* sel_out,
                              int* rest_out, int n_chain, int n, int n_sel, int n_rest, hipStream_t st) {
    if (!score || !row_off || !sel_off || !sel_out || n_chain <= 0 || n <= 0 || n_sel <= 0 || n_rest < 0 ||
        (n_rest > 0 && (!rest_off || !rest_out)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(select_rows_kernel, dim3((unsigned)std::min(n_chain, 8192)), dim3(256), 0, st, score, row_off, sel_off,
                       rest_off, sel_out, rest_out, n_chain, n, n_sel, n_rest);
    return hipGetLastError();
}

// tokens[slot[i], pos[i]] = token[i] on int64 [B, T]: the write-back of a sampling step.  A row with token < 0 (an empty
// candidate set) or a position outside [0, T) writes nothing; a slot outside [0, B) is clamped.  The (slot, pos) pairs of a
// call are distinct by contract, so no two lanes write the same element.
__global__ __launch_bounds__(256) void commit_tokens_kernel(int64_t* __restrict__ tokens, const int* __restrict__ slot,
                                                            const int* __restrict__ pos, const int* __restrict__ token, int n,
                                                            int B, int T) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += stride) {
        const int t = token[i], p = pos[i];
        if (t < 0 || p < 0 || p >= T) continue;
        const int b = min(max(slot[i], 0), B - 1);
        tokens[(size_t)b * T + p] = (int64_t)t;
    }
}

hipError_t launch_commit_tokens(int64_t* tokens, const int* slot, const int* pos, const int* token, int n, int B, int T,
                                hipStream_t st) {
    if (!tokens || !slot || !pos || !token || n <= 0 || B <= 0 || T <= 0) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)std::min<size_t>(((size_t)n + 255) / 256, 8192);
    hipLaunchKernelGGL(commit_tokens_kernel, dim3(blocks), dim3(256), 0, st, tokens, slot, pos, token, n, B, T);
    return hipGetLastError();
}

}  // namespace esmk
