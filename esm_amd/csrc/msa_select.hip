// msa_select.hip — choosing the rows of an MSA on the device (esm_amd/msa_select.py): Hamming mismatches between rows of a byte
// matrix, the neighbour counts behind sequence reweighting (the N^2 L hot path), the diversity-greedy row pick of the
// reference's contact notebook, and the exponential race that draws a weighted subsample.  An MSA is msa uint8 [N, ld],
// row-major; L <= ld columns count and every byte value 0 .. 255 is legal.  mism(i, j) = #{c < L : msa[i,c] != msa[j,c]}.
// Integer arithmetic and comparison logic only (the race keys are the one fp64 product), so every result is exact and none
// depends on the launch geometry.  The entries of the C ABI (include/esmk.h) are at the end of the file.
#include "common.h"
#include "engine_internal.h"
#include "philox.h"

#include <math.h>

#include <algorithm>

namespace esmk {
namespace {

// The number of non-zero bytes of x, for every byte value: bit 7 of a byte of t is set when its low seven bits are not all
// zero (the add carries into bit 7 and no further: 0x7f + 0x7f < 0x100), or-ing x adds the bytes whose only set bit is bit 7.
ESMK_DEV int nonzero_bytes(unsigned x) {
    const unsigned t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
    return __popc((t | x) & 0x80808080u);
}

// Columns c .. c + 3 of one row as a dword (column c in the low byte), columns at or past L as zero; c % 4 == 0.  ALIGNED: the
// matrix base and ld are multiples of 4, so the dword at c < L lies inside the row's ld bytes and is read whole, then masked.
// Otherwise the bytes below L are read one by one: nothing at or past column L is touched.
template <bool ALIGNED>
ESMK_DEV unsigned load_cols4(const unsigned char* __restrict__ row, int c, int L) {
    if (c >= L) return 0u;
    const int n = L - c;
    if (ALIGNED) {
        const unsigned v = *reinterpret_cast<const unsigned*>(row + c);
        return n >= 4 ? v : v & ((1u << (8 * n)) - 1u);
    }
    unsigned v = row[c];
    if (n > 1) v |= (unsigned)row[c + 1] << 8;
    if (n > 2) v |= (unsigned)row[c + 2] << 16;
    if (n > 3) v |= (unsigned)row[c + 3] << 24;
    return v;
}

// mism of two rows by one wavefront: lane l takes the columns 4 l .. 4 l + 3 of every 256, the 64 partial counts are added
// in a butterfly, so every lane returns the count.
template <bool ALIGNED>
ESMK_DEV int wave_mismatch(const unsigned char* __restrict__ ra, const unsigned char* __restrict__ rb, int L, int lane) {
    int m = 0;
    for (int c = lane * 4; c < L; c += 256) m += nonzero_bytes(load_cols4<ALIGNED>(ra, c, L) ^ load_cols4<ALIGNED>(rb, c, L));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
    return m;
}

// out[q, j] = mism(query[q], j): one wavefront per (q, j), grid-stride over the nq N pairs.  A query index outside [0, N) is
// clamped.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void mismatch_rows_kernel(const unsigned char* __restrict__ msa, int N, int L, int ld,
                                                            const int* __restrict__ query, int nq, int* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const size_t total = (size_t)nq * N, stride = (size_t)gridDim.x * 4;
    for (size_t p = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < total; p += stride) {  // wave uniform
        const int q = (int)(p / N), j = (int)(p % N);
        const int i = min(max(query[q], 0), N - 1);
        const int m = wave_mismatch<ALIGNED>(msa + (size_t)i * ld, msa + (size_t)j * ld, L, lane);
        if (lane == 0) out[p] = m;
    }
}

// Neighbour counts: count[i] += #{j in the workgroup's column tiles : mism(i, j) <= max_mismatch}.
//   tile    a workgroup owns the 64 rows i0 .. i0 + 63 and the 64-row column tiles blockIdx.y, blockIdx.y + gridDim.y, ...;
//           every (i, j) pair is computed once from each side (tile (I, J) and tile (J, I) are different workgroups), so a row's
//           count is the sum over its own workgroups and needs no credit to the other row: one integer atomic add per row and
//           workgroup at the very end, 64 gridDim.y per row tile, instead of 64 per tile pair
//   lanes   thread (ti, tj) = (tid / 16, tid % 16) owns the 4 x 4 pairs (i0 + 4 ti + r, j0 + 4 tj + c) and keeps their 16 mismatch
//           counts in registers
//   LDS     the columns go through LDS in chunks of 128 (32 dwords): sa / sb [dword k][row], row stride 68 dwords, so a thread
//           reads the dword k of its four rows with one 16-byte read (the 16 tj of a wavefront read 256 contiguous bytes, the
//           four ti are broadcasts), and the staging store of dword k of row r goes to bank (4 k + r) % 32
//   tail    columns at or past L are staged as zero on both sides: they never differ.  Rows at or past N are staged as zero
//           and never counted (j) or written (i)
// A dword pair costs xor, and, add, or, and, popcount-accumulate: 6 VALU operations per four columns per pair.
constexpr int kTile = 64, kChunk = 32, kStride = kTile + 4;

template <bool ALIGNED>
__global__ __launch_bounds__(256) void neighbor_counts_kernel(const unsigned char* __restrict__ msa, int N, int L, int ld,
                                                              int max_mismatch, int* __restrict__ count_out, int n_jt) {
    __shared__ __attribute__((aligned(16))) unsigned sa[kChunk * kStride];
    __shared__ __attribute__((aligned(16))) unsigned sb[kChunk * kStride];
    const int tid = threadIdx.x, lane = tid & 63;
    const int ti = (tid >> 6) * 4 + (lane >> 4), tj = lane & 15;
    const int i0 = blockIdx.x * kTile;
    const int n_dw = (L + 3) >> 2;
    const int sk = tid & 31, sr = tid >> 5;  // staging: dword sk of the rows sr, sr + 8, ... of the tile
    int cnt[4] = {0, 0, 0, 0};
    for (int jt = blockIdx.y; jt < n_jt; jt += gridDim.y) {  // block uniform
        const int j0 = jt * kTile;
        int acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = 0;
        for (int k0 = 0; k0 < n_dw; k0 += kChunk) {
            const int kc = min(kChunk, n_dw - k0);
            __syncthreads();  // the chunk before this one has been read by everyone
            if (sk < kc) {
                const int col = (k0 + sk) * 4;
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    const int r = p * 8 + sr;
                    const int ia = i0 + r, jb = j0 + r;
                    sa[sk * kStride + r] = ia < N ? load_cols4<ALIGNED>(msa + (size_t)ia * ld, col, L) : 0u;
                    sb[sk * kStride + r] = jb < N ? load_cols4<ALIGNED>(msa + (size_t)jb * ld, col, L) : 0u;
                }
            }
            __syncthreads();
            for (int k = 0; k < kc; ++k) {
                const uint4 a4 = *reinterpret_cast<const uint4*>(&sa[k * kStride + ti * 4]);
                const uint4 b4 = *reinterpret_cast<const uint4*>(&sb[k * kStride + tj * 4]);
                const unsigned a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[r][c] += nonzero_bytes(a[r] ^ b[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const bool live = j0 + tj * 4 + c < N;
#pragma unroll
            for (int r = 0; r < 4; ++r) cnt[r] += (live && acc[r][c] <= max_mismatch) ? 1 : 0;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        int v = cnt[r];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);  // the 16 tj of one ti are 16 neighbouring lanes
        const int i = i0 + ti * 4 + r;
        if (tj == 0 && i < N && v != 0) atomicAdd(&count_out[i], v);
    }
}

// The greedy pick, one step at a time.  sum[j] holds S_k[j] for the rows not yet selected and -1 for the selected ones (the
// sums are never negative: num L < 2^31).
__global__ __launch_bounds__(256) void greedy_init_kernel(int* __restrict__ sum, int* __restrict__ sel, int N, int first) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < (size_t)N; j += stride) sum[j] = (int)j == first ? -1 : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) sel[0] = first;
}

// sum[j] += mism(*prev, j) for every row not yet selected: one wavefront per row.  *prev is the pick of the step before, read
// on the device (clamped to [0, N): it always is inside).
template <bool ALIGNED>
__global__ __launch_bounds__(256) void greedy_accumulate_kernel(const unsigned char* __restrict__ msa, int N, int L, int ld,
                                                                const int* __restrict__ prev, int* __restrict__ sum) {
    const int lane = threadIdx.x & 63;
    const int i = min(max(*prev, 0), N - 1);
    const size_t stride = (size_t)gridDim.x * 4;
    for (size_t j = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < (size_t)N; j += stride) {  // wave uniform
        const int s = sum[j];
        if (s < 0) continue;
        const int m = wave_mismatch<ALIGNED>(msa + (size_t)i * ld, msa + j * ld, L, lane);
        if (lane == 0) sum[j] = s + m;
    }
}

// *pick = the row not yet selected with the largest (mode 0) or smallest (mode 1) sum, ties to the lowest row; its sum becomes
// -1.  One workgroup of 1024 threads: thread t scans the rows t, t + 1024, ... in ascending order and keeps the first best, the
// 1024 candidates are reduced by (key, row) through shuffles and LDS.  key = sum (mode 0) or -sum (mode 1): larger is better.
ESMK_DEV bool pick_better(int ka, int ja, int kb, int jb) {  // candidate a beats b; row -1: no candidate
    if (ja < 0) return false;
    if (jb < 0) return true;
    return ka > kb || (ka == kb && ja < jb);
}

__global__ __launch_bounds__(1024) void greedy_pick_kernel(int* __restrict__ sum, int* __restrict__ pick, int N, int mode) {
    __shared__ int wkey[16], wrow[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bk = 0, bj = -1;
    for (int j = tid; j < N; j += 1024) {
        const int s = sum[j];
        if (s < 0) continue;
        const int k = mode ? -s : s;
        if (bj < 0 || k > bk) bk = k, bj = j;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int ok = __shfl_xor(bk, o, 64), oj = __shfl_xor(bj, o, 64);
        if (pick_better(ok, oj, bk, bj)) bk = ok, bj = oj;
    }
    if (lane == 0) wkey[wave] = bk, wrow[wave] = bj;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (pick_better(wkey[w], wrow[w], bk, bj)) bk = wkey[w], bj = wrow[w];
        if (bj >= 0) {  // num <= N: a row is always left
            *pick = bj;
            sum[bj] = -1;
        }
    }
}

// key[i] = -log(u_i) * count[i] in fp64, u_i = (word0 >> 8) * 2^-24 at counter (subsample, 0, 2, i) under the key seed; a null
// count is all ones; u_i == 0 or count[i] <= 0: +inf.  The smallest keys are a weighted draw without replacement with
// weights 1 / count (an exponential race).
__global__ __launch_bounds__(256) void race_keys_kernel(const int* __restrict__ count, int N, unsigned long long seed,
                                                        int subsample, double* __restrict__ key) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)N; i += stride) {
        const double u = (double)(philox_word0(seed, subsample, 0, kPurposeRace, (int)i) >> 8) * 0x1p-24;
        const int c = count != nullptr ? count[i] : 1;
        key[i] = (u == 0.0 || c <= 0) ? (double)INFINITY : -log(u) * (double)c;
    }
}

// a ranks before b in ascending order of fp64 keys: the smaller key first, equal keys by the lower index, NaN behind
// everything (+inf included), among NaNs the lower index first.  A total order on (key, index).
ESMK_DEV bool key_before(double a, int ia, double b, int ib) {
    if (a != a) return b != b && ia < ib;
    if (b != b) return true;
    return a < b || (a == b && ia < ib);
}

// rank[i] = the number of keys that rank before key i: one thread per i, the keys pass through LDS in tiles of 256 (every
// thread reads the same key at the same time: a broadcast).  N^2 comparisons, no sort, no scratch.
__global__ __launch_bounds__(256) void rank_keys_kernel(const double* __restrict__ key, int* __restrict__ rank, int N) {
    __shared__ double tile[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const double ki = i < N ? key[i] : 0.0;
    int r = 0;
    for (int j0 = 0; j0 < N; j0 += 256) {  // block uniform
        __syncthreads();
        const int j = j0 + threadIdx.x;
        tile[threadIdx.x] = j < N ? key[j] : 0.0;
        __syncthreads();
        const int n = min(256, N - j0);
        for (int t = 0; t < n; ++t) r += key_before(tile[t], j0 + t, ki, i) ? 1 : 0;
    }
    if (i < N) rank[i] = r;
}

bool dword_rows(const void* msa, int ld) { return ld % 4 == 0 && (uintptr_t)msa % 4 == 0; }

unsigned wave_blocks(size_t waves) { return (unsigned)std::min<size_t>((waves + 3) / 4, 16384); }

}  // namespace
}  // namespace esmk

using namespace esmk;
using namespace esmk_host;

namespace {
// the checks every entry on an MSA shares; 0 when the matrix is acceptable
int bad_msa(const std::string& w, const void* msa, int N, int L, int ld) {
    if (!msa) return fail(w + ": null argument");
    if (N <= 0 || L <= 0) return fail(w + ": N and L must be positive");
    if (ld < L) return fail(w + ": ld must not be smaller than L");
    if ((long long)N * ld >= (1LL << 31)) return fail(w + ": N * ld must be below 2^31");
    if (L > 65535) return fail(w + ": L must not exceed 65535");
    return 0;
}
}  // namespace

extern "C" {

int esmk_op_msa_mismatch_rows(const uint8_t* msa_dev, int N, int L, int ld, const int32_t* query_dev, int nq, int32_t* out_dev,
                              void* stream) {
    const char* w = "esmk_op_msa_mismatch_rows";
    if (!query_dev || !out_dev) return fail(std::string(w) + ": null argument");
    if (int rc = bad_msa(w, msa_dev, N, L, ld)) return rc;
    if (nq <= 0) return fail(std::string(w) + ": nq must be positive");
    if ((long long)nq * N >= (1LL << 31)) return fail(std::string(w) + ": nq * N must be below 2^31");
    const unsigned blocks = wave_blocks((size_t)nq * N);
    if (dword_rows(msa_dev, ld))
        hipLaunchKernelGGL(mismatch_rows_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, msa_dev, N, L, ld,
                           query_dev, nq, out_dev);
    else
        hipLaunchKernelGGL(mismatch_rows_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, msa_dev, N, L, ld,
                           query_dev, nq, out_dev);
    ESMK_TRY(hipGetLastError());
    return 0;
}

int esmk_op_msa_neighbor_counts(const uint8_t* msa_dev, int N, int L, int ld, int max_mismatch, int32_t* count_out_dev,
                                void* stream) {
    const char* w = "esmk_op_msa_neighbor_counts";
    if (!count_out_dev) return fail(std::string(w) + ": null argument");
    if (int rc = bad_msa(w, msa_dev, N, L, ld)) return rc;
    hipStream_t st = (hipStream_t)stream;
    ESMK_TRY(hipMemsetAsync(count_out_dev, 0, (size_t)N * sizeof(int32_t), st));
    if (max_mismatch < 0) return 0;  // no pair is that close, not even (i, i)
    // enough workgroups to fill the device whatever N is: the column tiles of a row tile are dealt to gridDim.y workgroups
    const int n_t = (N + kTile - 1) / kTile;
    const int split = std::min(n_t, std::max(1, (4096 + n_t - 1) / n_t));
    const dim3 grid((unsigned)n_t, (unsigned)split);
    if (dword_rows(msa_dev, ld))
        hipLaunchKernelGGL(neighbor_counts_kernel<true>, grid, dim3(256), 0, st, msa_dev, N, L, ld, max_mismatch, count_out_dev,
                           n_t);
    else
        hipLaunchKernelGGL(neighbor_counts_kernel<false>, grid, dim3(256), 0, st, msa_dev, N, L, ld, max_mismatch, count_out_dev,
                           n_t);
    ESMK_TRY(hipGetLastError());
    return 0;
}

int esmk_op_msa_greedy_select(const uint8_t* msa_dev, int N, int L, int ld, int first, int num, int mode, int32_t* sum_work_dev,
                              int32_t* sel_out_dev, void* stream) {
    const char* w = "esmk_op_msa_greedy_select";
    if (!sum_work_dev || !sel_out_dev) return fail(std::string(w) + ": null argument");
    if (int rc = bad_msa(w, msa_dev, N, L, ld)) return rc;
    if (num < 1 || num > N) return fail(std::string(w) + ": num must be in 1 .. N");
    if (first < 0 || first >= N) return fail(std::string(w) + ": first must be in [0, N)");
    if ((long long)num * L >= (1LL << 31)) return fail(std::string(w) + ": num * L must be below 2^31");
    if (mode < 0 || mode > 1) return fail(std::string(w) + ": mode must be 0 (largest sum) or 1 (smallest sum)");
    hipStream_t st = (hipStream_t)stream;
    const bool aligned = dword_rows(msa_dev, ld);
    const unsigned blocks = wave_blocks((size_t)N);
    hipLaunchKernelGGL(greedy_init_kernel, dim3((unsigned)std::min((N + 255) / 256, 8192)), dim3(256), 0, st, sum_work_dev,
                       sel_out_dev, N, first);
    ESMK_TRY(hipGetLastError());
    for (int k = 1; k < num; ++k) {  // back to back on the stream: step k reads sel[k - 1] on the device
        if (aligned)
            hipLaunchKernelGGL(greedy_accumulate_kernel<true>, dim3(blocks), dim3(256), 0, st, msa_dev, N, L, ld,
                               sel_out_dev + (k - 1), sum_work_dev);
        else
            hipLaunchKernelGGL(greedy_accumulate_kernel<false>, dim3(blocks), dim3(256), 0, st, msa_dev, N, L, ld,
                               sel_out_dev + (k - 1), sum_work_dev);
        hipLaunchKernelGGL(greedy_pick_kernel, dim3(1), dim3(1024), 0, st, sum_work_dev, sel_out_dev + k, N, mode);
        ESMK_TRY(hipGetLastError());
    }
    return 0;
}

int esmk_op_msa_race_keys(const int32_t* count_dev, int N, uint64_t seed, int subsample, double* key_out_dev, void* stream) {
    if (!key_out_dev) return fail("esmk_op_msa_race_keys: null argument");
    if (N <= 0 || N > ESMK_MAX_ROWS) return fail("esmk_op_msa_race_keys: N must be in 1 .. 2^24");
    if (subsample < 0) return fail("esmk_op_msa_race_keys: subsample must not be negative");
    hipLaunchKernelGGL(race_keys_kernel, dim3((unsigned)std::min((N + 255) / 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                       count_dev, N, (unsigned long long)seed, subsample, key_out_dev);
    ESMK_TRY(hipGetLastError());
    return 0;
}

int esmk_op_rank_keys(const double* key_dev, int32_t* rank_out_dev, int N, void* stream) {
    if (!key_dev || !rank_out_dev) return fail("esmk_op_rank_keys: null argument");
    if (N <= 0 || N > ESMK_MAX_ROWS) return fail("esmk_op_rank_keys: N must be in 1 .. 2^24");
    hipLaunchKernelGGL(rank_keys_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, key_dev,
                       rank_out_dev, N);
    ESMK_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
