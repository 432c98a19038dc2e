// msa_build.hip — from search hits to a query-anchored MSA on the device (esm_amd/msa_build.py).
//
// The aligner leaves, per hit, the alignment columns (i, j) against the query; the two kernels here make an alignment of them
// and measure it:
//     msa_project_kernel        per hit: the path's match columns written into a row of Lq bytes, and six integers about the path
//     msa_pair_identity_kernel  per pair of rows: the share of identical bytes among the columns in which neither row has a gap
// Integer and comparison logic only (the one float operation is a correctly rounded division of two exact integers), no
// atomics, no scratch memory: a workgroup owns what it writes, and every result is the same bits whatever the launch geometry.
// Offsets, lengths and path columns are device data: each is clamped to what its buffer holds or ignored.
#include "common.h"
#include "engine_internal.h"

#include <algorithm>
#include <string>

using namespace esmk;
using namespace esmk_host;

namespace {

// ---- projection ---------------------------------------------------------------------------------------------------------
constexpr int kProjThreads = 256;
constexpr int kProjWaves = kProjThreads / 64;
constexpr int kProjMaxLq = 8192;  // the aligner's longest sequence; a wavefront's row of LDS
constexpr int kStats = 6;

struct ProjectArgs {
    const int* cols;  // [n_cols_total, 2]
    long long n_cols_total;
    const long long* col_offsets;  // [P + 1], into cols
    int P;
    const unsigned char* seqs;  // [n_bytes]
    long long n_bytes;
    const long long* seq_off;  // [P]
    const int* seq_len;        // [P]
    const unsigned char* query;  // [Lq]
    int Lq;
    unsigned char* msa;  // [P, ld]
    int ld;
    int* stats;  // [P, 6]
};

// One wavefront per hit, four hits per workgroup and round; the rounds are uniform over the workgroup (a wavefront without a
// hit takes part in the barriers and does nothing else).  A wavefront builds its row in LDS: a fill of '-' (zero from Lq to
// the next multiple of 4), the match letters scattered over it, the whole written out as dwords; columns Lq rounded up .. ld - 1
// are written as zero dwords.  A path column is
//     a match      0 <= i < Lq and 0 <= j < len        the letter seqs[off + j] lands in column i
//     a deletion   0 <= i < Lq and j == -1
//     an insertion i == -1 and 0 <= j < len
// and anything else is ignored; len is seq_len[p] clamped to the bytes the blob holds behind seq_off[p] (0 when seq_off[p] is
// outside the blob), and the path's range col_offsets[p] .. col_offsets[p + 1] is clamped into [0, n_cols_total], its end to no
// less than its start.  Pass 1 finds the path positions of the first and the last match (min / max butterflies), pass 2
// writes the letters and counts; "strictly inside" compares path positions.
__global__ __launch_bounds__(kProjThreads) void msa_project_kernel(const ProjectArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char s_row[kProjWaves][kProjMaxLq];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned char* row_lds = s_row[wave];
    const int lq_dw = (a.Lq + 3) >> 2, ld_dw = a.ld >> 2;
    const unsigned gaps = 0x2d2d2d2du;  // '-'
    for (long long p0 = (long long)blockIdx.x * kProjWaves; p0 < a.P; p0 += (long long)gridDim.x * kProjWaves) {  // block uniform
        const long long p = p0 + wave;
        const bool live = p < a.P;
        long long lo = 0, hi = 0, off = 0;
        int len = 0;
        if (live) {
            lo = min(max(a.col_offsets[p], 0ll), a.n_cols_total);
            hi = min(max(a.col_offsets[p + 1], lo), a.n_cols_total);
            off = a.seq_off[p];
            if (off >= 0 && off < a.n_bytes) len = (int)min((long long)max(a.seq_len[p], 0), a.n_bytes - off);
            for (int d = lane; d < lq_dw; d += 64) {
                const int n = a.Lq - 4 * d;  // the columns of this dword that lie before Lq: 1 .. 4 of them count
                reinterpret_cast<unsigned*>(row_lds)[d] = n >= 4 ? gaps : gaps & ((1u << (8 * n)) - 1u);
            }
        }
        // pass 1: the path positions of the first and the last match
        long long first = hi, last = lo - 1;
        for (long long c = lo + lane; c < hi; c += 64) {
            const int i = a.cols[2 * c], j = a.cols[2 * c + 1];
            if ((unsigned)i < (unsigned)a.Lq && (unsigned)j < (unsigned)len) {
                first = min(first, c);
                last = max(last, c);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            first = min(first, (long long)__shfl_xor(first, o, 64));
            last = max(last, (long long)__shfl_xor(last, o, 64));
        }
        __syncthreads();  // the fill stands before the letters
        // pass 2: the letters and the counts
        int n_match = 0, n_ident = 0, n_ins = 0, n_del = 0;
        for (long long c = lo + lane; c < hi; c += 64) {
            const int i = a.cols[2 * c], j = a.cols[2 * c + 1];
            const bool qi = (unsigned)i < (unsigned)a.Lq, tj = (unsigned)j < (unsigned)len;
            const bool inside = c > first && c < last;
            if (qi && tj) {
                const unsigned char ch = a.seqs[off + j];
                row_lds[i] = ch;
                n_match += 1;
                n_ident += ch == a.query[i] ? 1 : 0;
            } else if (qi && j == -1) {
                n_del += inside ? 1 : 0;
            } else if (i == -1 && tj) {
                n_ins += inside ? 1 : 0;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n_match += __shfl_xor(n_match, o, 64);
            n_ident += __shfl_xor(n_ident, o, 64);
            n_ins += __shfl_xor(n_ins, o, 64);
            n_del += __shfl_xor(n_del, o, 64);
        }
        __syncthreads();  // the letters stand before the row is read back
        if (live) {
            unsigned* out = reinterpret_cast<unsigned*>(a.msa + (size_t)p * a.ld);
            for (int d = lane; d < ld_dw; d += 64) out[d] = d < lq_dw ? reinterpret_cast<const unsigned*>(row_lds)[d] : 0u;
            if (lane == 0) {
                int* st = a.stats + (size_t)p * kStats;
                st[0] = n_match, st[1] = n_ident, st[2] = n_ins, st[3] = n_del;
                st[4] = n_match > 0 ? a.cols[2 * first] : -1;
                st[5] = n_match > 0 ? a.cols[2 * last] : -1;
            }
        }
        __syncthreads();  // the row has been read before the next round fills it
    }
}

// ---- pairwise identity --------------------------------------------------------------------------------------------------
// bit 7 of every non-zero byte of x (the carry trick of msa_select.hip's nonzero_bytes, kept as a mask)
ESMK_DEV unsigned nonzero_mask(unsigned x) { return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }

// Columns c .. c + 3 of one row as a dword (column c in the low byte), columns at or past L as the gap byte (g4: the gap byte
// in all four); c % 4 == 0.  ALIGNED: the matrix base and ld are multiples of 4, so the dword at c < L lies inside the row's ld
// bytes and is read whole, then masked.  Otherwise the bytes below L are read one by one: nothing at or past L is touched.
template <bool ALIGNED>
ESMK_DEV unsigned load_cols4_gap(const unsigned char* __restrict__ row, int c, int L, unsigned g4) {
    if (c >= L) return g4;
    const int n = L - c;
    if (ALIGNED) {
        const unsigned v = *reinterpret_cast<const unsigned*>(row + c);
        if (n >= 4) return v;
        const unsigned m = (1u << (8 * n)) - 1u;
        return (v & m) | (g4 & ~m);
    }
    unsigned v = row[c];
    v |= (n > 1 ? (unsigned)row[c + 1] : (g4 & 0xffu)) << 8;
    v |= (n > 2 ? (unsigned)row[c + 2] : (g4 & 0xffu)) << 16;
    v |= (n > 3 ? (unsigned)row[c + 3] : (g4 & 0xffu)) << 24;
    return v;
}

// S[r][j] = same / both of rows i0 + r and j over the columns below L (file header), 0 when both < min_overlap.
//   tile    a workgroup owns the 64 x 64 tile (blockIdx.y, blockIdx.x) of S: rows i0 + 64 y .., columns 64 x ..; the column
//           tiles run to ldS, and a row at or past N is staged as gaps: both = 0, so the padding columns come out as 0
//   lanes   thread (ti, tj) = (tid / 16, tid % 16) owns the 4 x 4 pairs (4 ti + r, 4 tj + c), `same` and `both` in registers,
//           and stores each of its four rows as one float4 (ldS % 4 == 0, S 16-byte aligned)
//   LDS     as neighbor_counts_kernel: chunks of 128 columns, [dword k][row] with a row stride of 68 dwords
// Per dword and pair: ma & mb, popcount-accumulate, xor, and, add, or, and-not, popcount-accumulate, and the two gap masks
// of a dword once per four pairs: about ten VALU operations per four columns per pair.
constexpr int kTile = 64, kChunk = 32, kStride = kTile + 4;

template <bool ALIGNED>
__global__ __launch_bounds__(256) void msa_pair_identity_kernel(const unsigned char* __restrict__ msa, int N, int L, int ld, unsigned g4,
                                                                int min_overlap, int i0, int nb, float* __restrict__ S, int ldS) {
    __shared__ __attribute__((aligned(16))) unsigned sa[kChunk * kStride];
    __shared__ __attribute__((aligned(16))) unsigned sb[kChunk * kStride];
    const int tid = threadIdx.x, lane = tid & 63;
    const int ti = (tid >> 6) * 4 + (lane >> 4), tj = lane & 15;
    const int r0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    const int n_dw = (L + 3) >> 2;
    const int sk = tid & 31, sr = tid >> 5;  // staging: dword sk of the rows sr, sr + 8, ... of the tile
    int same[4][4], both[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) same[r][c] = 0, both[r][c] = 0;
    for (int k0 = 0; k0 < n_dw; k0 += kChunk) {
        const int kc = min(kChunk, n_dw - k0);
        __syncthreads();  // the chunk before this one has been read by everyone
        if (sk < kc) {
            const int col = (k0 + sk) * 4;
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int r = p * 8 + sr;
                const int ra = r0 + r, jb = j0 + r;
                const int ia = i0 + ra;
                sa[sk * kStride + r] = (ra < nb && ia < N) ? load_cols4_gap<ALIGNED>(msa + (size_t)ia * ld, col, L, g4) : g4;
                sb[sk * kStride + r] = jb < N ? load_cols4_gap<ALIGNED>(msa + (size_t)jb * ld, col, L, g4) : g4;
            }
        }
        __syncthreads();
        for (int k = 0; k < kc; ++k) {
            const uint4 a4 = *reinterpret_cast<const uint4*>(&sa[k * kStride + ti * 4]);
            const uint4 b4 = *reinterpret_cast<const uint4*>(&sb[k * kStride + tj * 4]);
            const unsigned av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
            unsigned ma[4], mb[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) ma[r] = nonzero_mask(av[r] ^ g4), mb[r] = nonzero_mask(bv[r] ^ g4);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const unsigned m = ma[r] & mb[c], x = av[r] ^ bv[c];
                    const unsigned differ = ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x;  // bit 7 of a byte: the bytes differ
                    both[r][c] += __popc(m);
                    same[r][c] += __popc(m & ~differ);
                }
        }
    }
    const int j = j0 + tj * 4;
    if (j >= ldS) return;  // (a float4 lies wholly before ldS or wholly behind it)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int rr = r0 + ti * 4 + r;
        if (rr >= nb) continue;
        f32x4 v;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            v[c] = both[r][c] >= min_overlap ? __fdiv_rn((float)same[r][c], (float)both[r][c]) : 0.f;
        *reinterpret_cast<f32x4*>(S + (size_t)rr * ldS + j) = v;
    }
}

bool misaligned(const void* p, size_t a) { return ((size_t)p & (a - 1)) != 0; }

}  // namespace

extern "C" {

int esmk_op_msa_project(const int32_t* cols_dev, long long n_cols_total, const int64_t* col_offsets_dev, int P, const uint8_t* seqs_dev,
                        long long n_bytes, const int64_t* seq_off_dev, const int32_t* seq_len_dev, const uint8_t* query_dev, int Lq,
                        uint8_t* msa_dev, int ld, int32_t* stats_dev, void* stream) {
    const std::string w("esmk_op_msa_project");
    if (!col_offsets_dev || !seq_off_dev || !seq_len_dev || !query_dev || !msa_dev || !stats_dev) return fail(w + ": null argument");
    if (n_cols_total < 0 || n_bytes < 0) return fail(w + ": n_cols_total and n_bytes must not be negative");
    if (n_cols_total > 0 && !cols_dev) return fail(w + ": null cols with n_cols_total > 0");
    if (n_bytes > 0 && !seqs_dev) return fail(w + ": null seqs with n_bytes > 0");
    if (P < 0 || P > ESMK_MAX_ROWS) return fail(w + ": need 0 <= P <= 2^24");
    if (Lq < 1 || Lq > kProjMaxLq) return fail(w + ": Lq must be 1 .. 8192");
    if (ld < Lq || ld % 4 != 0) return fail(w + ": ld must be a multiple of 4 that is >= Lq");
    if ((long long)P * ld >= (1LL << 31)) return fail(w + ": P * ld must be below 2^31");
    if (misaligned(cols_dev, 4) || misaligned(col_offsets_dev, 8) || misaligned(seq_off_dev, 8) || misaligned(seq_len_dev, 4) ||
        misaligned(msa_dev, 4) || misaligned(stats_dev, 4))
        return fail(w + ": col_offsets and seq_off must be 8-byte aligned, cols, seq_len, msa and stats 4-byte aligned");
    if (P == 0) return 0;
    ProjectArgs a;
    a.cols = cols_dev, a.n_cols_total = n_cols_total, a.col_offsets = (const long long*)col_offsets_dev, a.P = P;
    a.seqs = seqs_dev, a.n_bytes = n_bytes, a.seq_off = (const long long*)seq_off_dev, a.seq_len = seq_len_dev;
    a.query = query_dev, a.Lq = Lq, a.msa = msa_dev, a.ld = ld, a.stats = stats_dev;
    const unsigned blocks = (unsigned)std::min<long long>(((long long)P + kProjWaves - 1) / kProjWaves, 16384);
    hipLaunchKernelGGL(msa_project_kernel, dim3(blocks), dim3(kProjThreads), 0, (hipStream_t)stream, a);
    ESMK_TRY(hipGetLastError());
    return 0;
}

int esmk_op_msa_pair_identity(const uint8_t* msa_dev, int N, int L, int ld, int gap, int min_overlap, int i0, int nb, float* S_dev,
                              int ldS, void* stream) {
    const std::string w("esmk_op_msa_pair_identity");
    if (!msa_dev || !S_dev) return fail(w + ": null argument");
    if (N <= 0 || L <= 0) return fail(w + ": N and L must be positive");
    if (N > (1 << 22)) return fail(w + ": N must not exceed 2^22");
    if (ld < L) return fail(w + ": ld must not be smaller than L");
    if ((long long)N * ld >= (1LL << 31)) return fail(w + ": N * ld must be below 2^31");
    if (L > 65535) return fail(w + ": L must not exceed 65535");
    if (gap < 0 || gap > 255) return fail(w + ": the gap byte must be 0 .. 255");
    if (min_overlap < 1) return fail(w + ": min_overlap must be at least 1");
    if (i0 < 0 || nb < 0 || (long long)i0 + nb > N) return fail(w + ": the row block must lie in [0, N)");
    if (nb > (1 << 21)) return fail(w + ": a row block holds at most 2^21 rows");
    if (ldS < N || ldS % 4 != 0 || ldS > (1 << 22)) return fail(w + ": ldS must be a multiple of 4 in N .. 2^22");
    if (misaligned(S_dev, 16)) return fail(w + ": S must be 16-byte aligned");
    if (nb == 0) return 0;
    const unsigned g4 = (unsigned)gap * 0x01010101u;
    const dim3 grid((unsigned)((ldS + kTile - 1) / kTile), (unsigned)((nb + kTile - 1) / kTile));
    if (ld % 4 == 0 && !misaligned(msa_dev, 4))
        hipLaunchKernelGGL(msa_pair_identity_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, msa_dev, N, L, ld, g4, min_overlap, i0,
                           nb, S_dev, ldS);
    else
        hipLaunchKernelGGL(msa_pair_identity_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, msa_dev, N, L, ld, g4, min_overlap, i0,
                           nb, S_dev, ldS);
    ESMK_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
