// align.hip — embedding-based alignment of two proteins (esm_amd/align.py).
//
// S[i][j] = <u_a[i], u_b[j]> comes from the existing dense GEMM over two f16x3 operand images (hi | hi | lo rows of the a side
// against hi | lo | hi rows of the b side, fp32 store epilogue); the kernels here are what stands around it, one launch each,
// no global atomics, every result a function of its inputs alone:
//     image_rows_kernel       (elementwise.hip) gather the listed rows, form u (cosine: x * float32(1 / sqrt(sum x^2))), write
//                             one of the two images
//     align_enhance_kernel    per pair block, in place: the mean of the row and the column z-score
//     align_dp_kernel         per pair: Needleman-Wunsch / Smith-Waterman with affine gaps, score, end cell, traceback bytes
//     align_traceback_kernel  per pair: walk the bytes, write the alignment's columns
//
// The recurrence (fp32 adds, subtractions and comparisons only; (i, j) over 0 .. La x 0 .. Lb; H[0][0] = 0, E[i][0] = F[0][j] =
// -inf; max(x, y) is "y if y > x else x"):
//     E[i][j] = max(H[i][j-1] - o, E[i][j-1] - e)        extend bit (4) iff E[i][j-1] - e > H[i][j-1] - o
//     F[i][j] = max(H[i-1][j] - o, F[i-1][j] - e)        extend bit (8), same rule
//     D       = S[i-1][j-1] + H[i-1][j-1]
//     H[i][j] = the first of maximal value among [stop = 0 (local only; global starts from -inf), D, F, E]     bits 0-1: 0 1 2 3
// Traceback bytes exist for the cells i, j >= 1 (row i - 1, column j - 1 of a byte matrix with a row stride of Lb rounded up to
// 16); on row 0 and column 0 the walk needs none: global mode emits the remaining gaps, local mode stops (H = 0 there).
//
// Free end gaps (global mode only; the `free_ends` mask of the _ex entries, wave-uniform; 0 is plain global mode).  Only the
// "stop" candidate on the borders and the end cell change, every fp32 operation and its order stay:
//     1 a_start  H[i][0] = 0 for all i (the column-0 value local mode uses); the walk stops on column 0
//     4 b_start  on row 0 the stop candidate is 0, so H[0][j] = 0 with choice "stop"; the walk stops on row 0
//     2 a_end    the cells (i, Lb), i = 1 .. La, are end-cell candidates next to the corner (La, Lb)
//     8 b_end    the cells (La, j), j = 1 .. Lb, are
// E and F on the borders are unchanged.  Among the candidates (never a cell with i = 0 or j = 0) the largest H wins, ties go
// to the lower row, then the lower column: a lane keeps its first best, and the wavefront reduction below orders the lanes.
//
// Several hits per pair (Waterman-Eggert): the traceback kernel, given a writable S, stores -inf at every MATCH cell of the
// path it walks (plain vector stores of one float by the thread that walks the pair), and the DP and the walk run again on the
// same S; gap states may still cross an earlier path.  A pair's block of S belongs to that pair alone — the callers list no
// pair twice (align.py's check_pairs) and every sequence of b has its own columns — so no other thread reads or writes those
// cells in the launch.  -inf + finite and the comparisons produce no NaN (H is never +inf).
//
// The DP kernel: one wavefront per pair, four per workgroup.  Lane l owns the 8 columns j0 + 8 l + 1 .. j0 + 8 l + 8 of a panel
// of 512 in registers (H and F of the previous row) and works on row t - l at step t; the strip's right edge (H, E) moves to lane
// l + 1 once per step.  A side wider than one panel goes panel by panel: lane 63 writes the boundary column (H, E per row) to
// the wavefront's workspace column and lane 0 of the next panel reads it back, in place (row r is read at step r - 1 and
// rewritten at step r + 63).  Row 0 goes through the array like any other row (D = F = -inf), so the boundary row's chain of
// subtractions is the reference's.  S: lane l reads 32 bytes of row t - l — a whole sector; the four lanes that share a 128-byte
// line read it in four consecutive steps, and the loads of step t + 1 are issued before the arithmetic of step t.
#include "common.h"
#include "engine_internal.h"

#include <cmath>
#include <string>

using namespace esmk;
using namespace esmk_host;

namespace {

constexpr int kStrip = 8;              // columns a lane owns
constexpr int kPanel = 64 * kStrip;    // columns a wavefront covers at once
constexpr int kAlignMaxLen = 8192;     // the longest side
constexpr int kAlignMaxWaves = 16384;  // wavefronts of a DP launch (pairs beyond are taken in turn)
constexpr int kAlignMaxWgs = 1024;     // workgroups of an enhancement launch

ESMK_DEV long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }
ESMK_DEV int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// A pair's table entry (device data: every value is clamped to what the launch's buffers hold).
struct PairGeom {
    int La, Lb, a_off, b_off;
};
ESMK_DEV PairGeom pair_geom(const long long* t, int max_la, int max_lb, int n_rows, int n_cols) {
    PairGeom g;
    g.La = (int)clampll(t[1], 0, min(max_la, n_rows));
    g.Lb = (int)clampll(t[3], 0, min(max_lb, n_cols));
    g.a_off = (int)clampll(t[0], 0, n_rows - g.La);
    g.b_off = (int)clampll(t[2] & ~7LL, 0, n_cols - ((g.Lb + 7) & ~7));  // n_cols % 8 == 0
    return g;
}

// ---- enhancement --------------------------------------------------------------------------------------------------------
// Workgroup w takes the pairs w, w + n_wg, ...  Column statistics first (thread per column, rows ascending), into the
// workgroup's workspace; then thread per row: the row's statistics (columns ascending) and the rewrite of the row.  Mean: the
// fp64 sum in ascending order / n, rounded to fp32.  Deviation: sqrt(fp64 sum of (S - m)^2 in ascending order / n) with m the
// fp64 mean before its rounding, rounded to fp32.
__global__ __launch_bounds__(256) void align_enhance_kernel(float* __restrict__ S, int ldS, int n_rows, int n_cols,
                                                            const long long* __restrict__ table, int n_pairs, int max_lb,
                                                            float* __restrict__ ws, int n_wg) {
    const int tid = threadIdx.x;
    float* mu_c = ws + (size_t)blockIdx.x * 2 * max_lb;
    float* inv_c = mu_c + max_lb;
    for (int p = blockIdx.x; p < n_pairs; p += n_wg) {
        const PairGeom g = pair_geom(table + 5 * (size_t)p, kAlignMaxLen, max_lb, n_rows, n_cols);
        float* Sp = S + (size_t)g.a_off * ldS + g.b_off;
        for (int j = tid; j < g.Lb; j += 256) {
            double s = 0.0;
            for (int i = 0; i < g.La; ++i) s = dadd_rn(s, (double)Sp[(size_t)i * ldS + j]);
            const double m = s / (double)g.La;
            double q = 0.0;
            for (int i = 0; i < g.La; ++i) {
                const double d = dsub_rn((double)Sp[(size_t)i * ldS + j], m);
                q = dadd_rn(q, dmul_rn(d, d));
            }
            const float sd = (float)sqrt(q / (double)g.La);
            mu_c[j] = (float)m;
            inv_c[j] = sd == 0.f ? 0.f : 1.f / sd;
        }
        __syncthreads();
        for (int i = tid; i < g.La; i += 256) {
            float* row = Sp + (size_t)i * ldS;
            double s = 0.0;
            for (int j = 0; j < g.Lb; ++j) s = dadd_rn(s, (double)row[j]);
            const double m = s / (double)g.Lb;
            double q = 0.0;
            for (int j = 0; j < g.Lb; ++j) {
                const double d = dsub_rn((double)row[j], m);
                q = dadd_rn(q, dmul_rn(d, d));
            }
            const float sd = (float)sqrt(q / (double)g.Lb);
            const float mu = (float)m, inv = sd == 0.f ? 0.f : 1.f / sd;
            for (int j = 0; j < g.Lb; ++j) {
                const float v = row[j];
                row[j] = mul_rn(0.5f, add_rn(mul_rn(sub_rn(v, mu), inv), mul_rn(sub_rn(v, mu_c[j]), inv_c[j])));
            }
        }
        __syncthreads();  // the column statistics have been read
    }
}

// ---- the dynamic program ------------------------------------------------------------------------------------------------
struct AlignDpArgs {
    const float* S;
    int ldS, n_rows, n_cols;
    const long long* table;  // [n_pairs, 5]: row offset of a, La, column offset of b (a multiple of 8), Lb, traceback offset (bytes)
    int n_pairs, local, free_ends;
    float o, e;
    int max_la, max_lb;
    float* score;
    int* end;
    unsigned char* tb;  // null: no traceback bytes
    long long tb_bytes;
    f32x2* ws;  // [n_waves, max_la + 1] boundary columns (H, E), or null when no side b exceeds one panel
    int n_waves;
};

// One body, two instances: kFree = false is the kernel of the plain modes (the mask is the constant 0 there, so the stop
// candidate is a constant and the candidate search below does not exist); kFree = true is launched when free_ends != 0.
template <bool kFree>
ESMK_DEV __attribute__((always_inline)) void align_dp_body(const AlignDpArgs& a) {
    const int lane = threadIdx.x & 63;
    const int gw = uniform(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (gw >= a.n_waves) return;
    const float NEG = -__builtin_inff();
    const float o = a.o, e = a.e;
    const bool local = a.local != 0;
    const int fe = kFree ? uniform(a.free_ends) : 0;
    const bool zero_col = local || (fe & 1) != 0, zero_row = (fe & 4) != 0, a_end = (fe & 2) != 0, b_end = (fe & 8) != 0;
    const bool track = local || fe != 0;  // the end cell is searched for, not given
    f32x2* wsw = a.ws ? a.ws + (size_t)gw * (a.max_la + 1) : nullptr;
    for (int p = gw; p < a.n_pairs; p += a.n_waves) {
        const long long* t = a.table + 5 * (size_t)p;
        const PairGeom g = pair_geom(t, a.max_la, wsw ? a.max_lb : min(a.max_lb, kPanel), a.n_rows, a.n_cols);
        const int La = uniform(g.La), Lb = uniform(g.Lb), a_off = uniform(g.a_off), b_off = uniform(g.b_off);
        if (La < 1 || Lb < 1) {
            if (lane == 0) {
                a.score[p] = 0.f;
                a.end[2 * p] = 0;
                a.end[2 * p + 1] = 0;
            }
            continue;
        }
        const int ldtb = (Lb + 15) & ~15;
        const long long need = (long long)La * ldtb;
        const bool wtb = a.tb != nullptr && need <= a.tb_bytes;
        const long long tb_off = wtb ? clampll(t[4] & ~7LL, 0, a.tb_bytes - need) : 0;
        float bv = local ? 0.f : NEG;
        int bi = 0, bj = 0;
        const int npanel = (Lb + kPanel - 1) / kPanel;
        for (int pn = 0; pn < npanel; ++pn) {
            const int j0 = pn * kPanel;
            const int nl = min(64, (Lb - j0 + kStrip - 1) / kStrip);
            const int jl = j0 + lane * kStrip;  // the strip's first column, 0-based in S
            const bool lane_on = lane < nl;     // jl < Lb
            const float* Sp = a.S + (size_t)a_off * a.ldS + b_off + jl;
            unsigned char* tp = wtb ? a.tb + tb_off + jl : nullptr;
            const bool carry_in = pn > 0, carry_out = pn + 1 < npanel;
            float Hp[kStrip], Fp[kStrip];
#pragma unroll
            for (int c = 0; c < kStrip; ++c) Hp[c] = Fp[c] = NEG;
            float hlast = NEG, elast = NEG, hdiag = NEG;
            float h0 = 0.f, f0 = NEG;  // column 0, kept by every lane for its own row, used by lane 0 of panel 0
            f32x4 s0n = f32x4{0.f, 0.f, 0.f, 0.f}, s1n = s0n;
            f32x2 cn = f32x2{NEG, NEG};
            if (carry_in && lane == 0) cn = wsw[0];
            const int steps = La + nl;
            for (int st = 0; st < steps; ++st) {
                const int i = st - lane;
                const bool on = lane_on && i >= 0 && i <= La;
                const f32x4 s0 = s0n, s1 = s1n;
                const f32x2 cin = cn;
                {  // the loads of the next step
                    const int i1 = i + 1;
                    if (lane_on && i1 >= 1 && i1 <= La) {
                        const float* q = Sp + (size_t)(i1 - 1) * a.ldS;
                        s0n = *reinterpret_cast<const f32x4*>(q);
                        s1n = *reinterpret_cast<const f32x4*>(q + 4);
                    }
                    if (carry_in && lane == 0 && i1 <= La) cn = wsw[i1];
                }
                float hl = __shfl_up(hlast, 1, 64), el = __shfl_up(elast, 1, 64);
                if (i <= 0) {
                    h0 = 0.f;
                    f0 = NEG;
                } else {
                    const float x = h0 - o, y = f0 - e;
                    f0 = y > x ? y : x;
                    h0 = zero_col ? 0.f : f0;
                }
                if (lane == 0) {
                    hl = carry_in ? cin[0] : h0;
                    el = carry_in ? cin[1] : NEG;
                }
                const float hleft = hl;
                const bool top = i <= 0;
                float hd = hdiag;
                const float sv[kStrip] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
                unsigned int w[2] = {0u, 0u};
                const float stop = local || (zero_row && top) ? 0.f : NEG;
                const bool corner_row = !track && on && i == La;
#pragma unroll
                for (int c = 0; c < kStrip; ++c) {
                    const float ex = hl - o, ey = el - e;
                    const bool eb = ey > ex;
                    const float E = eb ? ey : ex;
                    const float fx = Hp[c] - o, fy = Fp[c] - e;
                    const bool fb = !top && fy > fx;
                    const float F = top ? NEG : (fb ? fy : fx);
                    const float D = top ? NEG : sv[c] + hd;
                    float best = stop;
                    unsigned int ch = 0;
                    if (D > best) best = D, ch = 1;
                    if (F > best) best = F, ch = 2;
                    if (E > best) best = E, ch = 3;
                    hd = Hp[c];
                    Hp[c] = best;
                    Fp[c] = F;
                    hl = best;
                    el = E;
                    const bool valid = jl + c < Lb;
                    const unsigned int byte = valid ? (ch | (eb ? 4u : 0u) | (fb ? 8u : 0u)) : 0u;
                    w[c >> 2] |= byte << (8 * (c & 3));
                    if (local) {
                        if (on && valid && i >= 1 && (best > bv || (best == bv && i < bi))) bv = best, bi = i, bj = jl + c + 1;
                    } else if (corner_row && jl + c + 1 == Lb) {
                        bv = best, bi = La, bj = Lb;
                    }
                }
                // free ends: the row's end-cell candidates: all cells of row La with b_end, the cell in column Lb of the rows
                // i >= 1 with a_end, the corner in any case; the first best in row order is kept (as in local mode)
                if (kFree && on && i >= 1 && (a_end || i == La)) {
                    const bool all = b_end && i == La;
#pragma unroll
                    for (int c = 0; c < kStrip; ++c) {
                        const float h = Hp[c];
                        if (jl + c < Lb && (all || jl + c + 1 == Lb) && (h > bv || (h == bv && i < bi))) bv = h, bi = i, bj = jl + c + 1;
                    }
                }
                hdiag = hleft;
                hlast = hl;
                elast = el;
                if (tp && on && i >= 1) {
                    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
                    *reinterpret_cast<u32x2*>(tp + (size_t)(i - 1) * ldtb) = u32x2{w[0], w[1]};
                }
                if (carry_out && lane == 63 && i >= 0 && i <= La) wsw[i] = f32x2{hl, el};
            }
        }
        // the best cell of the wavefront: value descending, then row, then column ascending (global: the one lane that holds it)
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const float ov = __shfl_xor(bv, s, 64);
            const int oi = __shfl_xor(bi, s, 64), oj = __shfl_xor(bj, s, 64);
            if (ov > bv || (ov == bv && (oi < bi || (oi == bi && oj < bj)))) bv = ov, bi = oi, bj = oj;
        }
        if (lane == 0) {
            a.score[p] = bv;
            a.end[2 * p] = track ? bi : La;
            a.end[2 * p + 1] = track ? bj : Lb;
        }
    }
}

__global__ __launch_bounds__(256) void align_dp_kernel(const AlignDpArgs a) { align_dp_body<false>(a); }
__global__ __launch_bounds__(256) void align_dp_free_kernel(const AlignDpArgs a) { align_dp_body<true>(a); }

// ---- traceback ----------------------------------------------------------------------------------------------------------
// One thread per pair.  The columns are found from the end cell backwards and written from the back of the pair's slot of
// La + Lb columns, so that they stand in ascending order in [slot end - n_cols, slot end).  At most La + Lb steps are taken
// whatever the bytes hold (each step lowers i or j).  With a free start the walk stops where it reaches that border (H = 0
// there, choice "stop").  S_mask non-null: every match cell of the path is set to -inf in the pair's block of S.  The block
// is clamped by pair_geom to S (n_rows, n_cols) and to the longest side, so no table can direct a store outside S; for a
// table within the DP launch's max_la / max_lb — every table the callers build — it is the block the DP kernel read.
__global__ __launch_bounds__(64) void align_traceback_kernel(const long long* __restrict__ table, int n_pairs, int local,
                                                             int free_ends, float* __restrict__ S_mask, int ldS, int n_rows,
                                                             int n_cols_S,
                                                             const int* __restrict__ end, const unsigned char* __restrict__ tb,
                                                             long long tb_bytes, const long long* __restrict__ slot,
                                                             int* __restrict__ cols, long long cols_cap, int* __restrict__ n_cols,
                                                             int* __restrict__ n_match, int* __restrict__ start) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_pairs) return;
    const long long* t = table + 5 * (size_t)p;
    const int La = (int)clampll(t[1], 0, kAlignMaxLen), Lb = (int)clampll(t[3], 0, kAlignMaxLen);
    const int ldtb = (Lb + 15) & ~15;
    const long long need = (long long)La * ldtb, cap = (long long)La + Lb;
    int i = min(max(end[2 * p], 0), La), j = min(max(end[2 * p + 1], 0), Lb);
    int n = 0, nm = 0;
    PairGeom g = {0, 0, 0, 0};
    if (S_mask) g = pair_geom(t, kAlignMaxLen, kAlignMaxLen, n_rows, n_cols_S);
    float* Sp = S_mask ? S_mask + (size_t)g.a_off * ldS + g.b_off : nullptr;
    if (La >= 1 && Lb >= 1 && need <= tb_bytes && cap <= cols_cap) {
        const unsigned char* tp = tb + clampll(t[4] & ~7LL, 0, tb_bytes - need);
        int* out = cols + 2 * (clampll(slot[p], 0, cols_cap - cap) + cap);
        int state = 0;  // 0: H, 1: F (a vertical gap is open), 2: E (a horizontal gap is open)
        for (int step = 0; step < (int)cap; ++step) {
            if (i == 0 && j == 0) break;
            int ci, cj;
            if (i == 0 || j == 0) {
                if (local || (free_ends & (j == 0 ? 1 : 4))) break;
                if (j == 0) ci = --i, cj = -1;
                else ci = -1, cj = --j;
                state = 0;
            } else {
                const unsigned int b = tp[(size_t)(i - 1) * ldtb + (j - 1)];
                if (state == 0) {
                    const unsigned int c = b & 3u;
                    if (c == 0) break;
                    state = c == 1 ? 0 : (c == 2 ? 1 : 2);
                    if (c == 1) {
                        ci = --i, cj = --j;
                        ++nm, ++n;
                        out[-2 * n] = ci, out[-2 * n + 1] = cj;
                        if (Sp && ci < g.La && cj < g.Lb) Sp[(size_t)ci * ldS + cj] = -__builtin_inff();
                        continue;
                    }
                }
                if (state == 1) ci = --i, cj = -1, state = (b & 8u) ? 1 : 0;
                else ci = -1, cj = --j, state = (b & 4u) ? 2 : 0;
            }
            ++n;
            out[-2 * n] = ci, out[-2 * n + 1] = cj;
        }
    }
    n_cols[p] = n;
    n_match[p] = nm;
    start[2 * p] = i;
    start[2 * p + 1] = j;
}

bool misaligned(const void* p, size_t a) { return ((size_t)p & (a - 1)) != 0; }

}  // namespace

extern "C" {

int esmk_op_align_panel(void) { return kPanel; }

int esmk_op_align_rows(const float* x_dev, int ldx, int N, const int32_t* rows_dev, int n, int cosine, int b_side, void* image_dev,
                       int ld_image, int E, void* stream) {
    const std::string w("esmk_op_align_rows");
    if (!x_dev || !image_dev) return fail(w + ": null argument");
    if (E <= 0 || E % 4 != 0) return fail(w + ": E must be a positive multiple of 4");
    if (N <= 0 || N > ESMK_MAX_ROWS || n < 0 || n > ESMK_MAX_ROWS) return fail(w + ": need 0 < N <= 2^24 and 0 <= n <= 2^24");
    if (!rows_dev && n > N) return fail(w + ": without a row list the first n rows are taken, n must not exceed N");
    if (ldx < E || ldx % 4 != 0) return fail(w + ": ldx must be a multiple of 4 that is >= E");
    const int Ep = (E + 63) / 64 * 64;
    if (ld_image < 3 * Ep || ld_image % 4 != 0) return fail(w + ": ld_image must be a multiple of 4 that is >= 3 * (E rounded up to 64)");
    if (misaligned(x_dev, 16) || misaligned(image_dev, 8)) return fail(w + ": x must be 16-byte aligned, the image 8-byte aligned");
    if ((cosine | 1) != 1 || (b_side | 1) != 1) return fail(w + ": cosine and b_side must be 0 or 1");
    if (n == 0) return 0;
    ESMK_TRY(launch_image_rows(x_dev, ldx, N, rows_dev, n, /*b_dec=*/nullptr, /*scale=*/1.f, cosine, b_side, /*zero_negative=*/1,
                               image_dev, ld_image, E, (hipStream_t)stream));
    return 0;
}

static int check_s(const std::string& w, const void* S, int ldS, int n_rows, int n_cols, const void* table, int n_pairs) {
    if (!S || !table) return fail(w + ": null argument");
    if (n_pairs < 0 || n_pairs > ESMK_MAX_ROWS) return fail(w + ": need 0 <= n_pairs <= 2^24");
    if (n_rows <= 0 || n_rows > ESMK_MAX_ROWS || n_cols <= 0 || n_cols % 8 != 0 || ldS < n_cols || ldS % 4 != 0)
        return fail(w + ": need 0 < n_rows <= 2^24, n_cols a positive multiple of 8, ldS a multiple of 4 that is >= n_cols");
    if (misaligned(S, 16) || misaligned(table, 8)) return fail(w + ": S must be 16-byte aligned, the table 8-byte aligned");
    return 0;
}

int esmk_op_align_enhance(float* S_dev, int ldS, int n_rows, int n_cols, const int64_t* table_dev, int n_pairs, int max_lb,
                          float* ws_dev, long long ws_floats, void* stream) {
    const std::string w("esmk_op_align_enhance");
    if (int rc = check_s(w, S_dev, ldS, n_rows, n_cols, table_dev, n_pairs)) return rc;
    if (max_lb < 1 || max_lb > kAlignMaxLen) return fail(w + ": max_lb must be 1 .. 8192");
    if (!ws_dev || ws_floats < 2LL * max_lb) return fail(w + ": the workspace must hold at least 2 * max_lb floats");
    if (n_pairs == 0) return 0;
    long long n_wg = ws_floats / (2LL * max_lb);
    if (n_wg > kAlignMaxWgs) n_wg = kAlignMaxWgs;
    if (n_wg > n_pairs) n_wg = n_pairs;
    hipLaunchKernelGGL(align_enhance_kernel, dim3((unsigned)n_wg), dim3(256), 0, (hipStream_t)stream, S_dev, ldS, n_rows, n_cols,
                       (const long long*)table_dev, n_pairs, max_lb, ws_dev, (int)n_wg);
    ESMK_TRY(hipGetLastError());
    return 0;
}

static int check_free_ends(const std::string& w, int mode, int free_ends) {
    if (free_ends < 0 || free_ends > 15) return fail(w + ": free_ends must be 0 .. 15 (1 a_start, 2 a_end, 4 b_start, 8 b_end)");
    if (free_ends != 0 && mode != 0) return fail(w + ": free_ends requires mode 0 (global)");
    return 0;
}

static int align_dp(const std::string& w, const float* S_dev, int ldS, int n_rows, int n_cols, const int64_t* table_dev, int n_pairs,
                    int mode, int free_ends, float gap_open, float gap_extend, int max_la, int max_lb, float* score_dev,
                    int32_t* end_dev, uint8_t* tb_dev, long long tb_bytes, int want_traceback, float* ws_dev, long long ws_floats,
                    void* stream) {
    if (max_la < 1 || max_la > kAlignMaxLen || max_lb < 1 || max_lb > kAlignMaxLen) return fail(w + ": max_la and max_lb must be 1 .. 8192");
    if (int rc = check_s(w, S_dev, ldS, n_rows, n_cols, table_dev, n_pairs)) return rc;
    if (!score_dev || !end_dev) return fail(w + ": null argument");
    if (mode != 0 && mode != 1) return fail(w + ": mode must be 0 (global) or 1 (local)");
    if (int rc = check_free_ends(w, mode, free_ends)) return rc;
    if (!(gap_extend >= 0.f) || !(gap_open >= gap_extend) || std::isinf(gap_open)) return fail(w + ": need 0 <= gap_extend <= gap_open < inf");
    if ((want_traceback | 1) != 1) return fail(w + ": want_traceback must be 0 or 1");
    if (want_traceback && (!tb_dev || tb_bytes <= 0 || misaligned(tb_dev, 8))) return fail(w + ": the traceback buffer must be given, 8-byte aligned");
    if (n_pairs == 0) return 0;
    long long n_waves = n_pairs < kAlignMaxWaves ? n_pairs : kAlignMaxWaves;
    if (max_lb > kPanel) {
        const long long per = 2LL * (max_la + 1);
        if (!ws_dev || ws_floats < per || misaligned(ws_dev, 8)) return fail(w + ": a side b beyond one panel needs a workspace of at least 2 * (max_la + 1) floats, 8-byte aligned");
        if (ws_floats / per < n_waves) n_waves = ws_floats / per;
    }
    AlignDpArgs a;
    a.S = S_dev, a.ldS = ldS, a.n_rows = n_rows, a.n_cols = n_cols, a.table = (const long long*)table_dev, a.n_pairs = n_pairs;
    a.local = mode, a.free_ends = free_ends, a.o = gap_open, a.e = gap_extend, a.max_la = max_la, a.max_lb = max_lb, a.score = score_dev, a.end = end_dev;
    a.tb = want_traceback ? tb_dev : nullptr, a.tb_bytes = want_traceback ? tb_bytes : 0;
    a.ws = max_lb > kPanel ? (f32x2*)ws_dev : nullptr, a.n_waves = (int)n_waves;
    hipLaunchKernelGGL(free_ends != 0 ? align_dp_free_kernel : align_dp_kernel, dim3((unsigned)((n_waves + 3) / 4)), dim3(256), 0,
                       (hipStream_t)stream, a);
    ESMK_TRY(hipGetLastError());
    return 0;
}

int esmk_op_align_dp(const float* S_dev, int ldS, int n_rows, int n_cols, const int64_t* table_dev, int n_pairs, int mode,
                     float gap_open, float gap_extend, int max_la, int max_lb, float* score_dev, int32_t* end_dev, uint8_t* tb_dev,
                     long long tb_bytes, int want_traceback, float* ws_dev, long long ws_floats, void* stream) {
    return align_dp("esmk_op_align_dp", S_dev, ldS, n_rows, n_cols, table_dev, n_pairs, mode, 0, gap_open, gap_extend, max_la, max_lb,
                    score_dev, end_dev, tb_dev, tb_bytes, want_traceback, ws_dev, ws_floats, stream);
}

int esmk_op_align_dp_ex(const float* S_dev, int ldS, int n_rows, int n_cols, const int64_t* table_dev, int n_pairs, int mode,
                        int free_ends, float gap_open, float gap_extend, int max_la, int max_lb, float* score_dev, int32_t* end_dev,
                        uint8_t* tb_dev, long long tb_bytes, int want_traceback, float* ws_dev, long long ws_floats, void* stream) {
    return align_dp("esmk_op_align_dp_ex", S_dev, ldS, n_rows, n_cols, table_dev, n_pairs, mode, free_ends, gap_open, gap_extend,
                    max_la, max_lb, score_dev, end_dev, tb_dev, tb_bytes, want_traceback, ws_dev, ws_floats, stream);
}

static int align_traceback(const std::string& w, const int64_t* table_dev, int n_pairs, int mode, int free_ends,
                           const int32_t* end_dev, const uint8_t* tb_dev, long long tb_bytes, const int64_t* slot_dev,
                           int32_t* cols_dev, long long cols_cap, int32_t* n_cols_dev, int32_t* n_match_dev, int32_t* start_dev,
                           float* S_mask_dev, int ldS, int n_rows, int n_cols, void* stream) {
    if (!table_dev || !end_dev || !tb_dev || !slot_dev || !cols_dev || !n_cols_dev || !n_match_dev || !start_dev) return fail(w + ": null argument");
    if (n_pairs < 0 || n_pairs > ESMK_MAX_ROWS) return fail(w + ": need 0 <= n_pairs <= 2^24");
    if (mode != 0 && mode != 1) return fail(w + ": mode must be 0 (global) or 1 (local)");
    if (int rc = check_free_ends(w, mode, free_ends)) return rc;
    if (S_mask_dev) {
        if (n_rows <= 0 || n_rows > ESMK_MAX_ROWS || n_cols <= 0 || n_cols % 8 != 0 || ldS < n_cols || ldS % 4 != 0)
            return fail(w + ": S_mask needs 0 < n_rows <= 2^24, n_cols a positive multiple of 8, ldS a multiple of 4 that is >= n_cols");
        if (misaligned(S_mask_dev, 16)) return fail(w + ": S_mask must be 16-byte aligned");
    } else if (ldS != 0 || n_rows != 0 || n_cols != 0) {
        return fail(w + ": without S_mask, ldS, n_rows and n_cols must be 0");
    }
    if (tb_bytes <= 0 || cols_cap <= 0) return fail(w + ": tb_bytes and cols_cap must be positive");
    if (misaligned(table_dev, 8) || misaligned(slot_dev, 8)) return fail(w + ": the table and the slots must be 8-byte aligned");
    if (n_pairs == 0) return 0;
    hipLaunchKernelGGL(align_traceback_kernel, dim3((unsigned)((n_pairs + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                       (const long long*)table_dev, n_pairs, mode, free_ends, S_mask_dev, ldS, n_rows, n_cols, end_dev, tb_dev,
                       tb_bytes, (const long long*)slot_dev, cols_dev, cols_cap, n_cols_dev, n_match_dev, start_dev);
    ESMK_TRY(hipGetLastError());
    return 0;
}

int esmk_op_align_traceback(const int64_t* table_dev, int n_pairs, int mode, const int32_t* end_dev, const uint8_t* tb_dev,
                            long long tb_bytes, const int64_t* slot_dev, int32_t* cols_dev, long long cols_cap, int32_t* n_cols_dev,
                            int32_t* n_match_dev, int32_t* start_dev, void* stream) {
    return align_traceback("esmk_op_align_traceback", table_dev, n_pairs, mode, 0, end_dev, tb_dev, tb_bytes, slot_dev, cols_dev,
                           cols_cap, n_cols_dev, n_match_dev, start_dev, nullptr, 0, 0, 0, stream);
}

int esmk_op_align_traceback_ex(const int64_t* table_dev, int n_pairs, int mode, int free_ends, const int32_t* end_dev,
                               const uint8_t* tb_dev, long long tb_bytes, const int64_t* slot_dev, int32_t* cols_dev,
                               long long cols_cap, int32_t* n_cols_dev, int32_t* n_match_dev, int32_t* start_dev, float* S_mask_dev,
                               int ldS, int n_rows, int n_cols, void* stream) {
    return align_traceback("esmk_op_align_traceback_ex", table_dev, n_pairs, mode, free_ends, end_dev, tb_dev, tb_bytes, slot_dev,
                           cols_dev, cols_cap, n_cols_dev, n_match_dev, start_dev, S_mask_dev, ldS, n_rows, n_cols, stream);
}

}  // extern "C"
