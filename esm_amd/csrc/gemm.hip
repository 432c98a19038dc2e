// gemm.hip — the two one-tile-per-workgroup nn.Linear kernels and their launchers:
//     C[M,N] = A[M,K] . W[N,K]^T (+ bias, + epilogue)
//
// gemm256 is the reference the persistent kernels (gemm8.hip, gemm9.hip) are tested against bit for bit (force_old);
// gemm64 serves the shapes no other kernel covers (K % 64 != 0, N % 8 != 0 such as the 33-wide vocabulary projection).
// Which kernel a call gets is decided in gemm_dispatch.hip (gemm_plan); nothing here reads a switch.
//
// The linear layers replace every torch.nn.Linear / F.linear call of the ESM-2 layer stack
// (reference esm/multihead_attention.py:256-261,395; esm/modules.py:138-139,309,313) and fuse
// what the reference runs as separate elementwise ops into the epilogue (gemm_epi.h):
//   * bias add,
//   * q scaling (multihead_attention.py:261), rotary embedding (rotary_embedding.py:11-20,63-69)
//     and the head split / transpose (multihead_attention.py:280-284)        -> EPI_QKV_ROPE (q,k), EPI_V_T (v)
//   * exact-erf GELU (modules.py:17-24)                                      -> EPI_GELU_*
//   * residual add into the fp32 stream (modules.py:134,140)                 -> EPI_RESID_F32
//
// gemm256: 256x256 output tile, K step 64, 8 waves (2 along M x 4 along N, each
// wave 128x64 = 8x4 v_mfma_f32_16x16x32 blocks), operands staged HBM->LDS with
// global_load_lds_dwordx4 into two 64 KiB LDS buffers (one barrier per K step), LDS rows are
// 128 B with the 16-byte chunk index XOR-swizzled by ((row>>1)&7) so that every ds_read_b128
// lane group touches 16 distinct 16-byte slots (conflict free).  Because global_load_lds
// writes lane-linear, the swizzle is applied to the per-lane SOURCE address and again on the
// read side.  Workgroup ids are remapped so each XCD (private L2) owns a contiguous run of
// tiles with the N index fastest: the 256-row activation panel is fetched from HBM once per
// XCD and re-used from L2 by all N tiles.
//
// The MFMA is issued "swapped" (A operand = weight rows, B operand = activation rows) so a
// lane owns 4 consecutive output columns of one output row: epilogue stores are 8 B (f16/bf16)
// or 16 B (fp32) per lane, and the RoPE partner (column + 32 of the same head) lives in the
// same lane and register index two 16-column blocks further.
//
// gemm64: 64x64 tile, K step 32, register staged with row clamping and per-element predicated stores.
#include "gemm_epi.h"

namespace esmk {

// --------------------------------------------------------------------------------------------
// fast kernel: 256 x 256 x 64
// --------------------------------------------------------------------------------------------
constexpr int G_BM = 256, G_BN = 256, G_BK = 64;
constexpr int G_TILE_BYTES = G_BM * G_BK * 2;  // 32 KiB per operand per stage
constexpr int G_STAGE_BYTES = 2 * G_TILE_BYTES;
constexpr int G_LDS_BYTES = 2 * G_STAGE_BYTES;  // 128 KiB

template <typename T, int EPI>
__global__ __launch_bounds__(512, 2) void gemm256_kernel(GemmArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;

    const int tiles_n = (p.N + G_BN - 1) / G_BN;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int tm = wg / tiles_n, tn = wg - tm * tiles_n;
    const int m0 = tm * G_BM, n0 = tn * G_BN;

    const T* __restrict__ A = reinterpret_cast<const T*>(p.A);
    const T* __restrict__ W = reinterpret_cast<const T*>(p.W);

    // per-lane staging sources: 4 rounds x (A, W); LDS position (row r, slot s) receives global
    // chunk c = s ^ ((r >> 1) & 7) of row r (16-byte chunks of the 128-byte K slab).
    const T* ga[4];
    const T* gw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pos = j * 512 + tid;
        const int r = pos >> 3, s = pos & 7;
        const int c = s ^ ((r >> 1) & 7);
        const int ra = min(m0 + r, p.M - 1);
        const int rw = min(n0 + r, p.N - 1);
        ga[j] = A + (size_t)ra * p.K + c * 8;
        gw[j] = W + (size_t)rw * p.K + c * 8;
    }

    // One staging "part" = round j of the activation tile + round j of the weight tile (2 LDS-DMA
    // instructions per wave, 16 KiB per workgroup); a K tile is 4 parts.
    auto stage_part = [&](int buf, int kt, int j) {
        char* base = smem + buf * G_STAGE_BYTES;
        const int ko = kt * G_BK;
        glds16(ga[j] + ko, base + (j * 512 + wave * 64) * 16);
        glds16(gw[j] + ko, base + G_TILE_BYTES + (j * 512 + wave * 64) * 16);
    };
    auto stage = [&](int buf, int kt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) stage_part(buf, kt, j);
    };

    // fragment read offsets (bytes) inside a tile: 16 x 16 x 32 MFMA blocks, lane l reads row l & 15 of a 16-row
    // block and 16-byte chunk 4 kh + (l >> 4) of its 128-byte row (kh = K half of the tile)
    const int lrow = (lane & 15) * 128;
    const int swz = (lane >> 1) & 7;
    int xo[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) xo[ks] = ((4 * ks + (lane >> 4)) ^ swz) << 4;
    const int a_off = (wm * 128) * 128 + lrow;                // activation rows of this wave
    const int w_off = G_TILE_BYTES + (wn * 64) * 128 + lrow;  // weight rows of this wave

    // acc = bias (gemm8's order: the bias rides through the K loop), EPI_V_T adds it in its epilogue
    f32x4 acc[4][8];  // [16-column block][16-row block]
    {
        const int nb = n0 + wn * 64;
#pragma unroll
        for (int nj = 0; nj < 4; ++nj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = nb + 16 * nj + 4 * (lane >> 4) + r;
                const float b = (EPI != EPI_V_T && p.bias != nullptr && n < p.N) ? p.bias[n] : 0.f;
#pragma unroll
                for (int mi = 0; mi < 8; ++mi) acc[nj][mi][r] = b;
            }
    }

    using V8 = typename Op<T>::v8;
    struct Frags {  // one K half: 4 column blocks, 4 of the 8 row blocks (hm = 0: rows 0..63, 1: rows 64..127)
        V8 w[4], a[4];
    };
    // step ks = 0..3: K half ks >> 1, row blocks 4 (ks & 1) .. + 3
    auto read_frags = [&](Frags& f, const char* sb, int ks) {
        const int kh = ks >> 1, hm = ks & 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) f.w[j] = *reinterpret_cast<const V8*>(sb + w_off + j * 2048 + xo[kh]);
#pragma unroll
        for (int i = 0; i < 4; ++i) f.a[i] = *reinterpret_cast<const V8*>(sb + a_off + (4 * hm + i) * 2048 + xo[kh]);
    };
    auto mma8 = [&](const Frags& f, int ks) {
        const int hm = ks & 1;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f32x4& c = acc[j][4 * hm + i];
                if constexpr (EPI == EPI_V_T)  // lane owns 4 consecutive tokens of one channel
                    c = Op<T>::mma16(f.a[i], f.w[j], c);
                else  // lane owns 4 consecutive channels of one token
                    c = Op<T>::mma16(f.w[j], f.a[i], c);
            }
    };

    // Software pipeline: the fragments of k-slice s+1 are requested from the LDS BEFORE the 8 MFMAs
    // of slice s are issued (two register sets), and the first slice of the NEXT tile is requested
    // right after the tile barrier, in front of the last 8 MFMAs of the current tile, so LDS
    // latency and the barrier skew hide behind matrix work instead of idling the pipe.
    const int nk = p.K / G_BK;
    Frags f0, f1;
    stage(0, 0);
    wait_vmcnt0();
    __syncthreads();
    read_frags(f0, smem, 0);

    // `arrived(f)` is an empty asm that "uses" the fragment registers: hipcc places the LDS wait
    // (lgkmcnt) in front of it, i.e. BEFORE the next slice's reads are issued, when only the needed
    // reads are outstanding (it otherwise waits for the just-issued prefetch as well).
    auto arrived = [&](Frags& f) {
        asm volatile("" : "+v"(f.w[0]), "+v"(f.w[1]), "+v"(f.w[2]), "+v"(f.w[3]), "+v"(f.a[0]), "+v"(f.a[1]), "+v"(f.a[2]), "+v"(f.a[3]));
        __builtin_amdgcn_sched_barrier(0);
    };
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nk;
        // The LDS-DMA instructions of the next tile are spread over the MFMA groups (2, 1, 1, 0 parts in front of
        // group 0..3): a burst of all 64 per CU at the top of the K step parks every wave in the memory-issue queue
        // while the matrix pipe idles.
        auto stage_some = [&](int first, int count) {
            if (more) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j >= first && j < first + count) stage_part(cur ^ 1, kt + 1, j);
            }
        };
        const char* sb = smem + cur * G_STAGE_BYTES;
        arrived(f0);
        read_frags(f1, sb, 1);
        stage_some(0, 2);
        __builtin_amdgcn_sched_barrier(0);
        mma8(f0, 0);
        __builtin_amdgcn_sched_barrier(0);
        arrived(f1);
        read_frags(f0, sb, 2);
        stage_some(2, 1);
        __builtin_amdgcn_sched_barrier(0);
        mma8(f1, 1);
        __builtin_amdgcn_sched_barrier(0);
        arrived(f0);
        read_frags(f1, sb, 3);
        stage_some(3, 1);
        __builtin_amdgcn_sched_barrier(0);
        mma8(f0, 2);
        __builtin_amdgcn_sched_barrier(0);
        arrived(f1);
        wait_vmcnt0();     // next tile has landed (issued one whole K step ago)
        __syncthreads();   // ... for every wave, and every wave is done reading this buffer
        read_frags(f0, smem + (cur ^ 1) * G_STAGE_BYTES, 0);  // (harmless stale read after the last tile)
        __builtin_amdgcn_sched_barrier(0);
        mma8(f1, 3);
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();  // all MFMA operands consumed before the LDS is reused by the epilogue

    epilogue8m<T, EPI, false>(p, acc, 0, m0 + wm * 128, n0 + wn * 64, lane, smem + wave * 16384, 0, 0, 0);
}

// --------------------------------------------------------------------------------------------
// generic kernel: 64 x 64 x 32, any M, N; K % 32 == 0
// --------------------------------------------------------------------------------------------
constexpr int S_ROW = 80;  // bytes per LDS row: 32 elements (64 B) + 16 B pad

template <typename T, int EPI>
__global__ __launch_bounds__(256) void gemm64_kernel(GemmArgs p) {
    __shared__ __attribute__((aligned(16))) char sA[64 * S_ROW];
    __shared__ __attribute__((aligned(16))) char sW[64 * S_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tiles_n = (p.N + 63) / 64;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
    const int m0 = tm * 64, n0 = tn * 64;
    const T* __restrict__ A = reinterpret_cast<const T*>(p.A);
    const T* __restrict__ W = reinterpret_cast<const T*>(p.W);
    using V8 = typename Op<T>::v8;

    const int lr = tid >> 2, lc = tid & 3;  // 64 rows x 4 chunks of 8 elements
    const T* ga = A + (size_t)min(m0 + lr, p.M - 1) * p.K + lc * 8;
    const T* gw = W + (size_t)min(n0 + lr, p.N - 1) * p.K + lc * 8;

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    const int nk = p.K / 32;
    for (int kt = 0; kt < nk; ++kt) {
        const V8 va = *reinterpret_cast<const V8*>(ga + kt * 32);
        const V8 vw = *reinterpret_cast<const V8*>(gw + kt * 32);
        __syncthreads();
        *reinterpret_cast<V8*>(sA + lr * S_ROW + lc * 16) = va;
        *reinterpret_cast<V8*>(sW + lr * S_ROW + lc * 16) = vw;
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int off = (lane & 31) * S_ROW + ks * 32 + (lane >> 5) * 16;
            const V8 wf = *reinterpret_cast<const V8*>(sW + wn * 32 * S_ROW + off);
            const V8 af = *reinterpret_cast<const V8*>(sA + wm * 32 * S_ROW + off);
            acc = Op<T>::mma(wf, af, acc);
        }
    }

    const int h = lane >> 5;
    const int m = m0 + wm * 32 + (lane & 31);
    if (m >= p.M) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int n = n0 + wn * 32 + mfma32_row(r, h);
        if (n >= p.N) continue;
        float v = acc[r] + (p.bias ? p.bias[n] : 0.f);
        if constexpr (EPI == EPI_GELU_T || EPI == EPI_GELU_F32) v = gelu_erf(v);
        const size_t o = (size_t)m * p.N + n;
        if constexpr (EPI == EPI_STORE_T || EPI == EPI_GELU_T)
            reinterpret_cast<T*>(p.out)[o] = Op<T>::from(v);
        else if constexpr (EPI == EPI_RESID_F32)
            reinterpret_cast<float*>(p.out)[o] += v;
        else
            reinterpret_cast<float*>(p.out)[o] = v;
    }
}

// --------------------------------------------------------------------------------------------
// host launchers
// --------------------------------------------------------------------------------------------
template <typename T, int EPI>
static hipError_t launch_fast(const GemmArgs& p, hipStream_t st) {
    static bool attr_set = false;
    auto kern = gemm256_kernel<T, EPI>;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, G_LDS_BYTES);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    const int tiles = ((p.M + G_BM - 1) / G_BM) * ((p.N + G_BN - 1) / G_BN);
    hipLaunchKernelGGL(kern, dim3(tiles), dim3(512), G_LDS_BYTES, st, p);
    return hipGetLastError();
}

template <typename T, int EPI>
static hipError_t launch_generic(const GemmArgs& p, hipStream_t st) {
    const int tiles = ((p.M + 63) / 64) * ((p.N + 63) / 64);
    hipLaunchKernelGGL((gemm64_kernel<T, EPI>), dim3(tiles), dim3(256), 0, st, p);
    return hipGetLastError();
}

// Which of the two tile kernels takes a dense call: 256, 64, or 0 = neither (gemm_plan asks; the launchers re-check).
int gemm_tile_kernel(const GemmArgs& p, int epi) {
    const bool fast = (p.K % G_BK == 0) && (p.N % 8 == 0) && !p.force_generic;
    if (epi == EPI_QKV_ROPE || epi == EPI_V_T) return (fast && p.N % 64 == 0) ? 256 : 0;
    if (epi < EPI_STORE_T || epi > EPI_RESID_F32) return 0;
    return fast ? 256 : (p.K % 32 == 0 ? 64 : 0);
}

template <typename T>
static hipError_t dispatch256(const GemmArgs& p, int epi, hipStream_t st) {
    switch (epi) {
        case EPI_STORE_T: return launch_fast<T, EPI_STORE_T>(p, st);
        case EPI_STORE_F32: return launch_fast<T, EPI_STORE_F32>(p, st);
        case EPI_GELU_T: return launch_fast<T, EPI_GELU_T>(p, st);
        case EPI_GELU_F32: return launch_fast<T, EPI_GELU_F32>(p, st);
        case EPI_RESID_F32: return launch_fast<T, EPI_RESID_F32>(p, st);
        case EPI_QKV_ROPE: return launch_fast<T, EPI_QKV_ROPE>(p, st);
        case EPI_V_T: return launch_fast<T, EPI_V_T>(p, st);
    }
    return hipErrorInvalidValue;
}

template <typename T>
static hipError_t dispatch64(const GemmArgs& p, int epi, hipStream_t st) {
    switch (epi) {
        case EPI_STORE_T: return launch_generic<T, EPI_STORE_T>(p, st);
        case EPI_STORE_F32: return launch_generic<T, EPI_STORE_F32>(p, st);
        case EPI_GELU_T: return launch_generic<T, EPI_GELU_T>(p, st);
        case EPI_GELU_F32: return launch_generic<T, EPI_GELU_F32>(p, st);
        case EPI_RESID_F32: return launch_generic<T, EPI_RESID_F32>(p, st);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_gemm256(const GemmArgs& p, int epi, int operand_dtype, hipStream_t st) {
    if (gemm_tile_kernel(p, epi) != 256) return hipErrorInvalidValue;
    if (operand_dtype == ESMK_DT_F16) return dispatch256<_Float16>(p, epi, st);
    if (operand_dtype == ESMK_DT_BF16) return dispatch256<__bf16>(p, epi, st);
    return hipErrorInvalidValue;
}

hipError_t launch_gemm64(const GemmArgs& p, int epi, int operand_dtype, hipStream_t st) {
    if (gemm_tile_kernel(p, epi) != 64) return hipErrorInvalidValue;
    if (operand_dtype == ESMK_DT_F16) return dispatch64<_Float16>(p, epi, st);
    if (operand_dtype == ESMK_DT_BF16) return dispatch64<__bf16>(p, epi, st);
    return hipErrorInvalidValue;
}

}  // namespace esmk
