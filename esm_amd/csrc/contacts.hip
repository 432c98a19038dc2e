// contacts.hip — contact maps WITHOUT the [B,L,H,T,T] attention tensor (fused form).
//
// Reference: ESM2.forward collects every layer's head-wise attention weights (esm/model/esm2.py:119-121,
// 132-139; 2.77 GB of fp32 per 1024-token sequence for the 650M model) and hands them to
// ContactPredictionHead.forward (esm/modules.py:338-357): eos mask, crop of the first/last position,
// symmetrize + apc (modules.py:27-41) per channel c = (layer, head), a 1-output regression, sigmoid.
// With m[t] = 1 for residue tokens (not <pad>, not <eos>, not the cropped first/last position) and P_c the
// softmax of channel c, that is
//     logit[i][j] = m_i m_j (A[i][j] + A[j][i]) - sum_c (w_c / t_c) r_c[i] r_c[j] + bias
//     A = sum_c w_c P_c,     r_c[i] = m_i (sum_j m_j P_c[i][j] + sum_j m_j P_c[j][i]),     t_c = sum_i r_c[i]
// so one [T,T] fp32 accumulator per sequence plus the masked row and column sums of every channel are enough.
// `model.predict_contacts(tokens)` (esm2.py:146-147) returns only the map, so the engine takes this path for
// it; `forward(return_contacts=True)` also returns "attentions" and keeps the materialised path
// (elementwise.hip: contact_sums_kernel / contact_out_kernel).
//
// Per layer, after the flash attention kernel has left q, k (scaled, rotated) and the row log-sum-exp:
//   accumulate  re-computes S = q k^T in 32x32 MFMA blocks, P = exp(S + key_bias - lse), and adds w_c P into A,
//               partial masked row / column sums into rowp / colp (no atomics: every output element has exactly
//               one writer, so the result is deterministic);
//   reduce      sums the partials in a fixed order into rowsum[c,:] and colsum[c,:].
// After the last layer: rt (r_c, w_c / t_c) and final (the formula above).
//
// Each of the five computations is written ONCE, as a force-inlined body in the coordinates of one sequence: its
// pointers already point at that sequence, and the two layouts differ only in two strides (the rows between the
// heads of q / k / lse, the elements between the head-group accumulators).  Every computation has two __global__
// wrappers that decode the workgroup id and move the pointers:
//   padded  contact_*_kernel          [B,H,T,.] batch, id -> (head group, b, key chunk, query block) / blockIdx
//   packed  contact_*_packed_kernel   token-packed batch (esmk_forward_packed_ex), id -> an item of the launch's
//                                     work list; Tlen = the segment's length, so every chunk and block boundary,
//                                     and with them the sums, are the ones of the sequence run alone.
#include <algorithm>
#include <vector>

#include "common.h"
#include "kernels.h"

namespace esmk {

namespace {

template <int CTRL>
ESMK_DEV float dpp_add(float v) {
    const int t = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true);
    return v + __builtin_bit_cast(float, t);
}
// sum over the 16 lanes of a DPP row, result in every lane of the row
ESMK_DEV float row16_sum(float v) {
    v = dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]
    v = dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]
    v = dpp_add<0x141>(v);  // row_half_mirror
    v = dpp_add<0x140>(v);  // row_mirror
    return v;
}

// v[lane] + v[lane ^ 32] in every lane: v_permlane32_swap_b32 exchanges the upper half of its first operand with
// the lower half of its second one (a VALU op; __shfl_xor goes through the LDS crossbar and an lgkmcnt wait)
ESMK_DEV float half_swap_sum(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// residue mask of token position t of one sequence (modules.py:340-347 + the pad mask of esm2.py:135-139)
ESMK_DEV float residue_mask(const int64_t* tok, int t, int Tlen, int pad_idx, int eos_idx, int bos, int eos) {
    if (t < bos || t >= Tlen - eos) return 0.f;
    const long long v = tok[t];
    return (v == pad_idx || (eos && v == eos_idx)) ? 0.f : 1.f;
}

// ---- prologues of the accumulate kernels: workgroup id -> (head group g, key chunk, query block) of one sequence,
// the pointers moved to it: q, k, lse to head 0 of the sequence (heads are `hstride` rows apart), key_bias and
// tokens to its first position, acc to head group g's [Tlen,Tlen] accumulator, rowp / colp to its partials.
// padded batch: (g, b, chunk, qblock), qblock fastest; q, k [B,H,T,HD], acc [G][B,T,T], rowp [B,nQ,H,T], colp [B,nP,H,T]
template <int HD, typename T>
ESMK_DEV void ct_padded_item(int B, int H, int Tlen, int id, int& g, int& kci, int& qb, size_t& hstride,
                             const T* __restrict__& q, const T* __restrict__& k, const float* __restrict__& lse,
                             const float* __restrict__& key_bias, const int64_t* __restrict__& tokens,
                             float* __restrict__& acc, float* __restrict__& rowp, float* __restrict__& colp) {
    const int nQ = (Tlen + 127) >> 7, nP = (Tlen + 31) >> 5;  // query blocks == key chunks
    qb = id % nQ;
    id /= nQ;
    kci = id % nQ;
    id /= nQ;
    const int b = id % B;
    g = id / B;
    hstride = (size_t)Tlen;
    q += (size_t)b * H * Tlen * HD;
    k += (size_t)b * H * Tlen * HD;
    lse += (size_t)b * H * Tlen;
    if (key_bias != nullptr) key_bias += (size_t)b * Tlen;
    tokens += (size_t)b * Tlen;
    acc += ((size_t)g * B + b) * Tlen * Tlen;
    rowp += (size_t)b * nQ * H * Tlen;
    colp += (size_t)b * nP * H * Tlen;
}

// token-packed batch: work item id % n_items of cs.work = (segment, key chunk, query block), head group id / n_items;
// q, k, lse are [H, cs.rows, .], the G accumulators [G][cs.acc_stride]; Tlen becomes the segment's length
template <int HD, typename T>
ESMK_DEV void ct_packed_item(const CtSegs& cs, int id, int& g, int& kci, int& qb, int& Tlen, size_t& hstride,
                             const T* __restrict__& q, const T* __restrict__& k, const float* __restrict__& lse,
                             const float* __restrict__& key_bias, const int64_t* __restrict__& tokens,
                             float* __restrict__& acc, float* __restrict__& rowp, float* __restrict__& colp) {
    const int it = id % cs.n_items;
    g = id / cs.n_items;
    const int s = __builtin_amdgcn_readfirstlane(cs.work[4 * it]);
    kci = __builtin_amdgcn_readfirstlane(cs.work[4 * it + 1]);
    qb = __builtin_amdgcn_readfirstlane(cs.work[4 * it + 2]);
    const int row0 = __builtin_amdgcn_readfirstlane(cs.seg[2 * s]);
    Tlen = __builtin_amdgcn_readfirstlane(cs.seg[2 * s + 1]);
    hstride = (size_t)cs.rows;
    const long long* off = cs.off + 4 * (size_t)s;
    q += (size_t)row0 * HD;
    k += (size_t)row0 * HD;
    lse += row0;
    if (key_bias != nullptr) key_bias += row0;
    tokens += row0;
    acc += (size_t)g * cs.acc_stride + off[0];
    rowp += off[1];
    colp += off[2];
}

// ---- accumulate, direct-load form (head_dim 128) ----------------------------------------------------------------
// One workgroup of 4 waves = (head group g, 128-key chunk kci, 128-query block qb) of one sequence; wave w owns
// queries [q0, q0 + 32), q0 = 128 qb + 32 w, times the chunk's 128 keys (4 accumulator blocks = 64 VGPRs) with the
// group's heads as the loop, so the w_c-weighted sum over those heads is formed in registers and A is
// read-modified-written once per layer by exactly one wave per element.  MFMA orientation as in attn_probs_rows:
// D[row = query][col = key], lane & 31 = key, register = query row.  Masks are folded into the exponent: a masked
// query row gets lse = +inf, a masked key bias = -inf, so their probabilities are exact zeros in A and in both sums
// (the final formula multiplies by m_i m_j anyway).  K fragments are fetched one block ahead (register double
// buffer) to cover the L2 latency.  The partial sums are parked in wave-private LDS and written after the last
// load: on gfx9 stores share the in-order vmcnt counter with loads, so a store between two prefetches puts its HBM
// write-acknowledge latency (~2 us) on the critical path of every block (measured: 71 % of the wave cycles parked
// in s_waitcnt, profiles/r1_v19_*).
// Outputs per layer: A += sum_{h in g} w P_h;  rowp[chunk, h, q] partial row sums;  colp[q0/32, h, key] partial
// column sums.  Every element has one writer.
template <typename T, int HD>
ESMK_DEV void contact_accum_seq(const T* __restrict__ q, const T* __restrict__ k, const float* __restrict__ lse,
                                const float* __restrict__ key_bias, const int64_t* __restrict__ tok,
                                const float* __restrict__ wreg, float* __restrict__ A, float* __restrict__ rowp,
                                float* __restrict__ colp, int H, int Tlen, size_t hstride, int layer, int G, int g,
                                int kci, int qb, int pad_idx, int eos_idx, int bos, int eos) {
    // per wave and head of the group: lse (log2 domain, as q.k is: attention.hip) of the 32 queries, 128 column sums, 2 x 32 row sums
    extern __shared__ float s_dyn[];
    using V8 = typename Op<T>::v8;
    constexpr int KS = HD / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hh = lane >> 5, lm = lane & 31;
    // element (head hd, position t) of the row spaces of q, k and lse
    auto hrow = [&](int hd, int t) -> size_t {
        return (size_t)hd * hstride + t;
    };
    const int hg = (H + G - 1) / G;  // heads per group
    const int h0 = g * hg, h1 = min(H, h0 + hg);
    const int q0 = qb * 128 + wave * 32, kc = kci * 128;
    if (q0 >= Tlen || h0 >= h1) return;  // no barriers below: waves are independent
    float* s_lse = s_dyn + wave * (hg * 224);
    float* s_col = s_lse + hg * 32;
    float* s_row = s_col + hg * 128;

    for (int idx = lane; idx < (h1 - h0) * 32; idx += 64) {
        const int hd = h0 + (idx >> 5), qq = q0 + (idx & 31);
        const bool keep = qq < Tlen && residue_mask(tok, qq, Tlen, pad_idx, eos_idx, bos, eos) != 0.f;
        s_lse[idx] = keep ? lse[hrow(hd, qq)] : __builtin_inff();  // lse is log2-domain
    }
    float kb2[4];  // key bias in the exp2 domain: 0, or -inf for <pad> / masked / out-of-range keys
    int krow[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int key = kc + jj * 32 + lm;
        krow[jj] = min(key, Tlen - 1);
        const bool keep = key < Tlen && residue_mask(tok, key, Tlen, pad_idx, eos_idx, bos, eos) != 0.f;
        kb2[jj] = keep ? (key_bias != nullptr ? key_bias[key] : 0.f) : -__builtin_inff();
    }
    const int qr = min(q0 + lm, Tlen - 1);
    const int nblk = min(4, (Tlen - kc + 31) >> 5);  // key blocks of this chunk that hold a key (wave uniform)

    f32x16 acc[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[jj][r] = 0.f;

    auto load_k = [&](V8 (&kf)[KS], int hd, int jj) {
        const T* kp = k + hrow(hd, krow[jj]) * HD + 8 * hh;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[ks] = *reinterpret_cast<const V8*>(kp + 16 * ks);
    };
    auto load_q = [&](V8 (&qf)[KS], int hd) {
        const T* qp = q + hrow(hd, qr) * HD + 8 * hh;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const V8*>(qp + 16 * ks);
    };
    V8 qf[KS], qn[KS], kf[KS], kn[KS];
    load_q(qf, h0);
    load_k(kf, h0, 0);
    for (int hd = h0; hd < h1; ++hd) {
        const int hn = min(hd + 1, h1 - 1);
        load_q(qn, hn);  // next head's queries: a whole head of lead time
        float cr[16], rs[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            cr[r] = -s_lse[(hd - h0) * 32 + mfma32_row(r, hh)];
            rs[r] = 0.f;
        }
        const float wl = wreg[layer * H + hd];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            // fetch the next block's K rows (next head's block 0 after the last block)
            if (jj + 1 < 4) load_k(kn, hd, jj + 1);
            else load_k(kn, hn, 0);
            if (jj < nblk) {
                f32x16 s;
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) s = Op<T>::mma(qf[ks], kf[ks], s);
                float cs = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    // 2^(s + key_bias - lse) with log2-domain scores; -inf + (-(+inf)) stays -inf -> 0
                    const float p = __builtin_amdgcn_exp2f(s[r] + cr[r] + kb2[jj]);
                    acc[jj][r] = __builtin_fmaf(wl, p, acc[jj][r]);
                    rs[r] += p;
                    cs += p;
                }
                cs += __shfl_xor(cs, 32, 64);  // the two lane halves hold different query rows of one key
                if (hh == 0) s_col[(hd - h0) * 128 + jj * 32 + lm] = cs;
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) kf[ks] = kn[ks];
        }
        // row sums over this chunk's keys: reduce over the 16 lanes of each DPP row; the two rows of a lane half
        // go to two partial slots
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = row16_sum(rs[r]);
            if ((lane & 15) == 0) s_row[((hd - h0) * 2 + ((lane >> 4) & 1)) * 32 + mfma32_row(r, hh)] = v;
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = qn[ks];
    }
    // every load of the main loop has retired: now the stores
    for (int idx = lane; idx < (h1 - h0) * 128; idx += 64) {
        const int key = kc + (idx & 127);
        if (key < Tlen) colp[((size_t)(q0 >> 5) * H + h0 + (idx >> 7)) * Tlen + key] = s_col[idx];
    }
    for (int idx = lane; idx < (h1 - h0) * 32; idx += 64) {  // the two 16-lane slots of a row are summed here
        const int qq = q0 + (idx & 31), hl = idx >> 5;
        if (qq < Tlen)
            rowp[((size_t)kci * H + h0 + hl) * Tlen + qq] =
                s_row[(hl * 2) * 32 + (idx & 31)] + s_row[(hl * 2 + 1) * 32 + (idx & 31)];
    }
    float* arow = A + (size_t)(q0 + 4 * hh) * Tlen;  // query row q0 + mfma32_row(r, hh) = this + a wave-uniform offset
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int key = kc + jj * 32 + lm;
        if (key < Tlen) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qrow = q0 + mfma32_row(r, hh);
                if (qrow < Tlen) {
                    float* a = arow + (size_t)mfma32_row(r, 0) * Tlen + key;
                    *a = (layer == 0 ? 0.f : *a) + acc[jj][r];
                }
            }
        }
    }
}

// ---- accumulate, head_dim 64 (every model but the 15B) ----------------------------------------------------------
// The same computation with the K chunk of a head staged ONCE per workgroup through the LDS.  The direct fragment
// loads above touch 32 different 128-byte lines per instruction (a lane reads 16 bytes of "its" key row), which
// makes the texture-address path the bottleneck (measured: 71 % of the wave cycles parked, 1.2 ms per layer at
// B = 64 where the VALU work is 0.2 ms).  Here 256 threads copy the chunk's 128 rows x 128 B with 4 coalesced
// global_load_lds each (XOR-swizzled 16-byte slots, the layout of attn_fwd_kernel), double buffered across heads
// with one barrier per head; fragments come from ds_read_b128.  The partial sums are parked per slab of PARK heads,
// so the LDS budget (67 KiB: two workgroups per CU) does not depend on the number of heads.
template <typename T>
ESMK_DEV void contact_accum64_seq(const T* __restrict__ q, const T* __restrict__ k, const float* __restrict__ lse,
                                  const float* __restrict__ key_bias, const int64_t* __restrict__ tok,
                                  const float* __restrict__ wreg, float* __restrict__ A, float* __restrict__ rowp,
                                  float* __restrict__ colp, int H, int Tlen, size_t hstride, int layer, int G, int g,
                                  int kci, int qb, int pad_idx, int eos_idx, int bos, int eos) {
    extern __shared__ __attribute__((aligned(16))) char s_raw[];
    using V8 = typename Op<T>::v8;
    constexpr int PARK = 10, KBUF = 128 * 128;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hh = lane >> 5, lm = lane & 31;
    auto hrow = [&](int hd, int t) -> size_t {  // row spaces of q, k and lse
        return (size_t)hd * hstride + t;
    };
    const int hg = (H + G - 1) / G;
    const int h0 = g * hg, h1 = min(H, h0 + hg);
    if (h0 >= h1) return;  // workgroup uniform
    const int q0 = qb * 128 + wave * 32, kc = kci * 128;
    const bool active = q0 < Tlen;  // wave uniform; inactive waves still stage K and meet the barriers
    char* s_k = s_raw;
    float* s_lse = reinterpret_cast<float*>(s_raw + 2 * KBUF) + wave * (PARK * 224);
    float* s_col = s_lse + PARK * 32;
    float* s_row = s_col + PARK * 128;

    // K staging: position pos = 256 j + tid of the chunk image = (row pos / 8, 16-byte slot pos % 8)
    size_t ksrc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pos = j * 256 + tid;
        const int r = pos >> 3, sl = pos & 7;
        ksrc[j] = (size_t)min(kc + r, Tlen - 1) * 64 + (sl ^ ((r >> 1) & 7)) * 8;
    }
    auto stage = [&](int buf, int hd) {
        const T* kh = k + (size_t)hd * hstride * 64;
#pragma unroll
        for (int j = 0; j < 4; ++j) glds16(kh + ksrc[j], s_k + buf * KBUF + (j * 256 + wave * 64) * 16);
    };
    int xo[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) xo[ks] = lm * 128 + (((2 * ks + hh) ^ ((lane >> 1) & 7)) << 4);

    // key bias (0 / -inf for <pad>), -inf for masked and out-of-range keys: the score accumulators START from it,
    // so the MFMA chain delivers s + bias and the masking costs no VALU work
    float kbr[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int key = kc + jj * 32 + lm;
        const bool keep = key < Tlen && residue_mask(tok, key, Tlen, pad_idx, eos_idx, bos, eos) != 0.f;
        kbr[jj] = keep ? (key_bias != nullptr ? key_bias[key] : 0.f) : -__builtin_inff();
    }
    const int qr = min(q0 + lm, Tlen - 1);
    const int nblk = min(4, (Tlen - kc + 31) >> 5);
    const bool qkeep = q0 + lm < Tlen && residue_mask(tok, q0 + lm, Tlen, pad_idx, eos_idx, bos, eos) != 0.f;
    // does the wave's 128-key chunk hold a masked key (<cls>, <eos>, a pad, the sequence end)?  wave uniform, the same
    // for every head: 6 of the 8 chunks of a full-length sequence do not
    const unsigned masked_blocks = __builtin_amdgcn_readfirstlane(
        __builtin_amdgcn_ballot_w64(kbr[0] != 0.f || kbr[1] != 0.f || kbr[2] != 0.f || kbr[3] != 0.f) != 0 ? 1u : 0u);

    // fp32 VALU instructions take 4 cycles per wave on gfx950 (PMC: 4.5 cycles per VALU instruction in this kernel)
    // and the packed forms process two values in the same 4: the per-score arithmetic is written on float pairs
    f32x2 acc[4][8];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[jj][i] = f32x2{0.f, 0.f};
    auto load_q = [&](V8 (&qf)[4], int hd) {
        const T* qp = q + hrow(hd, qr) * 64 + 8 * hh;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const V8*>(qp + 16 * ks);
    };
    V8 qf[4], qn[4];
    stage(0, h0);
    load_q(qf, h0);
    int cur = 0;
    for (int hs = h0; hs < h1; hs += PARK) {  // slab of heads whose partial sums are parked in the LDS
        const int he = min(h1, hs + PARK);
        if (active) {
            for (int idx = lane; idx < (he - hs) * 32; idx += 64) {
                // lane idx & 31 == lm for both halves: qkeep is the mask of query q0 + (idx & 31)
                const int qq = min(q0 + (idx & 31), Tlen - 1);
                const float v = lse[hrow(hs + (idx >> 5), qq)];  // log2 domain
                s_lse[idx] = qkeep ? -v : -__builtin_inff();  // stored NEGATED: it is the start value of the score accumulators
            }
        }
        for (int hd = hs; hd < he; ++hd) {
            wait_vmcnt0();    // this thread's share of head hd's chunk has landed
            __syncthreads();  // ... everybody's has, and nobody reads the other buffer any more
            if (hd + 1 < h1) stage(cur ^ 1, hd + 1);
            if (active) {
                const char* sk = s_k + cur * KBUF;
                load_q(qn, min(hd + 1, h1 - 1));
                // -lse of the 16 query rows this lane holds (a masked query: -inf, its row comes out as exact zeros).  The
                // score accumulators of every block START from it — one set of 16 registers per head, kept intact by
                // the early-clobber MFMA of common.h — so a score leaves the matrix pipe as s - lse: no 16 v_mov per
                // block to seed the accumulator, no packed add per score pair.  The key bias (0 / -inf) is added
                // afterwards, and only by waves whose chunk holds a masked key.
                f32x16 nlse;
                f32x2 rs[8];
#pragma unroll
                for (int r = 0; r < 16; ++r) nlse[r] = s_lse[(hd - hs) * 32 + mfma32_row(r, hh)];
#pragma unroll
                for (int i = 0; i < 8; ++i) rs[i] = f32x2{0.f, 0.f};
                const float wl = wreg[layer * H + hd];
                const f32x2 wl2 = f32x2{wl, wl};
                // two copies of the block loop, chosen per wave: hipcc turns a per-block "add the key bias if the block
                // has a masked key" into 16 v_cndmask per block, which costs more than it saves
                auto blocks = [&](auto any_masked_c) {
                    constexpr bool ANY_MASKED = decltype(any_masked_c)::value;
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        if (jj < nblk) {  // wave uniform
                            f32x16 s = Op<T>::mma_keep_c(qf[0], *reinterpret_cast<const V8*>(sk + jj * 4096 + xo[0]), nlse);
#pragma unroll
                            for (int ks = 1; ks < 4; ++ks) {
                                const V8 kf = *reinterpret_cast<const V8*>(sk + jj * 4096 + xo[ks]);
                                s = Op<T>::mma(qf[ks], kf, s);
                            }
                            f32x2 cs2 = f32x2{0.f, 0.f};
#pragma unroll
                            for (int i = 0; i < 8; ++i) {
                                // 2^(s + key_bias - lse) with log2-domain scores; -inf stays -inf -> 0
                                f32x2 t = f32x2{s[2 * i], s[2 * i + 1]};
                                if constexpr (ANY_MASKED) t += f32x2{kbr[jj], kbr[jj]};
                                const f32x2 p = f32x2{__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
                                acc[jj][i] = __builtin_elementwise_fma(wl2, p, acc[jj][i]);
                                rs[i] += p;
                                cs2 += p;
                            }
                            const float cs = half_swap_sum(cs2[0] + cs2[1]);  // the lane halves hold different query rows
                            if (hh == 0) s_col[(hd - hs) * 128 + jj * 32 + lm] = cs;
                        }
                    }
                };
                if (masked_blocks == 0) blocks(std::false_type{});
                else blocks(std::true_type{});
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = row16_sum(rs[r >> 1][r & 1]);
                    if ((lane & 15) == 0) s_row[((hd - hs) * 2 + ((lane >> 4) & 1)) * 32 + mfma32_row(r, hh)] = v;
                }
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) qf[ks] = qn[ks];
            }
            cur ^= 1;
        }
        if (active) {
            for (int idx = lane; idx < (he - hs) * 128; idx += 64) {
                const int key = kc + (idx & 127);
                if (key < Tlen) colp[((size_t)(q0 >> 5) * H + hs + (idx >> 7)) * Tlen + key] = s_col[idx];
            }
            for (int idx = lane; idx < (he - hs) * 32; idx += 64) {  // the two 16-lane slots of a row are summed here
                const int qq = q0 + (idx & 31), hl = idx >> 5;
                if (qq < Tlen)
                    rowp[((size_t)kci * H + hs + hl) * Tlen + qq] =
                        s_row[(hl * 2) * 32 + (idx & 31)] + s_row[(hl * 2 + 1) * 32 + (idx & 31)];
            }
        }
    }
    if (!active) return;
    float* arow = A + (size_t)(q0 + 4 * hh) * Tlen;  // query row q0 + mfma32_row(r, hh) = this + a wave-uniform offset
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int key = kc + jj * 32 + lm;
        if (key < Tlen) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qrow = q0 + mfma32_row(r, hh);
                if (qrow < Tlen) {
                    float* a = arow + (size_t)mfma32_row(r, 0) * Tlen + key;
                    *a = (layer == 0 ? 0.f : *a) + acc[jj][r >> 1][r & 1];
                }
            }
        }
    }
}

// ---- reduce: rowsum[layer*H + hd, t] = sum of the nR = ceil(T/128) row partials, colsum[...] = sum of the
// nP = ceil(T/32) column partials, both in index order (deterministic); rowsum / colsum [C, Tlen] of the sequence
ESMK_DEV void contact_reduce_seq(const float* __restrict__ rowp, const float* __restrict__ colp,
                                 float* __restrict__ rowsum, float* __restrict__ colsum, int H, int Tlen, int layer,
                                 int nR, int nP, int hd, int t) {
    if (t >= Tlen) return;
    float s = 0.f;
    for (int p = 0; p < nR; ++p) s += rowp[((size_t)p * H + hd) * Tlen + t];
    rowsum[((size_t)layer * H + hd) * Tlen + t] = s;
    s = 0.f;
    for (int p = 0; p < nP; ++p) s += colp[((size_t)p * H + hd) * Tlen + t];
    colsum[((size_t)layer * H + hd) * Tlen + t] = s;
}

// ---- rt: one workgroup per channel c of a sequence: r = m (rowsum + colsum) written over rowsum,
// wt[c] = w_c / sum_i r[i]
ESMK_DEV void contact_rt_seq(float* __restrict__ rowsum, const float* __restrict__ colsum,
                             const int64_t* __restrict__ tok, const float* __restrict__ wreg, float* __restrict__ wt,
                             int Tlen, int c, int pad_idx, int eos_idx, int bos, int eos) {
    __shared__ float s_w[4];
    float tot = 0.f;
    for (int i = threadIdx.x; i < Tlen; i += 256) {
        const size_t o = (size_t)c * Tlen + i;
        const float r = residue_mask(tok, i, Tlen, pad_idx, eos_idx, bos, eos) * (rowsum[o] + colsum[o]);
        rowsum[o] = r;
        tot += r;
    }
    tot = wave_sum(tot);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = tot;
    __syncthreads();
    // no residue at all: 0/0 like the reference's apc (modules.py:36-38)
    if (threadIdx.x == 0) wt[c] = wreg[c] / ((s_w[0] + s_w[1]) + (s_w[2] + s_w[3]));
}

// ---- final: 32 x 32 output tile (i0, j0) per workgroup (cropped coordinates i, j in [0,S); token position = i + bos).
// A is the sum of the G head-group accumulators, `gstride` elements apart; the rank-C apc term runs over LDS-staged
// slabs of 32 channels.  r [C, Tlen], wt [C] and out [S, S] are the sequence's.
ESMK_DEV void contact_final_seq(const float* __restrict__ A, const float* __restrict__ rb,
                                const float* __restrict__ wb, const int64_t* __restrict__ tok,
                                const float* __restrict__ bias, float* __restrict__ out, int G, int C, int Tlen,
                                size_t gstride, int i0, int j0, int pad_idx, int eos_idx, int bos, int eos) {
    __shared__ float s_t[32][33];
    __shared__ float s_ri[32][33], s_rj[32][33];
    const int S = Tlen - bos - eos;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {  // mirrored tile A[j][i], read coalesced along i
        const int j = j0 + ty + 8 * kq, i = i0 + tx;
        float v = 0.f;
        if (j < S && i < S)
            for (int g = 0; g < G; ++g) v += A[g * gstride + (size_t)(j + bos) * Tlen + i + bos];
        s_t[ty + 8 * kq][tx] = v;
    }
    __syncthreads();
    const int jc = min(j0 + tx, S - 1) + bos;
    const int it = min(i0 + tx, S - 1) + bos;
    const float mj = (j0 + tx < S) ? residue_mask(tok, jc, Tlen, pad_idx, eos_idx, bos, eos) : 0.f;
    float sym[4], apc[4];
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
        const int i = i0 + ty + 8 * kq;
        const int ic = min(i, S - 1) + bos;
        const float mi = (i < S) ? residue_mask(tok, ic, Tlen, pad_idx, eos_idx, bos, eos) : 0.f;
        float v = 0.f;
        if (i < S && j0 + tx < S)
            for (int g = 0; g < G; ++g) v += A[g * gstride + (size_t)ic * Tlen + jc];
        sym[kq] = (v + s_t[tx][ty + 8 * kq]) * mi * mj;
        apc[kq] = 0.f;
    }
    for (int c0 = 0; c0 < C; c0 += 32) {
        __syncthreads();
#pragma unroll
        for (int kq = 0; kq < 4; ++kq) {  // channel c0 + ty + 8 kq: r[i0 + tx] and (w/t) r[j0 + tx]
            const int c = c0 + ty + 8 * kq;
            const bool ok = c < C;
            const float* rc = rb + (size_t)(ok ? c : 0) * Tlen;
            s_ri[ty + 8 * kq][tx] = ok ? rc[it] : 0.f;
            s_rj[ty + 8 * kq][tx] = ok ? wb[c] * rc[jc] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int cc = 0; cc < 32; ++cc) {
            const float f = s_rj[cc][tx];
#pragma unroll
            for (int kq = 0; kq < 4; ++kq) apc[kq] += f * s_ri[cc][ty + 8 * kq];
        }
    }
    const float bb = bias ? bias[0] : 0.f;
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
        const int i = i0 + ty + 8 * kq, j = j0 + tx;
        if (i < S && j < S) {
            const float z = sym[kq] - apc[kq] + bb;
            out[(size_t)i * S + j] = 1.0f / (1.0f + expf(-z));
        }
    }
}

}  // namespace

// ---- padded batch: the wrappers ---------------------------------------------------------------------------------
// grid: G * B * ceil(T/128) * ceil(T/128) workgroups.  Workgroup ids are XCD-remapped so that the query blocks of
// one (b, chunk) — which read the same K rows — share an L2 (contiguous id ranges per XCD).
template <typename T, int HD>
__global__ __launch_bounds__(256, HD == 128 ? 1 : 2) void contact_accum_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const float* __restrict__ lse,
    const float* __restrict__ key_bias, const int64_t* __restrict__ tokens, const float* __restrict__ wreg,
    float* __restrict__ acc_out, float* __restrict__ rowp, float* __restrict__ colp, int B, int H, int Tlen,
    int layer, int G, int pad_idx, int eos_idx, int bos, int eos) {
    int g, kci, qb;
    size_t hstride;
    ct_padded_item<HD>(B, H, Tlen, xcd_remap(blockIdx.x, gridDim.x), g, kci, qb, hstride, q, k, lse, key_bias, tokens,
                       acc_out, rowp, colp);
    contact_accum_seq<T, HD>(q, k, lse, key_bias, tokens, wreg, acc_out, rowp, colp, H, Tlen, hstride, layer, G, g, kci,
                             qb, pad_idx, eos_idx, bos, eos);
}

template <typename T>
__global__ __launch_bounds__(256, 2) void contact_accum64_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const float* __restrict__ lse,
    const float* __restrict__ key_bias, const int64_t* __restrict__ tokens, const float* __restrict__ wreg,
    float* __restrict__ acc_out, float* __restrict__ rowp, float* __restrict__ colp, int B, int H, int Tlen,
    int layer, int G, int pad_idx, int eos_idx, int bos, int eos) {
    int g, kci, qb;
    size_t hstride;
    ct_padded_item<64>(B, H, Tlen, xcd_remap(blockIdx.x, gridDim.x), g, kci, qb, hstride, q, k, lse, key_bias, tokens,
                       acc_out, rowp, colp);
    contact_accum64_seq<T>(q, k, lse, key_bias, tokens, wreg, acc_out, rowp, colp, H, Tlen, hstride, layer, G, g, kci,
                           qb, pad_idx, eos_idx, bos, eos);
}

// grid: B * H * ceil(T/256); rowp [B,nR,H,T], colp [B,nP,H,T], rowsum / colsum [B,C,T]
__global__ __launch_bounds__(256) void contact_reduce_kernel(const float* __restrict__ rowp,
                                                              const float* __restrict__ colp,
                                                              float* __restrict__ rowsum, float* __restrict__ colsum,
                                                              int H, int Tlen, int C, int layer, int nR, int nP) {
    const int nKb = (Tlen + 255) >> 8;
    const int bh = blockIdx.x / nKb;
    const int t = (blockIdx.x - bh * nKb) * 256 + threadIdx.x;
    const int b = bh / H, hd = bh - b * H;
    contact_reduce_seq(rowp + (size_t)b * nR * H * Tlen, colp + (size_t)b * nP * H * Tlen,
                       rowsum + (size_t)b * C * Tlen, colsum + (size_t)b * C * Tlen, H, Tlen, layer, nR, nP, hd, t);
}

// grid: B * C; wt [B,C]
__global__ __launch_bounds__(256) void contact_rt_kernel(float* __restrict__ rowsum, const float* __restrict__ colsum,
                                                          const int64_t* __restrict__ tokens,
                                                          const float* __restrict__ wreg, float* __restrict__ wt,
                                                          int C, int Tlen, int pad_idx, int eos_idx, int bos, int eos) {
    const int b = blockIdx.x / C, c = blockIdx.x - b * C;
    contact_rt_seq(rowsum + (size_t)b * C * Tlen, colsum + (size_t)b * C * Tlen, tokens + (size_t)b * Tlen, wreg,
                   wt + (size_t)b * C, Tlen, c, pad_idx, eos_idx, bos, eos);
}

// grid: (tile column, tile row, b); acc [G][B,T,T], out [B,S,S]
__global__ __launch_bounds__(256) void contact_final_kernel(const float* __restrict__ acc,
                                                             const float* __restrict__ r,
                                                             const float* __restrict__ wt,
                                                             const int64_t* __restrict__ tokens,
                                                             const float* __restrict__ bias, float* __restrict__ out,
                                                             int B, int G, int C, int Tlen, int pad_idx, int eos_idx,
                                                             int bos, int eos) {
    const int b = blockIdx.z, S = Tlen - bos - eos;
    contact_final_seq(acc + (size_t)b * Tlen * Tlen, r + (size_t)b * C * Tlen, wt + (size_t)b * C,
                      tokens + (size_t)b * Tlen, bias, out + (size_t)b * S * S, G, C, Tlen, (size_t)B * Tlen * Tlen,
                      blockIdx.y * 32, blockIdx.x * 32, pad_idx, eos_idx, bos, eos);
}

// ---- token-packed batch: the wrappers (work lists: contacts_packed_tables) ---------------------------------------
// grid: G * n_items, XCD-remapped like the padded one
template <typename T, int HD>
__global__ __launch_bounds__(256, HD == 128 ? 1 : 2) void contact_accum_packed_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const float* __restrict__ lse,
    const float* __restrict__ key_bias, const int64_t* __restrict__ tokens, const float* __restrict__ wreg,
    float* __restrict__ acc_out, float* __restrict__ rowp, float* __restrict__ colp, int H, int layer, int G,
    int pad_idx, int eos_idx, int bos, int eos, CtSegs cs) {
    int g, kci, qb, Tlen;
    size_t hstride;
    ct_packed_item<HD>(cs, xcd_remap(blockIdx.x, gridDim.x), g, kci, qb, Tlen, hstride, q, k, lse, key_bias, tokens,
                       acc_out, rowp, colp);
    contact_accum_seq<T, HD>(q, k, lse, key_bias, tokens, wreg, acc_out, rowp, colp, H, Tlen, hstride, layer, G, g, kci,
                             qb, pad_idx, eos_idx, bos, eos);
}

template <typename T>
__global__ __launch_bounds__(256, 2) void contact_accum64_packed_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const float* __restrict__ lse,
    const float* __restrict__ key_bias, const int64_t* __restrict__ tokens, const float* __restrict__ wreg,
    float* __restrict__ acc_out, float* __restrict__ rowp, float* __restrict__ colp, int H, int layer, int G,
    int pad_idx, int eos_idx, int bos, int eos, CtSegs cs) {
    int g, kci, qb, Tlen;
    size_t hstride;
    ct_packed_item<64>(cs, xcd_remap(blockIdx.x, gridDim.x), g, kci, qb, Tlen, hstride, q, k, lse, key_bias, tokens,
                       acc_out, rowp, colp);
    contact_accum64_seq<T>(q, k, lse, key_bias, tokens, wreg, acc_out, rowp, colp, H, Tlen, hstride, layer, G, g, kci,
                           qb, pad_idx, eos_idx, bos, eos);
}

// blockIdx.x = work item (segment, 256-row block), blockIdx.y = head; a segment's rowsum / colsum are [C, len] at
// C * (its first row)
__global__ __launch_bounds__(256) void contact_reduce_packed_kernel(const float* __restrict__ rowp,
                                                                     const float* __restrict__ colp,
                                                                     float* __restrict__ rowsum,
                                                                     float* __restrict__ colsum, int H, int C,
                                                                     int layer, CtSegs cs) {
    const int sg = __builtin_amdgcn_readfirstlane(cs.work[2 * blockIdx.x]);
    const int t = __builtin_amdgcn_readfirstlane(cs.work[2 * blockIdx.x + 1]) * 256 + threadIdx.x;
    const int row0 = __builtin_amdgcn_readfirstlane(cs.seg[2 * sg]);
    const int Tlen = __builtin_amdgcn_readfirstlane(cs.seg[2 * sg + 1]);
    contact_reduce_seq(rowp + cs.off[4 * (size_t)sg + 1], colp + cs.off[4 * (size_t)sg + 2], rowsum + (size_t)C * row0,
                       colsum + (size_t)C * row0, H, Tlen, layer, (Tlen + 127) >> 7, (Tlen + 31) >> 5, blockIdx.y, t);
}

// blockIdx.x = work item (a segment with S > 0), blockIdx.y = c; the segment's row of wt is wt[s, :]
__global__ __launch_bounds__(256) void contact_rt_packed_kernel(float* __restrict__ rowsum,
                                                                 const float* __restrict__ colsum,
                                                                 const int64_t* __restrict__ tokens,
                                                                 const float* __restrict__ wreg,
                                                                 float* __restrict__ wt, int C, int pad_idx,
                                                                 int eos_idx, int bos, int eos, CtSegs cs) {
    const int sg = __builtin_amdgcn_readfirstlane(cs.work[blockIdx.x]);
    const int row0 = __builtin_amdgcn_readfirstlane(cs.seg[2 * sg]);
    const int Tlen = __builtin_amdgcn_readfirstlane(cs.seg[2 * sg + 1]);
    contact_rt_seq(rowsum + (size_t)C * row0, colsum + (size_t)C * row0, tokens + row0, wreg, wt + (size_t)C * sg, Tlen,
                   blockIdx.y, pad_idx, eos_idx, bos, eos);
}

// blockIdx.x = work item (segment, tile row, tile column); the segment's [S,S] map starts at out + off[3]
__global__ __launch_bounds__(256) void contact_final_packed_kernel(const float* __restrict__ acc,
                                                                    const float* __restrict__ r,
                                                                    const float* __restrict__ wt,
                                                                    const int64_t* __restrict__ tokens,
                                                                    const float* __restrict__ bias,
                                                                    float* __restrict__ out, int G, int C, int pad_idx,
                                                                    int eos_idx, int bos, int eos, CtSegs cs) {
    const int* wk = cs.work + 4 * (size_t)blockIdx.x;
    const int sg = __builtin_amdgcn_readfirstlane(wk[0]);
    const int i0 = __builtin_amdgcn_readfirstlane(wk[1]) * 32;
    const int j0 = __builtin_amdgcn_readfirstlane(wk[2]) * 32;
    const int row0 = __builtin_amdgcn_readfirstlane(cs.seg[2 * sg]);
    const int Tlen = __builtin_amdgcn_readfirstlane(cs.seg[2 * sg + 1]);
    contact_final_seq(acc + cs.off[4 * (size_t)sg], r + (size_t)C * row0, wt + (size_t)C * sg, tokens + row0, bias,
                      out + cs.off[4 * (size_t)sg + 3], G, C, Tlen, (size_t)cs.acc_stride, i0, j0, pad_idx, eos_idx, bos,
                      eos);
}

// head groups: enough workgroups to fill 256 CUs a few times over even for one short sequence.  `pairs` = the
// (128-query block, 128-key chunk) pairs of the batch: B ceil(T/128)^2 padded, sum of ceil(len/128)^2 packed — so
// a packed batch gets the G of the same sequences run padded whenever it has as many pairs (one sequence alone;
// B equal lengths), and with G the same accumulation order.
int contacts_head_groups(long long pairs, int H, int head_dim) {
    const long long per_group = pairs > 0 ? pairs : 1;
    long long G = (1024 + per_group - 1) / per_group;
    if (G > H) G = H;
    if (G < 1) G = 1;
    int hg = (int)((H + G - 1) / G);
    if (head_dim == 128 && hg > 20) hg = 20;  // direct-load kernel: 4 waves x 224 LDS floats per head of the group
    return (H + hg - 1) / hg;  // groups that actually hold a head
}

// one accumulate launch, padded or packed (`tail` = the kernel's arguments after k): the kernel of (T, HD), its
// dynamic LDS size and the one-time attribute that lets it have that much
template <typename T, int HD, bool PACKED, typename... Tail>
static hipError_t launch_accum(long long grid, int hg, hipStream_t st, const void* q, const void* k, Tail... tail) {
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    if (HD == 128 && hg > 20) return hipErrorInvalidValue;  // contacts_head_groups() keeps groups at <= 20 heads (70 KiB)
    // d64: K double buffer + parked sums of 10 heads; d128: parked sums of the group's heads
    const size_t lds = HD == 64 ? 2 * 128 * 128 + 4 * 10 * 224 * sizeof(float) : (size_t)4 * hg * 224 * sizeof(float);
    constexpr int lds_max = HD == 64 ? 2 * 128 * 128 + 4 * 10 * 224 * 4 : 4 * 20 * 224 * 4;
    auto kern = [] {
        if constexpr (HD == 64 && PACKED) return contact_accum64_packed_kernel<T>;
        else if constexpr (HD == 64) return contact_accum64_kernel<T>;
        else if constexpr (PACKED) return contact_accum_packed_kernel<T, HD>;
        else return contact_accum_kernel<T, HD>;
    }();
    static bool attr_set = false;  // per (T, HD, PACKED) = per kernel
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, st, (const T*)q, (const T*)k, tail...);
    return hipGetLastError();
}

template <bool PACKED, typename... Args>
static hipError_t launch_accum_any(int operand_dtype, int head_dim, Args... args) {
    const bool bf = operand_dtype == ESMK_DT_BF16;
    if (head_dim == 128)
        return bf ? launch_accum<__bf16, 128, PACKED>(args...) : launch_accum<_Float16, 128, PACKED>(args...);
    return bf ? launch_accum<__bf16, 64, PACKED>(args...) : launch_accum<_Float16, 64, PACKED>(args...);
}

hipError_t launch_contacts_fused_layer(const void* q, const void* k, const float* lse, const float* key_bias,
                                       const int64_t* tokens, const float* wreg, float* acc, float* rowsum,
                                       float* colsum, float* rowp, float* colp, int B, int H, int T, int C, int layer,
                                       int head_dim, int pad_idx, int eos_idx, int prepend_bos, int append_eos,
                                       int operand_dtype, hipStream_t st, int G_force) {
    const int bos = prepend_bos ? 1 : 0, eos = append_eos ? 1 : 0;
    const long long nQ = (T + 127) / 128;
    const int G = G_force > 0 ? G_force : contacts_head_groups((long long)B * nQ * nQ, H, head_dim);
    hipError_t e = launch_accum_any<false>(operand_dtype, head_dim, (long long)G * B * nQ * nQ, (H + G - 1) / G, st, q, k,
                                           lse, key_bias, tokens, wreg, acc, rowp, colp, B, H, T, layer, G, pad_idx,
                                           eos_idx, bos, eos);
    if (e != hipSuccess) return e;
    const int nP = (T + 31) / 32, nR = (T + 127) / 128;
    const unsigned grid = (unsigned)(B * H) * (unsigned)((T + 255) / 256);
    hipLaunchKernelGGL(contact_reduce_kernel, dim3(grid), dim3(256), 0, st, rowp, colp, rowsum, colsum, H, T, C, layer,
                       nR, nP);
    return hipGetLastError();
}

hipError_t launch_contacts_fused_final(const float* acc, float* rowsum, const float* colsum, float* wt,
                                       const int64_t* tokens, const float* wreg, const float* bias, float* out,
                                       int B, int H, int C, int T, int head_dim, int pad_idx, int eos_idx,
                                       int prepend_bos, int append_eos, hipStream_t st, int G_force) {
    const int bos = prepend_bos ? 1 : 0, eos = append_eos ? 1 : 0;
    const int S = T - bos - eos;
    if (S <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(contact_rt_kernel, dim3(B * C), dim3(256), 0, st, rowsum, colsum, tokens, wreg, wt, C, T,
                       pad_idx, eos_idx, bos, eos);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int nt = (S + 31) / 32;
    const long long nQ = (T + 127) / 128;
    hipLaunchKernelGGL(contact_final_kernel, dim3(nt, nt, B), dim3(256), 0, st, acc, rowsum, wt, tokens, bias, out, B,
                       G_force > 0 ? G_force : contacts_head_groups((long long)B * nQ * nQ, H, head_dim), C, T, pad_idx,
                       eos_idx, bos, eos);
    return hipGetLastError();
}

// ---- token-packed batches ------------------------------------------------------------------------------------
CtPackedPlan contacts_packed_plan(const int32_t* seg, int n_seg, int H, int head_dim, int bos, int eos) {
    CtPackedPlan p;
    p.n_seg = n_seg;
    long long pairs = 0;
    for (int s = 0; s < n_seg; ++s) {
        const long long len = seg[2 * s + 1], S = len - bos - eos;
        if (S <= 0) continue;  // empty map: no work, no scratch
        const long long nQ = (len + 127) / 128, nP = (len + 31) / 32, nt = (S + 31) / 32;
        pairs += nQ * nQ;
        p.sum_len2 += len * len;
        p.rowp += nQ * H * len;
        p.colp += nP * H * len;
        p.out += S * S;
        p.n_acc += nQ * nQ;
        p.n_red += (len + 255) / 256;
        p.n_rt += 1;
        p.n_fin += nt * nt;
    }
    p.G = contacts_head_groups(pairs, H, head_dim);
    return p;
}

void contacts_packed_tables(const CtPackedPlan& p, const int32_t* seg, int bos, int eos, int H, int32_t* dst) {
    const int n_seg = p.n_seg;
    long long* off = reinterpret_cast<long long*>(dst);
    int32_t* acc = dst + 8 * (size_t)n_seg;
    int32_t* red = acc + 4 * p.n_acc;
    int32_t* rt = red + 2 * p.n_red;
    int32_t* fin = rt + p.n_rt;
    long long o_acc = 0, o_rp = 0, o_cp = 0, o_out = 0;
    for (int s = 0; s < n_seg; ++s) {
        const long long len = seg[2 * s + 1], S = len - bos - eos;
        off[4 * s] = o_acc;
        off[4 * s + 1] = o_rp;
        off[4 * s + 2] = o_cp;
        off[4 * s + 3] = o_out;
        if (S <= 0) continue;
        o_acc += len * len;
        o_rp += (len + 127) / 128 * H * len;
        o_cp += (len + 31) / 32 * H * len;
        o_out += S * S;
        for (int t0 = 0; t0 < len; t0 += 256) {
            *red++ = s;
            *red++ = t0 / 256;
        }
        *rt++ = s;
        const int nt = (int)((S + 31) / 32);
        for (int i = 0; i < nt; ++i)
            for (int j = 0; j < nt; ++j) {
                fin[0] = s;
                fin[1] = i;
                fin[2] = j;
                fin[3] = 0;
                fin += 4;
            }
    }
    // accumulate items, longest segments first (the tail of the grid is made of short items); within a segment
    // chunk-major, query block fastest: the blocks that read one chunk's K rows are neighbours, hence on one XCD
    std::vector<int> order;
    for (int s = 0; s < n_seg; ++s)
        if (seg[2 * s + 1] - bos - eos > 0) order.push_back(s);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return seg[2 * a + 1] > seg[2 * b + 1]; });
    for (int s : order) {
        const int nQ = (seg[2 * s + 1] + 127) / 128;
        for (int kc = 0; kc < nQ; ++kc)
            for (int qb = 0; qb < nQ; ++qb) {
                acc[0] = s;
                acc[1] = kc;
                acc[2] = qb;
                acc[3] = 0;
                acc += 4;
            }
    }
}

hipError_t launch_contacts_packed_layer(const void* q, const void* k, const float* lse, const float* key_bias,
                                        const int64_t* tokens, const float* wreg, float* acc, float* rowsum,
                                        float* colsum, float* rowp, float* colp, const CtPackedPlan& p,
                                        const CtPackedDev& d, int H, int C, int layer, int head_dim, int pad_idx,
                                        int eos_idx, int prepend_bos, int append_eos, int operand_dtype,
                                        hipStream_t st) {
    if (p.n_acc <= 0) return hipSuccess;  // every segment is empty
    const int bos = prepend_bos ? 1 : 0, eos = append_eos ? 1 : 0;
    const int G = p.G;
    if (p.n_red > 0x7fffffff) return hipErrorInvalidValue;
    CtSegs cs;
    cs.seg = d.seg;
    cs.off = d.off;
    cs.work = d.acc_work;
    cs.acc_stride = p.sum_len2;
    cs.rows = d.rows;
    cs.n_items = (int)p.n_acc;
    hipError_t e = launch_accum_any<true>(operand_dtype, head_dim, (long long)G * p.n_acc, (H + G - 1) / G, st, q, k, lse,
                                          key_bias, tokens, wreg, acc, rowp, colp, H, layer, G, pad_idx, eos_idx, bos,
                                          eos, cs);
    if (e != hipSuccess) return e;
    cs.work = d.red_work;
    cs.n_items = (int)p.n_red;
    hipLaunchKernelGGL(contact_reduce_packed_kernel, dim3((unsigned)p.n_red, (unsigned)H), dim3(256), 0, st, rowp, colp,
                       rowsum, colsum, H, C, layer, cs);
    return hipGetLastError();
}

hipError_t launch_contacts_packed_final(const float* acc, float* rowsum, const float* colsum, float* wt,
                                        const int64_t* tokens, const float* wreg, const float* bias, float* out,
                                        const CtPackedPlan& p, const CtPackedDev& d, int C, int pad_idx, int eos_idx,
                                        int prepend_bos, int append_eos, hipStream_t st) {
    if (p.n_rt <= 0) return hipSuccess;  // every map is empty
    if (p.n_fin > 0x7fffffff || p.n_rt > 0x7fffffff) return hipErrorInvalidValue;
    const int bos = prepend_bos ? 1 : 0, eos = append_eos ? 1 : 0;
    CtSegs cs;
    cs.seg = d.seg;
    cs.off = d.off;
    cs.acc_stride = p.sum_len2;
    cs.rows = d.rows;
    cs.work = d.rt_work;
    cs.n_items = (int)p.n_rt;
    hipLaunchKernelGGL(contact_rt_packed_kernel, dim3((unsigned)p.n_rt, (unsigned)C), dim3(256), 0, st, rowsum, colsum,
                       tokens, wreg, wt, C, pad_idx, eos_idx, bos, eos, cs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    cs.work = d.fin_work;
    cs.n_items = (int)p.n_fin;
    hipLaunchKernelGGL(contact_final_packed_kernel, dim3((unsigned)p.n_fin), dim3(256), 0, st, acc, rowsum, wt, tokens,
                       bias, out, p.G, C, pad_idx, eos_idx, bos, eos, cs);
    return hipGetLastError();
}

}  // namespace esmk
