// gemm_dispatch.hip — which kernel serves an nn.Linear call.  Host code only: no kernel lives here.
//
// Every linear layer of every model goes through launch_gemm = gemm_plan (a pure decision: no HIP call, no launch) + one
// switch over the planned kernel.  The kernels:
//     9    gemm9.hip   persistent, one wave per SIMD: every dense call it supports, and the only home of the
//                      LayerNorm-fold forms, the f16x3 output form and the one-launch q / k / v form (EPI_QKV_ALL)
//     8    gemm8.hip   persistent, two waves per SIMD: the generalised-addressing calls (MSA Transformer, batched,
//                      strided, remapped, packed batches) and every dense call under ESMK_GEMM_IMPL=8
//     256  gemm.hip    one 256 x 256 tile per workgroup: force_old (the reference of the bit-for-bit tests)
//     64   gemm.hip    generic 64 x 64 tiles: K % 64 != 0, N % 8 != 0, force_generic
// gemm8, gemm9 and gemm256 give the same bits.  esmk_debug_gemm_plan (engine.hip) shows the plan of a call without a GPU.
//
// Process-wide switches, all in one record that is filled from the environment once:
//     ESMK_GEMM_IMPL = 8 | 9 | auto     / esmk_debug_gemm_impl(impl, 0)         the persistent kernel of dense calls
//     ESMK_QKV_ONE_LAUNCH = 0 | 1 | -1  / esmk_debug_set("qkv_one_launch", v)   q, k and v as one launch: never / always / by rounds
// The closed experiments (gemm9 issue-pattern variants, start-up delays of the residual GEMMs) are in git history and profiles/.
#include "common.h"
#include "kernels.h"
#include <atomic>
#include <mutex>
#include <stdlib.h>
#include <string.h>

namespace esmk {

// Atomics: launches and esmk_debug_* calls may come from several host threads.  A debug call overrides the environment.
struct GemmSettings {
    std::atomic<int> impl{0};      // 8 = gemm8 always, 9 = gemm9 wherever it applies (tile height as the caller says), 0 = by rule
    std::atomic<int> qkv_one{-1};  // 1 / 0 = always / never, -1 = where it saves rounds of tiles
    int qkv_one_env = -1;
};

static GemmSettings& settings() {
    static GemmSettings s;
    static std::once_flag once;
    std::call_once(once, [] {
        if (const char* e = getenv("ESMK_GEMM_IMPL")) s.impl = e[0] == '9' ? 9 : e[0] == '8' ? 8 : 0;
        if (const char* e = getenv("ESMK_QKV_ONE_LAUNCH")) s.qkv_one = s.qkv_one_env = atoi(e);
    });
    return s;
}

bool gemm_set_impl(int impl, int var) {
    if (var != 0) return false;  // gemm9 has one form
    settings().impl = impl;
    return true;
}

bool gemm_set_knob(const char* key, double value) {
    GemmSettings& s = settings();
    if (strcmp(key, "qkv_one_launch") == 0) s.qkv_one = (int)value < -1 ? s.qkv_one_env : (int)value;
    else return false;
    return true;
}

// Cost of a dense gemm9 launch: rounds of tiles over the 256 workgroups, a half-height tile counted as 0.58 of a full
// one (1470 against 2400 - 2600 cycles per K tile, profiles/r3_gemm9_half_height_b4.log).  Half-height tiles are taken
// where they cost less than 0.92 of the full-height launch.  THE tile-height rule: gemm_plan picks with it and
// gemm_qkv_one_launch predicts with it what the two separate launches would cost.
static double gemm9_cost(int M, int N, bool half) {
    const long long tiles = (long long)((M + (half ? 127 : 255)) / (half ? 128 : 256)) * ((N + 255) / 256);
    return (half ? 0.58 : 1.0) * (double)((tiles + 255) / 256);
}
static bool gemm9_half_pays(int M, int N) { return gemm9_cost(M, N, true) < 0.92 * gemm9_cost(M, N, false); }
static double gemm9_best_cost(int M, int N) { return gemm9_cost(M, N, gemm9_half_pays(M, N)); }

GemmPlan gemm_plan(const GemmArgs& p, int epi) {
    const GemmPlan none;
    if (p.M <= 0 || p.N <= 0 || p.K <= 0) return none;
    const GemmSettings& s = settings();
    const int impl = s.impl.load();
    const bool ok9 = gemm9_supports(p, epi);
    GemmPlan pl;
    if (p.x3_out) {  // the hi | hi | lo output form of the f16x3 mode exists in gemm9 only (full-height tiles)
        pl.kernel = ok9 ? 9 : 0;
        return pl;
    }
    // the LayerNorm-fold forms of the epilogues and the one-launch q / k / v form (the caller asks gemm_qkv_one_launch
    // first) exist in gemm9 only: such a call never takes another kernel
    const bool lnf = gemm9_ln_fold(p, epi);
    const bool only9 = lnf || epi == EPI_QKV_ALL;
    const bool hooks = p.force_old || p.force_generic;
    if (only9 && (!ok9 || (epi == EPI_QKV_ALL && hooks))) return none;
    if (only9 || (ok9 && !hooks && impl != 8)) {
        pl.kernel = 9;
        if (!only9 && impl == 9) {
            pl.half_m = p.half_m > 0;
        } else {
            // EPI_QKV_ALL exists with HALF-height tiles only (see gemm_qkv_one_launch)
            pl.half_m = p.half_m > 0 || (p.half_m == 0 && gemm9_half_pays(p.M, p.N)) || epi == EPI_QKV_ALL;
        }
        return pl;
    }
    if (!p.force_old && !p.force_generic && gemm8_supports(p, epi)) {
        pl.kernel = 8;  // the generalised forms run full-height tiles (dispatch8)
        pl.half_m = !gemm8_generalised(p, epi) && gemm8_half_height(p);
        return pl;
    }
    if (gemm8_generalised(p, epi)) return none;  // the tile kernels only know dense calls
    pl.kernel = gemm_tile_kernel(p, epi);
    return pl;
}

// q / k (N = 2E) and v (N = E) as ONE launch (EPI_QKV_ALL)?  Only when it saves rounds: the two launches each round their
// tile count up to whole rounds of 256 workgroups, the combined launch rounds once (B = 1 x 1022 at E = 1280: 80 + 40
// half-height tiles = two part-filled rounds against one of 120; B = 64: 10 + 5 against 15 rounds — no gain, the two
// launches stay).  The results are bit-identical either way.
bool gemm_qkv_one_launch(const GemmArgs& qk) {
    const GemmSettings& s = settings();
    const int mode = s.qkv_one.load();
    GemmArgs all = qk;
    all.N = 3 * qk.E;
    if (mode == 0 || qk.N != 2 * qk.E || s.impl.load() == 8 || gemm_plan(all, EPI_QKV_ALL).kernel != 9) return false;
    if (mode == 1) return true;
    // The combined kernel exists with HALF-height tiles only.  A full-height instantiation holding both K loops was built
    // twice: round 4 (accumulator quads shuffled through VGPRs: 1.7 x the time per tile) and round 5 with the quads pinned
    // to the AGPR file — clean K loops in the ISA report, but on the GPU 26.1 against 20.4 ms per step for q / k / v at
    // B = 64 and 7.12 against 6.25 ms at B = 16 (profiles/r5_qkv_one_launch_full_height.log): removed again.
    return gemm9_cost(qk.M, 3 * qk.E, true) < gemm9_best_cost(qk.M, 2 * qk.E) + gemm9_best_cost(qk.M, qk.E) - 0.25;
}

hipError_t launch_gemm(const GemmArgs& p, int epi, int operand_dtype, hipStream_t st) {
    const GemmPlan pl = gemm_plan(p, epi);
    switch (pl.kernel) {
        case 9: {
            GemmArgs q = p;
            q.half_m = pl.half_m;
            return launch_gemm9(q, epi, operand_dtype, st);
        }
        case 8: return launch_gemm8(p, epi, operand_dtype, st);  // asks gemm8_half_height itself, as the plan did
        case 256: return launch_gemm256(p, epi, operand_dtype, st);
        case 64: return launch_gemm64(p, epi, operand_dtype, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace esmk
