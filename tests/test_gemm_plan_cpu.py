"""Which GEMM kernel the library launches for an nn.Linear call (gemm_plan, esm_amd/csrc/gemm_dispatch.hip), seen without
a GPU through esmk_debug_gemm_plan: the rule restated here independently and compared over every shape the models
produce, the properties the engine relies on, the ESMK_GEMM_IMPL semantics, and what the shipped library refuses."""
import ctypes

import pytest

from esm_amd import _native as N

EPI_GELU_T, EPI_RESID, EPI_QK, EPI_V, EPI_MSA_CTX, EPI_QKV_ALL = 2, 4, 5, 6, 7, 8
GENERIC, OLD, FOLD, SPLIT, BATCHED = 1, 2, 4, 8, 16

MS = sorted({B * T for B in (1, 2, 4, 8, 16, 32, 64) for T in (64, 513, 1022, 1024)} | {65664})
ES = (320, 480, 640, 768, 1280, 2560, 5120)


def nks(E):
    return ((2 * E, E), (E, E), (3 * E, E), (4 * E, E), (E, 4 * E), (33, E))


def admitted(flags):
    """the epilogues a form exists for (kernels.h; esmk_op_linear_split)"""
    return {FOLD: (EPI_GELU_T, EPI_RESID, EPI_QK, EPI_V, EPI_QKV_ALL), SPLIT: (0, 1, 2, 4)}.get(flags, tuple(range(9)))


def plan(M, n, K, epi, flags=0):
    out = (ctypes.c_int32 * 4)()
    assert N.lib.esmk_debug_gemm_plan(M, n, K, epi, flags, out) == 0, N.lib.esmk_last_error()
    assert out[3] == 0
    return out[0], out[1], out[2]


def set_impl(impl):
    assert N.lib.esmk_debug_gemm_impl(impl, 0) == 0


@pytest.fixture(autouse=True)
def _library_choice():
    set_impl(0)
    yield
    set_impl(0)


# ---- the rule, restated -----------------------------------------------------------------------------------------------
def rounds(M, n, rows):
    return (-(-M // rows) * -(-n // 256) + 255) // 256  # tiles over 256 workgroups, rounded up


def half9(M, n):
    return 0.58 * rounds(M, n, 128) < 0.92 * rounds(M, n, 256)


def half8(M, n):
    return 0.8 * rounds(M, n, 128) < 0.97 * rounds(M, n, 256)


def cost9(M, n, half):
    return 0.58 * rounds(M, n, 128) if half else float(rounds(M, n, 256))


def expected(M, n, K, epi, flags=0, impl=0):
    fold, split, batched = bool(flags & FOLD), bool(flags & SPLIT), bool(flags & BATCHED)
    Kg = 2 * K if split else K  # the split-weight GEMM runs over the hi | lo image of the weight
    aligned = Kg % 64 == 0 and n % 8 == 0
    heads = n % 64 == 0 or epi not in (EPI_QK, EPI_V, EPI_MSA_CTX)
    ok9 = (aligned and heads and not batched and not (fold and split) and epi != EPI_MSA_CTX
           and (epi != EPI_QKV_ALL or (n % 3 == 0 and (n // 3) % 128 == 0 and not split)) and 512 * Kg <= 0x7fffffff)
    hooks = bool(flags & (GENERIC | OLD))
    if fold or epi == EPI_QKV_ALL:  # forms that exist in gemm9 only
        return (9, int(epi == EPI_QKV_ALL or half9(M, n)), 0) if ok9 and not (epi == EPI_QKV_ALL and hooks) else (0, 0, 0)
    if ok9 and not hooks and impl != 8:
        return (9, int(impl != 9 and half9(M, n)), 0)
    generalised = split or batched or epi == EPI_MSA_CTX
    if aligned and heads and not hooks and not (generalised and epi == 3):  # gemm8 has no generalised fp32-GELU form
        return (8, int(not generalised and half8(M, n)), 0)
    if generalised or epi > EPI_V:
        return (0, 0, 0)
    if aligned and not flags & GENERIC:
        return (256, 0, 0) if heads else (0, 0, 0)
    return (64, 0, 0) if Kg % 32 == 0 and epi <= EPI_RESID else (0, 0, 0)


def grid(flag_set):
    for flags in flag_set:
        for E in ES:
            for n, K in nks(E):
                for epi in admitted(flags):
                    for M in MS:
                        yield M, n, K, epi, flags


@pytest.mark.parametrize("impl", [0, 8, 9])
def test_plan_follows_the_rule_on_every_model_shape(impl):
    set_impl(impl)
    count, bad = 0, []
    for M, n, K, epi, flags in grid((0, FOLD, SPLIT, BATCHED, GENERIC, OLD)):
        got, want = plan(M, n, K, epi, flags), expected(M, n, K, epi, flags, impl)
        count += 1
        if got != want:
            bad.append((M, n, K, epi, flags, got, want))
    assert count > 30000 and not bad, (len(bad), bad[:10])


def test_properties_the_engine_relies_on():
    kernels = set()
    for M, n, K, epi, flags in grid((0, FOLD, SPLIT, BATCHED)):
        kernel, half, variant = plan(M, n, K, epi, flags)
        kernels.add(kernel)
        assert variant == 0
        if flags == 0 and epi <= EPI_RESID and (K % 64 != 0 or n == 33):  # E = 480 as K; the vocabulary projection
            assert kernel == 64, (M, n, K, epi)
        if epi == EPI_QKV_ALL and kernel != 0:  # the combined kernel exists with half-height tiles only
            assert (kernel, half) == (9, 1), (M, n, K, flags)
        if flags == FOLD:  # a fold-form call never takes another kernel than gemm9
            ok9 = K % 64 == 0 and n % 8 == 0 and (epi in (EPI_GELU_T, EPI_RESID) or n % 64 == 0) and \
                (epi != EPI_QKV_ALL or (n % 3 == 0 and (n // 3) % 128 == 0))
            assert kernel == (9 if ok9 else 0), (M, n, K, epi)
        if flags in (SPLIT, BATCHED) and kernel == 8:
            assert half == 0  # the generalised forms of gemm8 run full-height tiles
    assert kernels == {0, 8, 9, 64}  # the 256 x 256 tile kernel only through force_old
    assert plan(4096, 1280, 1280, 0, OLD) == (256, 0, 0) and plan(4096, 1280, 1280, 0, GENERIC) == (64, 0, 0)
    assert plan(4096, 1280, 480, 0, OLD) == (64, 0, 0) and plan(4096, 2560, 480, EPI_QK) == (0, 0, 0)
    assert plan(0, 1280, 1280, 0) == (0, 0, 0)
    out = (ctypes.c_int32 * 4)()
    for args in ((64, 64, 64, 9, 0), (64, 64, 64, -1, 0), (64, 64, 64, 0, 32), (64, 64, 64, 0, FOLD), (64, 64, 64, 1, FOLD)):
        assert N.lib.esmk_debug_gemm_plan(*args, out) != 0 and b"esmk_debug_gemm_plan" in N.lib.esmk_last_error(), args
    assert N.lib.esmk_debug_gemm_plan(64, 64, 64, 0, 0, None) != 0


def test_gemm_impl_switch_and_what_the_shipped_library_refuses():
    M, E = 4 * 1022, 1280  # half-height tiles pay here: 32 x 5 tiles in one round against 16 x 5
    assert plan(M, E, E, EPI_RESID) == (9, 1, 0) and plan(64 * 1024, E, E, EPI_RESID) == (9, 0, 0)
    set_impl(8)
    assert plan(M, E, E, EPI_RESID) == (8, 1, 0) and plan(64 * 1024, E, E, EPI_RESID) == (8, 0, 0)
    assert plan(M, E, E, EPI_RESID, FOLD) == (9, 1, 0)  # the forms only gemm9 has stay there
    assert plan(M, 3 * E, E, EPI_QKV_ALL) == (9, 1, 0)
    set_impl(9)
    assert plan(M, E, E, EPI_RESID) == (9, 0, 0)  # gemm9 as the caller asks for it: full height unless half_m is forced
    assert plan(M, E, E, 0, BATCHED) == (8, 0, 0) and plan(M, 33, E, 1) == (64, 0, 0)
    set_impl(0)
    assert plan(M, E, E, EPI_RESID) == (9, 1, 0)
    assert N.lib.esmk_debug_gemm_impl(7, 0) != 0
    # experiments closed as zero-sum: compiled only into ESMK_EXPERIMENTS builds (common.h)
    for impl, variant in ((9, 1), (9, 2), (9, 2048), (0, 3), (9, -1)):
        assert N.lib.esmk_debug_gemm_impl(impl, variant) != 0 and b"variant must be 0" in N.lib.esmk_last_error()
    assert plan(M, E, E, EPI_RESID) == (9, 1, 0)  # a refused call changes nothing
    for key in (b"resid_desync", b"resid_desync_group", b"attn_stagger", b"lnf_dbg"):
        assert N.lib.esmk_debug_set(key, ctypes.c_double(1)) != 0 and b"unknown key" in N.lib.esmk_last_error(), key
    assert N.lib.esmk_debug_set(b"qkv_one_launch", ctypes.c_double(-1)) == 0


@pytest.mark.parametrize("flags", [0, FOLD])
def test_one_launch_qkv_is_cheaper_by_the_plans_own_costs(flags):
    """gemm_qkv_one_launch takes the combined launch where 0.58 x its rounds of half-height tiles undercut the two
    separate launches by more than a quarter round.  What the two launches cost follows from the tile height gemm_plan
    gives each of them: wherever the rule (restated) chooses one launch, the costs of the three PLANS agree with it.
    (The choice itself needs a model handle: tests/test_qkv_one_launch_gpu.py.)"""
    chosen = 0
    for E in (640, 768, 1280, 2560, 5120):  # E % 128 == 0: the shapes the combined kernel takes
        for M in MS:
            one = 0.58 * rounds(M, 3 * E, 128) < cost9(M, 2 * E, half9(M, 2 * E)) + cost9(M, E, half9(M, E)) - 0.25
            plans = [plan(M, n, E, epi, flags) for n, epi in ((3 * E, EPI_QKV_ALL), (2 * E, EPI_QK), (E, EPI_V))]
            assert all(p[0] == 9 for p in plans) and plans[0][1] == 1, (M, E, plans)
            costs = [cost9(M, n, p[1]) for n, p in zip((3 * E, 2 * E, E), plans)]
            if one:
                chosen += 1
                assert costs[0] < costs[1] + costs[2] - 0.25, (M, E, plans, costs)
    assert chosen > 0
