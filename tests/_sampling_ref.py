"""numpy references of the sampling kernels (esm_amd/csrc/sampling.hip): Philox4x32-10 in integer arithmetic, the
Fisher-Yates shuffle of a chain's position list, and the token draw in fp64 with the rule that says which draws a comparison
may count ("decided": the threshold is far enough from every boundary of the cumulative sum that fp32 and fp64 must agree).
No torch, no engine: the CPU tests check this file against known answers, the GPU tests check the kernels against it."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
PERMUTATION, TOKEN = 0, 1  # counter word 2
DECIDED_MARGIN = 1e-5  # a draw is decided when |u * total - boundary| > DECIDED_MARGIN * total at every boundary
UNDECIDED_CAP = 0.005  # at most this fraction of the draws of a test may be undecided


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (ints or equally shaped arrays) -> the 4 output words as uint64 arrays holding 32-bit
    values.  Ten rounds; the key is bumped between them."""
    c = [np.asarray(w, dtype=np.uint64) & np.uint64(MASK32) for w in counter]
    k = [np.asarray(w, dtype=np.uint64) & np.uint64(MASK32) for w in key]
    m32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & m32, (p0 >> s32) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(W0)) & m32, (k[1] + np.uint64(W1)) & m32]
    return c


def word0(seed, chain, epoch_or_step, purpose, index):
    """First output word at counter (chain, epoch_or_step, purpose, index) under key (seed & 0xffffffff, seed >> 32)."""
    seed = int(seed)
    chain = np.asarray(chain, dtype=np.int64) & MASK32  # int32 chain ids enter as their 32-bit pattern
    index = np.asarray(index, dtype=np.int64) & MASK32
    step = np.asarray(epoch_or_step, dtype=np.int64) & MASK32
    return philox4x32_10((chain, step, purpose, index), (seed & MASK32, seed >> 32))[0]


def uniform(seed, chain, step, index):
    """fp32 u = (word0 >> 8) * 2^-24 of the token draw at (chain, step, index): exact, in [0, 1)."""
    w = word0(seed, chain, step, TOKEN, index)
    return ((w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def shuffle(positions, seed, chain, epoch):
    """The kernel's Fisher-Yates shuffle of one chain's list: for i = len - 1 .. 1, j = (word0(chain, epoch, 0, i) * (i + 1)) >> 32,
    swap elements i and j."""
    p = [int(x) for x in positions]
    if len(p) > 1:
        idx = np.arange(len(p))
        w = word0(seed, chain, epoch, PERMUTATION, idx)
        for i in range(len(p) - 1, 0, -1):
            j = (int(w[i]) * (i + 1)) >> 32
            p[i], p[j] = p[j], p[i]
    return p


def candidates(V, allowed_mask, exclude=-1):
    return [v for v in range(V) if (allowed_mask >> v) & 1 and v != exclude]


def draw(row, u, allowed_mask, inv_temperature, exclude=-1):
    """The draw of one row in fp64 from its fp32 log-probabilities: (token, logq, decided).  inv_temperature is rounded to fp32
    first, as the kernel receives it.  Greedy (0): the largest log-probability, ties to the lowest index; always decided."""
    row = np.asarray(row, dtype=np.float32)
    cand = candidates(row.shape[0], allowed_mask, exclude)
    if not cand:
        return -1, 0.0, True
    x = row[cand].astype(np.float64)
    inv_t = float(np.float32(inv_temperature))
    if inv_t == 0.0:
        return cand[int(np.argmax(x))], 0.0, True  # np.argmax: the first of equal maxima
    z = x * inv_t
    m = z.max()
    w = np.exp(z - m)
    cum = np.cumsum(w)
    total = cum[-1]
    thr = float(u) * total
    over = np.nonzero(cum > thr)[0]
    k = int(over[0]) if over.size else len(cand) - 1
    decided = bool(np.all(np.abs(cum - thr) > DECIDED_MARGIN * total))
    return cand[k], float(z[k] - m - np.log(total)), decided


def draw_fp32(row, u, allowed_mask, inv_temperature, exclude=-1):
    """An fp32 emulation of the kernel's arithmetic (numpy's expf in place of the device's): the token only."""
    row = np.asarray(row, dtype=np.float32)
    cand = candidates(row.shape[0], allowed_mask, exclude)
    if not cand:
        return -1
    z = row[cand] * np.float32(inv_temperature)
    w = np.exp(z - z.max()).astype(np.float32)
    cum = np.float32(0.0)
    sums = []
    for wi in w:
        cum = np.float32(cum + wi)
        sums.append(cum)
    thr = np.float32(np.float32(u) * cum)
    for k, c in enumerate(sums):
        if c > thr:
            return cand[k]
    return cand[-1]


def logq_bound(total_log):
    """4 fp32 ulp at max(1, |log total|)."""
    return 4.0 * float(np.spacing(np.float32(max(1.0, abs(total_log)))))
