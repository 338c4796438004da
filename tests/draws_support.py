"""Host models of the DDQN loop's random draws and of its loss's tie rule, restated from their definitions in numpy:
the epsilon-greedy mix (csrc/tron_dqn.hip::k_eps_greedy), the replay sampler's permutation
(csrc/tron_replay.hip::k_sample_indices) and the Double-DQN loss with its gradient (k_td_loss).  All three are integer
or exactly rounded float32 arithmetic, so the kernels are held to these models bit for bit (tests/test_gpu_draws.py);
tests/test_draws_model_cpu.py holds the models to the oracle's Philox and to what a sampler must be.  No GPU, no torch."""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_SH32 = np.uint64(32)


def _u64(x):
    return np.asarray(x, dtype=np.uint64) & _M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 (Salmon et al., SC'11) -> uint32[..., 4], broadcast over its arguments.  Ten rounds of
    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key bumped by the Weyl
    constants after each; 32 x 32 -> 64-bit products in uint64, every word masked back to 32 bits."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(v) for v in (c0, c1, c2, c3, k0, k1)))
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> _SH32) ^ c1 ^ k0, p1 & _M32, (p0 >> _SH32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def eps_greedy_words(n, seed, stream, call):
    """The Philox word of each of n observations: word j % 4 of the block at counter (q low, q high, call low, call high),
    q = j // 4, key (seed, stream)."""
    call = int(call)
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    x = philox4x32_10(q & _M32, q >> _SH32, call & 0xFFFFFFFF, call >> 32, seed, stream)
    return x.reshape(-1)[:n]


def eps_greedy_model(greedy, eps, seed, stream, call):
    """int8[n] actions: the high 16 bits h of the observation's word decide (u = (h + 0.5) / 65536, exact in float32),
    its low 2 bits are the random action; u <= eps explores, in float32 (a NaN eps never does)."""
    greedy = np.asarray(greedy, dtype=np.int8)
    x = eps_greedy_words(greedy.shape[0], seed, stream, call)
    u = ((x >> np.uint32(16)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -16)
    explore = u <= np.float32(eps)
    return np.where(explore, (x & np.uint32(3)).astype(np.int8), greedy)


def half_bits(size):
    """The smallest h >= 1 with 4**h >= size, at most 16: the sampler permutes 2h-bit numbers."""
    h = 1
    while h < 16 and 4 ** h < size:
        h += 1
    return h


def feistel_keys(seed, stream, call):
    """uint32[..., 8]: the round keys of one sample() call, Philox blocks b = 0, 1 at counter (call, b, 0, "SMPL") under
    key (seed, stream).  Broadcasts over `call`."""
    call = _u64(call)
    return np.concatenate([philox4x32_10(call, b, 0, 0x5A4D504C, seed, stream) for b in (0, 1)], axis=-1)


def _feistel_f(x, k):
    x = ((x ^ k) * np.uint64(0x9E3779B1)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x85EBCA77)) & _M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE3D)) & _M32
    return x ^ (x >> np.uint64(16))


def feistel_permute(x, keys, size):
    """pi(x) for every x (all < size) under round keys uint32[..., 8] broadcast against x: eight rounds of
    (l, r) <- (r, l ^ (f(r, key[t]) & mask)) on the two half_bits(size)-bit halves, repeated while the image is >= size."""
    hb = np.uint64(half_bits(size))
    mask = np.uint64((1 << int(hb)) - 1)
    keys = np.asarray(keys, dtype=np.uint64)
    shape = np.broadcast(np.asarray(x), keys[..., 0]).shape
    x = np.broadcast_to(np.asarray(x, dtype=np.uint64), shape).reshape(-1).copy()
    keys = np.broadcast_to(keys, shape + (8,)).reshape(-1, 8)
    todo = np.arange(x.shape[0])
    while todo.size:
        v, k = x[todo], keys[todo]
        l, r = (v >> hb) & mask, v & mask
        for t in range(8):
            l, r = r, l ^ (_feistel_f(r, k[:, t]) & mask)
        v = (l << hb) | r
        x[todo] = v
        todo = todo[v >= np.uint64(size)]
    return x.astype(np.int64).reshape(shape)


def sample_indices_model(size, batch, seed, stream, call):
    """int64[batch]: draw j of sample() call number `call` (a uint32) on a ring with `size` filled slots is pi(j)."""
    assert 1 <= batch <= size
    return feistel_permute(np.arange(batch, dtype=np.uint64), feistel_keys(seed, stream, int(call) & 0xFFFFFFFF), size)


def expand_codes(codes, channels, plane4):
    """util.pop_up on rows of observation codes int8[n, cells] -> float32[n, channels, cells]: wall (-1), mine (-2 -> 1,
    10 -> 10), the enemy's (-3 -> 1, -10 -> 10), and with four channels a constant plane; any other byte is empty."""
    v = np.asarray(codes, dtype=np.int8).astype(np.int32)
    out = np.zeros((v.shape[0], channels, v.shape[1]), np.float32)
    out[:, 0] = v == -1
    out[:, 1] = np.where(v == -2, 1.0, np.where(v == 10, 10.0, 0.0))
    out[:, 2] = np.where(v == -3, 1.0, np.where(v == -10, 10.0, 0.0))
    if channels == 4:
        out[:, 3] = np.float32(plane4)
    return out


def td_model(q, a, r, d, ql, qt, gamma):
    """(loss float64, grad_q float32[B, 4], e float32[B]) of the Double-DQN loss.  am = first maximum of ql's row
    (-0.0 == 0.0: the earlier one), y = r + (gamma * qt[am]) * (1 - d), e = q[a] - y, every operation rounded to float32
    once.  With d in {0, 1} the product by (1 - d) is exact, so fusing it into the add changes nothing.  grad_q[b][a_b]
    = 2 e / B evaluated as the mean-squared-error gradient is, (2 e) * float32(1 / B): scaling by two is exact, so
    (2 * float32(1 / B)) * e has the same bits; a true division by B differs in the last bit whenever B is not a power
    of two.  loss = sum(float64(e) ** 2) / B from those exact e."""
    f32 = np.float32
    q, ql, qt = (np.asarray(v, f32).reshape(-1, 4) for v in (q, ql, qt))
    B = q.shape[0]
    a = np.asarray(a, np.int64).reshape(B)
    r, d = np.asarray(r, f32).reshape(B), np.asarray(d, f32).reshape(B)
    rows = np.arange(B)
    am = np.argmax(ql, axis=1)
    with np.errstate(invalid="ignore"):
        y = r + (f32(gamma) * qt[rows, am]) * (f32(1.0) - d)
        e = q[rows, a] - y
        g = (f32(2.0) * e) * (f32(1.0) / f32(B))
    grad = np.zeros((B, 4), f32)
    grad[rows, a] = g
    return float(np.sum(e.astype(np.float64) ** 2) / B), grad, e


# ---- the cases tests/test_gpu_draws.py runs (kept here so that the CPU tests can check their coverage) ----------------
EPS_BIG_N = 4 * 256 * 4096 + 5                     # the first size at which k_eps_greedy's grid-stride loop takes a second trip
EPS_NS = (1, 2, 3, 4, 5, 255, 1024, 1025, 65537, EPS_BIG_N)
_T17 = np.float32(2.0 ** -17)
EPSILONS = {"0": np.float32(0.0), "2^-17": _T17, "below 2^-17": np.nextafter(_T17, np.float32(0.0)), "0.3": np.float32(0.3),
            "1-2^-17": np.float32(1.0) - _T17, "1": np.float32(1.0), "nan": np.float32(np.nan)}
EPS_CALLS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1)
EPS_KEYS = ((0, 0), (11, 3), (0xFFFFFFFF, 0xFFFFFFFF))


def eps_cases():
    """The cross product of the four axes thinned to a few dozen (n, epsilon name, call, (seed, stream)): three per small
    n, stepping through the other axes at different strides, and the large n where it is needed: at both sides of the
    u <= eps boundary, at a mid epsilon on both grid-stride trips, and for NaN."""
    names = list(EPSILONS)
    cases = []
    for i, n in enumerate(EPS_NS[:-1]):
        for k in range(3):
            cases.append((n, names[(2 * i + 3 * k) % 7], EPS_CALLS[(i + 2 * k) % 5], EPS_KEYS[(i + k) % 3]))
    cases += [(65537, "0.3", 2 ** 32 + 1, (11, 3)), (65537, "1-2^-17", 2 ** 32, (0xFFFFFFFF, 0xFFFFFFFF)),
              (EPS_BIG_N, "2^-17", 2 ** 32 + 1, (11, 3)), (EPS_BIG_N, "below 2^-17", 2 ** 32 + 1, (11, 3)),
              (EPS_BIG_N, "0.3", 2 ** 32 - 1, (0xFFFFFFFF, 0xFFFFFFFF)), (EPS_BIG_N, "nan", 0, (0, 0))]
    return cases


SAMPLER_CASES = ((1, 1), (2, 2), (3, 2), (4, 4), (5, 5), (16, 16), (17, 17), (64, 64), (65, 64), (256, 256), (257, 256),
                 (1000, 999), (4096, 4096), (4097, 4096), (65537, 300), (1048577, 300))


# ---- chi-square quantiles ---------------------------------------------------------------------------------------------
# (0.01 %, 99.99 %) quantiles of the chi-square distribution; the small degrees of freedom from tables (the
# Wilson-Hilferty cube is off by tens of percent in the lower tail there), any other from Wilson-Hilferty:
# k (1 - 2 / (9 k) + z sqrt(2 / (9 k))) ** 3 with z = +-3.7190165 (the normal 99.99 % point), good to 1e-5 relative at k >= 1000.
CHI2_TABLE = {1: (1.5708e-8, 15.1367), 3: (5.2148e-3, 21.1075), 5: (8.2177e-2, 25.7448), 19: (3.9683, 50.7955)}


def chi2_window(dof):
    if dof in CHI2_TABLE:
        return CHI2_TABLE[dof]
    assert dof >= 1000, dof
    z, c = 3.7190165, 2.0 / (9.0 * dof)
    return dof * (1.0 - c - z * c ** 0.5) ** 3, dof * (1.0 - c + z * c ** 0.5) ** 3
