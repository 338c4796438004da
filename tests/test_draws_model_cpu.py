"""The host models of tests/draws_support.py on their own: the numpy Philox against the oracle's (the one pinned to the
reference fixtures) and the published known answers, the sampler model as a permutation at the sizes a learner starts in,
its uniformity over ordered outcomes at sizes no GPU test can afford, the independence of the two bit fields the
epsilon-greedy mix takes from one word, and the coverage of the cases the GPU tests run.  No GPU."""
import itertools
import math

import numpy as np
import pytest

import draws_support as ds


def test_philox_equals_the_oracle():
    import oracle
    rs = np.random.RandomState(20)
    words = rs.randint(0, 2 ** 32, (300, 6), dtype=np.uint64)
    edge = np.array([0, 1, 0xFFFFFFFF, 0x80000000, 0xFFFFFFFE], np.uint64)
    words[:60, 1:4] = edge[rs.randint(0, 5, (60, 3))]                   # high counter words set, small and saturated ones
    words[60:90, :4] = edge[rs.randint(0, 5, (30, 4))]
    words[90:110, 4:] = edge[rs.randint(0, 5, (20, 2))]
    got = ds.philox4x32_10(*words.T)
    assert got.shape == (300, 4) and got.dtype == np.uint32
    for w, g in zip(words, got):
        assert np.array_equal(g, oracle.philox(w[:4], w[4:])), [hex(int(v)) for v in w]
    one = ds.philox4x32_10(*words[7])                                   # scalars in, one block out
    assert one.shape == (4,) and np.array_equal(one, got[7])


# Random123's known-answer vectors for philox4x32-10 (kat_vectors): counter, key -> block
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert [int(v) for v in ds.philox4x32_10(*ctr, *key)] == list(want)


def test_half_bits():
    assert [ds.half_bits(s) for s in (1, 2, 4, 5, 16, 17, 64, 65, 4096, 4097, 1 << 30, (1 << 30) + 1, 1 << 32)] == \
        [1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 15, 16, 16]
    for s in range(1, 300):
        h = ds.half_bits(s)
        assert 4 ** h >= s and (h == 1 or 4 ** (h - 1) < s)


PERM_SIZES = sorted(set(range(1, 71)) | {4 ** h + k for h in range(1, 7) for k in (-1, 0, 1)})


@pytest.mark.parametrize("key", [(5, 0), (0xFFFFFFFF, 7)])
def test_sampler_model_is_a_permutation(key):
    for size in PERM_SIZES:
        for call in (0, 1, 0xFFFFFFFF):
            full = ds.sample_indices_model(size, size, *key, call)
            assert full.dtype == np.int64 and np.array_equal(np.sort(full), np.arange(size)), (size, call)
            for batch in {1, (size + 1) // 2, size - 1} - {0}:
                assert np.array_equal(ds.sample_indices_model(size, batch, *key, call), full[:batch]), (size, batch, call)


def test_sampler_model_depends_on_every_part_of_its_key():
    base = ds.sample_indices_model(1000, 1000, 5, 1, 2)
    for other in ((6, 1, 2), (5, 2, 2), (5, 1, 3)):
        assert not np.array_equal(ds.sample_indices_model(1000, 1000, *other), base)
    keys = ds.feistel_keys(5, 1, 2)
    assert keys.shape == (8,) and len(set(keys.tolist())) == 8
    assert np.array_equal(keys, ds.feistel_keys(5, 1, np.arange(4))[2])


UNIFORMITY_CALLS = 60000


@pytest.mark.parametrize("size,batch,seed,stream", [(2, 1, 5, 0), (3, 2, 5, 0), (5, 2, 5, 0), (17, 3, 5, 0)])
def test_sampler_model_is_uniform_over_ordered_outcomes(size, batch, seed, stream):
    """Pearson's chi-square of the size! / (size - batch)! ordered outcomes over 60 000 consecutive calls under one key,
    inside the (0.01 %, 99.99 %) quantiles for cells - 1 degrees of freedom.  One deterministic number per case:
    (2, 1): 1.46 in (1.6e-8, 15.1); (3, 2): 8.00 in (0.082, 25.7); (5, 2): 46.6 in (3.97, 50.8);
    (17, 3): 4048 in (3752, 4424).
    (5, 2) sits high because the sampler is not quite uniform there: on the 4-bit domain of sizes 5 ... 16 (two-bit
    halves, a two-bit round function) the ordered PAIRS of the first two draws keep a bias of about 2 % per cell — 600 000
    calls give 256 at 19 degrees of freedom for size 5, 200 at 41 for size 7, 305 at 239 for size 16; single draws are
    uniform (0.7 at 4), and so are pairs at sizes up to 4 and from 17 on.  At 60 000 calls six of eight keys tried pass
    this window at size 5 and two do not (56 and 90); a learner holds 5 ... 16 transitions only for its first pushes.)"""
    keys = ds.feistel_keys(seed, stream, np.arange(UNIFORMITY_CALLS))[:, None, :]
    draws = ds.feistel_permute(np.arange(batch, dtype=np.uint64)[None, :], keys, size)
    assert draws.shape == (UNIFORMITY_CALLS, batch) and draws.min() >= 0 and draws.max() < size
    code = np.zeros(UNIFORMITY_CALLS, np.int64)
    for j in range(batch):
        code = code * size + draws[:, j]
    cells = [sum(v * size ** (batch - 1 - j) for j, v in enumerate(t)) for t in itertools.permutations(range(size), batch)]
    assert len(cells) == math.factorial(size) // math.factorial(size - batch)
    counts = np.bincount(code, minlength=size ** batch)
    assert counts[cells].sum() == UNIFORMITY_CALLS                     # no draw repeats a slot
    expect = UNIFORMITY_CALLS / len(cells)
    chi2 = float(((counts[cells] - expect) ** 2 / expect).sum())
    lo, hi = ds.chi2_window(len(cells) - 1)
    print(f"sampler size {size} batch {batch}: chi2 {chi2:.4f}, {len(cells) - 1} dof, window ({lo:.4g}, {hi:.4g})")
    assert lo < chi2 < hi, (chi2, lo, hi)


def test_explore_bits_and_action_bits_are_independent():
    """epsilon 0.5 over 2^20 observations: the 2 x 4 table of (explored, the word's low two bits) has a chi-square of
    independence inside the (0.01 %, 99.99 %) quantiles for 3 degrees of freedom (0.67 in (0.0052, 21.1)); an action taken
    from the bits that decide the comparison makes it ~1e6."""
    n = 1 << 20
    x = ds.eps_greedy_words(n, 11, 3, 1)
    marker = np.full(n, 4, np.int8)
    out = ds.eps_greedy_model(marker, 0.5, 11, 3, 1)
    explored = out != 4
    assert np.array_equal(out[explored], (x[explored] & 3).astype(np.int8))
    assert abs(explored.mean() - 0.5) < 4 * 0.5 / n ** 0.5
    table = np.zeros((2, 4))
    np.add.at(table, (explored.astype(np.int64), (x & 3).astype(np.int64)), 1)
    expect = table.sum(1, keepdims=True) * table.sum(0, keepdims=True) / n
    chi2 = float(((table - expect) ** 2 / expect).sum())
    lo, hi = ds.chi2_window(3)
    print(f"explore x action: chi2 {chi2:.4f}, 3 dof, window ({lo:.4g}, {hi:.4g})")
    assert lo < chi2 < hi, (chi2, lo, hi)
    top = (x >> 30).astype(np.int64)                                    # what the check catches: an action from bits that decide u <= 0.5
    t3 = np.zeros((2, 4))
    np.add.at(t3, (explored.astype(np.int64), top), 1)
    e3 = t3.sum(1, keepdims=True) * t3.sum(0, keepdims=True) / n
    assert float(((t3 - e3) ** 2 / e3).sum()) > 1e5


def test_eps_model_at_the_boundary_of_the_comparison():
    """u <= eps: at eps = 2^-17 exactly the observations with h == 0 explore (u = 2^-17), one ulp below none; at
    1 - 2^-17 all do (h == 65535 gives u = 1 - 2^-17); NaN never explores.  u is exact in float32 for every h."""
    h = np.arange(65536, dtype=np.uint32)
    u = (h.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -16)
    assert np.array_equal(u.astype(np.float64), (h.astype(np.float64) + 0.5) / 65536.0)
    n = ds.EPS_BIG_N
    x = ds.eps_greedy_words(n, 11, 3, 2 ** 32 + 1)
    zero_h = (x >> 16) == 0
    assert 20 <= int(zero_h.sum()) <= 130                              # expected 64
    marker = np.full(n, 4, np.int8)
    assert np.array_equal(ds.eps_greedy_model(marker, ds.EPSILONS["2^-17"], 11, 3, 2 ** 32 + 1) != 4, zero_h)
    assert not np.any(ds.eps_greedy_model(marker, ds.EPSILONS["below 2^-17"], 11, 3, 2 ** 32 + 1) != 4)
    assert not np.any(ds.eps_greedy_model(marker[:70000], ds.EPSILONS["nan"], 11, 3, 0) != 4)
    assert np.all(ds.eps_greedy_model(marker[:70000], ds.EPSILONS["1-2^-17"], 11, 3, 0) != 4)
    assert not np.any(ds.eps_greedy_model(marker[:70000], ds.EPSILONS["0"], 11, 3, 0) != 4)


def test_gpu_cases_cover_every_axis():
    cases = ds.eps_cases()
    assert len(cases) <= 48
    assert {c[0] for c in cases} == set(ds.EPS_NS) and {c[1] for c in cases} == set(ds.EPSILONS)
    assert {c[2] for c in cases} == set(ds.EPS_CALLS) and {c[3] for c in cases} == set(ds.EPS_KEYS)
    assert {(ds.EPS_BIG_N, "2^-17"), (ds.EPS_BIG_N, "below 2^-17")} <= {c[:2] for c in cases}
    assert ds.EPS_BIG_N == 4 * 256 * 4096 + 5


def test_td_model_ties_and_signed_zeros():
    f = np.float32
    ql = np.array([[1, 1, 1, 1], [2, 0, 1, 2], [0, 2, 1, 2], [0, 1, 2, 2], [0.0, -0.0, -1, -2], [-0.0, 0.0, -1, -2],
                   [-np.inf] * 4, [0, 3, 1, 2]], f)
    qt = np.tile(np.array([10, 20, 30, 40], f), (8, 1))
    q = np.zeros((8, 4), f)
    a = np.arange(8) % 4
    r, d = np.ones(8, f), np.zeros(8, f)
    loss, grad, e = ds.td_model(q, a, r, d, ql, qt, 1.0)
    assert np.array_equal(e, -(1 + np.array([10, 10, 20, 30, 10, 10, 10, 20], f)))
    assert np.array_equal(grad[np.arange(8), a], f(2) * e * (f(1) / f(8))) and np.count_nonzero(grad) == 8
    assert loss == float(np.sum(e.astype(np.float64) ** 2) / 8)
    _, _, e1 = ds.td_model(q, a, r, np.ones(8, f), ql, qt, 1.0)
    assert np.array_equal(e1, -np.ones(8, f))                           # done: the target is the reward
