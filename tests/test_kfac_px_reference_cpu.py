"""kfac_px_support, what the GPU tests of csrc/tron_kfac_px.hip stand on, checked without a GPU: ref_factor against the
definition written out as loops, the integer inputs, and the Python copy of the kernel's launch plan against the batches
worked out by hand for a 256-CU device."""
import pytest

torch = pytest.importorskip("torch")

from kfac_px_support import (EXACT_LIMIT, FLUSH_STEPS, PX_KERNELS, exact_bound, flush_batch, flushes, int_input,
                             least_flush_batches, px_plan, ref_factor, steps_per_stack)


def loop_factor(x, scale):
    """A[c 9 + t][c' 9 + t'] = scale * sum over images and output positions p of x[c][p + t] x[c'][p + t'], x zero outside the
    image: a loop over (t, t') and the channel pairs on an explicitly zero-padded copy."""
    B, C, S, _ = x.shape
    xp = torch.zeros(B, C, S + 2, S + 2, dtype=torch.float64)
    xp[:, :, 1:S + 1, 1:S + 1] = x.double()
    A = torch.zeros(9 * C, 9 * C, dtype=torch.float64)
    for t in range(9):
        for u in range(9):
            for c in range(C):
                a = xp[:, c, t // 3:t // 3 + S, t % 3:t % 3 + S]
                for cp in range(C):
                    A[c * 9 + t, cp * 9 + u] = (a * xp[:, cp, u // 3:u // 3 + S, u % 3:u % 3 + S]).sum()
    return A * scale


@pytest.mark.parametrize("nonneg", [False, True])
def test_ref_factor_is_the_definition(nonneg):
    """B = 3, C = 8, S = 5, integers: equal, not close (every sum is a small integer), also in chunks of one and two images
    and with a power-of-two scale."""
    x = int_input(3, 8, 5, nonneg, seed=5)
    want = loop_factor(x, 1.0)
    assert want.abs().max() > 0 and not torch.equal(want, torch.diag(torch.diag(want)))
    for chunk in (512, 2, 1):
        assert torch.equal(ref_factor(x, 1.0, chunk=chunk), want)
    assert torch.equal(ref_factor(x, 2.0 ** -10), want * 2.0 ** -10)
    assert torch.equal(want, want.t())


def test_ref_factor_of_an_impulse_names_the_taps():
    """A single 1 at pixel (y, x) of channel c is seen by output position (y - dy, x - dx) through tap t = 3 (dy + 1) + (dx + 1),
    where that position exists: ones at A[c 9 + t][c 9 + t] for those taps and nothing else.  At the corner (0, 0) the
    positions (y - dy, x - dx) with dy, dx in {-1, 0} exist: taps 0, 1, 3, 4."""
    x = torch.zeros(2, 8, 5, 5)
    x[1, 7, 0, 0] = 1.0
    want = torch.zeros(72, 72, dtype=torch.float64)
    for t in (0, 1, 3, 4):
        want[7 * 9 + t, 7 * 9 + t] = 1.0
    assert torch.equal(ref_factor(x, 1.0), want)


def test_int_input_values():
    for nonneg, values in ((False, [-2, -1, 0, 1, 2]), (True, [0, 1, 2])):
        x = int_input(40, 32, 12, nonneg, seed=3)
        assert x.dtype == torch.float32 and sorted(x.unique().tolist()) == values
        zeros = (x == 0).float().mean().item()
        assert abs(zeros - 1 / 3) < 0.01
        assert torch.equal(x, int_input(40, 32, 12, nonneg, seed=3)) and not torch.equal(x, int_input(40, 32, 12, nonneg, seed=4))
    assert exact_bound(8717, 12) < EXACT_LIMIT <= exact_bound(30000, 12)


# band 0's least flushing batch on 256 CUs, by hand: per_kind = 51;
#   side 12 (two images a stack, 3 bands of 3 slabs): n = 51 * 3 // 9 = 17; C = 64: 3 steps a stack, 86 stacks, 2 * 86 * 17 + 1;
#     C = 32 (KG = 4): 1 step a stack, 256 stacks, 2 * 256 * 17 + 1;
#   side 26 (bands of 5, 5, 5, 5, 2 slabs): n = 51 * 5 // 22 = 11; C = 64: 5 steps, 52 stacks, 52 * 11 + 1; C = 32: 2 steps, 128 * 11 + 1;
#   side 34 (bands of 7, 7, 7, 7, 7, 5 slabs): n = 51 * 7 // 40 = 8; C = 64: 7 steps, 37 stacks, 37 * 8 + 1; C = 32: 2 steps, 128 * 8 + 1.
BAND0_256 = {(64, 12): 2925, (32, 12): 8705, (64, 26): 573, (32, 26): 1409, (64, 34): 297, (32, 34): 1025}
# the short last band of sides 26 and 34 has fewer workgroups and fewer slabs: 26: n = 51 * 2 // 22 = 4, 2 slabs: C = 64: 128 stacks,
# 128 * 4 + 1; C = 32: 256 * 4 + 1; 34: n = 51 * 5 // 40 = 6, 5 slabs: C = 64: 52 * 6 + 1 (here later than band 0); C = 32: 128 * 6 + 1
LAST_256 = {(64, 12): 2925, (32, 12): 8705, (64, 26): 513, (32, 26): 1025, (64, 34): 313, (32, 34): 769}


@pytest.mark.parametrize("C,S", sorted(PX_KERNELS))
def test_flush_batches_on_256_cus(C, S):
    """least_flush_batches' closed form against the hand derivation, and against the kernel's stack loop walked by flushes():
    one image fewer and the band does not flush."""
    least = least_flush_batches(256, C, S)
    assert least[:-1] == [BAND0_256[(C, S)]] * (len(least) - 1) and least[-1] == LAST_256[(C, S)]
    for b, B in enumerate(least):
        assert flushes(256, C, S, B)[b] == 1 and flushes(256, C, S, B - 1)[b] == 0
    assert sum(flushes(256, C, S, min(least) - 1)) == 0
    B = flush_batch(256, C, S)
    p = px_plan(256, C, S, B)
    assert max(least) + 5 <= B <= max(least) + 40 and B <= 12000
    assert all(f >= 1 for f in flushes(256, C, S, B))
    assert all(p["nstack"] % n for n in p["n"]) and (p["NI"] == 1 or B % 2 == 1)
    assert exact_bound(B, S) < EXACT_LIMIT


def test_plan_on_256_cus():
    """Workgroups per band, and whether the grid has idle workgroups whose parts are zeroed (wgs != used)."""
    p = px_plan(256, 32, 12, 4096)
    assert (p["n"], p["used"], p["wgs"]) == ([17, 17, 17], 51, 56)
    p = px_plan(256, 64, 26, 4096)
    assert (p["n"], p["used"], p["wgs"]) == ([11, 11, 11, 11, 4], 48, 48)
    p = px_plan(256, 64, 34, 4096)
    assert (p["n"], p["used"], p["wgs"]) == ([8, 8, 8, 8, 8, 6], 46, 48)
    assert px_plan(256, 64, 12, 3)["n"] == [2, 2, 2] and px_plan(256, 64, 26, 1)["n"] == [1] * 5
    assert [steps_per_stack(3, 4, k) for k in range(4)] == [1, 1, 1, 0] and steps_per_stack(7, 1, 0) == 7
    assert FLUSH_STEPS == 256
