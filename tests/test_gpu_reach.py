"""tron_reach_codes / tron.vec.reach_codes / fill_winner / VecTron.reach and judge="fill" on the playout calls, on the GPU,
against the host model of tests/reach_support.py.  Every comparison is exact.  tests/test_reach_model_cpu.py shows, without a
GPU, that the model equals a literal BFS on the boards used here and that these boards tell every wrong model from the
right one."""
import ctypes as C

import numpy as np
import pytest

from playout_gpu_support import mods, dev, same  # noqa: F401 (mods is a fixture)
import playout_support as ps
import playout_values_support as pv
import reach_support as rch
import rollout_support as rs
import territory_support as terr

pytestmark = pytest.mark.gpu

REACH = ("counts", "dist")
COUNT_FILL, DIST_FILL = 0x5A5A5A5A, 0x7777
JUDGE_WIDTHS = (4, 5, 10)
# where the fill verdict of an unfinished playout is not the territory verdict, found on the CPU with the two models: the
# k_steps of test_playout_codes_judge (under both tapes) and the widths of test_playout_values_judge
VERDICTS_DIFFER_AT = {4: (0, 1), 5: (0, 1, 7), 10: (0, 1)}
VALUE_VERDICTS_DIFFER_AT = (4, 5)


def run_reach(mods, boards, want_dist=True):
    """reach_codes on host arrays -> (counts, dist | None) as host arrays."""
    tv, torch = mods
    counts, dist = tv.reach_codes(dev(torch, boards), want_dist=want_dist)
    torch.cuda.synchronize()
    return rs.np_(counts), (None if dist is None else rs.np_(dist))


@pytest.mark.parametrize("W", terr.WIDTHS)
def test_counts_and_planes_equal_the_model(mods, W):
    """The soup, the early and the planted boards of the width, rejected boards and the serpentines included."""
    boards, exp = rch.boards(W), rch.expected(W)
    same(run_reach(mods, boards), exp, W, REACH)
    counts, dist = run_reach(mods, boards, want_dist=False)
    assert dist is None and np.array_equal(counts, exp[0])
    tv, torch = mods
    assert np.array_equal(rs.np_(tv.fill_winner(dev(torch, exp[0]))), rch.winner(exp[0]))


@pytest.mark.parametrize("S", rch.SIDES)
def test_hand_built_boards_at_the_instantiation_boundaries(mods, S):
    """8, 16 and 32 rows per board with 32-bit masks up to side 32, 64 rows and 64-bit masks at sides 33 and 34; 8 level
    slices up to side 16, 10 above.  The split arena's last interior column is mask bit 31 / 32 at sides 33 / 34."""
    boards = rch.hand_boards(S)
    exp = rch.model(boards)
    same(run_reach(mods, boards), exp, S, REACH)
    assert np.array_equal(run_reach(mods, boards, want_dist=False)[0], exp[0])


@pytest.mark.parametrize("S", (8, 16, 32, 34))
def test_serpentine_next_to_empty_arenas(mods, S):
    """One long corridor (525 levels at side 34, 462 at side 32: past 127 and 255) among empty arenas that finish after a
    few levels.  Sides 8, 16 and 32 put 8, 4 and 2 boards in a wave, so the corridor and the arenas share one."""
    snake, plain = terr.serpentine(S), terr.arena(S, (1, 1), (S - 2, S - 2))
    boards = np.stack([snake if i in (1, 6, 19) else plain for i in range(21)])
    exp = rch.model(boards)
    assert exp[0][1][rch.FILL1] == (snake == 1).sum() and exp[0][0][rch.DEPTH1] == 2 * (S - 3) - 1
    assert S < 32 or exp[0][1][rch.DEPTH1] > 255
    same(run_reach(mods, boards), exp, S, REACH)
    assert np.array_equal(run_reach(mods, boards, want_dist=False)[0], exp[0])


@pytest.mark.parametrize("W", (4, 10, 24))
def test_a_ring_of_ones_between_ordinary_boards(mods, W):
    """Every other board of a wave has a border ring of all 1: it counts as the same board with a wall ring, and its
    neighbours' rows are what they are without it."""
    boards = ps.soup_boards(W)[:96]
    exp = rch.model(boards)
    for odd in (1, 0):
        mixed = boards.copy()
        mixed[odd::2] = terr.ring_of_ones(boards[odd::2])
        assert (mixed != boards).any()
        same(run_reach(mods, mixed), exp, (W, odd), REACH)


def raw(mods, codes_ptr, n, side, counts, dist, row=1):
    """The C entry on raw pointers; counts / dist are the guarded buffers or None, the outputs start at their row `row`."""
    tv, torch = mods
    nat = tv.nat
    cp = None if counts is None else C.c_void_p(counts.data_ptr() + row * 8 * 4)
    dp = None if dist is None else C.c_void_p(dist.data_ptr() + row * 2 * side * side * 2)
    rc = nat.lib().tron_reach_codes(codes_ptr, n, side, cp, dp, nat.stream_ptr())
    torch.cuda.synchronize()
    return rc


def guarded(torch, n, side):
    counts = torch.full((n + 2, 8), COUNT_FILL, dtype=torch.int32, device="cuda")
    dist = torch.full((n + 2, 2, side, side), DIST_FILL, dtype=torch.int16, device="cuda")
    return counts, dist


def check_guarded(counts, dist, n, exp, want_counts=True, want_dist=True):
    c, d = rs.np_(counts), rs.np_(dist)
    assert (c[0] == COUNT_FILL).all() and (c[n + 1] == COUNT_FILL).all() and (d[0] == DIST_FILL).all() and (d[n + 1] == DIST_FILL).all()
    assert np.array_equal(c[1:n + 1], exp[0][:n]) if want_counts else (c == COUNT_FILL).all()
    assert np.array_equal(d[1:n + 1], exp[1][:n]) if want_dist else (d == DIST_FILL).all()


@pytest.mark.parametrize("W", (5, 10, 32))
def test_batch_sizes_and_null_outputs(mods, W):
    """n of 1, 63, 64, 65 and 203 (a last wave partly empty at every side), sentinel rows round both outputs, each output
    NULL in turn."""
    tv, torch = mods
    S = W + 2
    boards = rch.boards(W)[1000:1203]
    exp = rch.model(boards)
    codes = dev(torch, boards)
    for n in (1, 63, 64, 65, 203):
        for want_counts, want_dist in ((True, True), (True, False), (False, True)):
            counts, dist = guarded(torch, n, S)
            rc = raw(mods, tv.nat.ptr(codes), n, S, counts if want_counts else None, dist if want_dist else None)
            assert rc == tv.nat.OK
            check_guarded(counts, dist, n, exp, want_counts, want_dist)


@pytest.mark.parametrize("W", (5, 10, 32))
def test_misaligned_boards_at_the_end_of_the_allocation(mods, W):
    """codes 1, 5 and 15 bytes and the planes 2, 6 and 14 bytes past a 16-byte boundary, the last board of either ending
    with its allocation."""
    tv, torch = mods
    S, n = W + 2, 37
    boards = rch.boards(W)[1040:1040 + n]
    exp = rch.model(boards)
    for off, doff in ((1, 2), (5, 6), (15, 14)):
        buf = torch.empty(off + n * S * S, dtype=torch.int8, device="cuda")
        dbuf = torch.full((doff + (n + 2) * 4 * S * S,), 0x77, dtype=torch.int8, device="cuda")
        assert buf.data_ptr() % 16 == 0 and dbuf.data_ptr() % 16 == 0
        codes = buf[off:].view(n, S, S)
        codes.copy_(dev(torch, boards))
        counts = torch.full((n + 2, 8), COUNT_FILL, dtype=torch.int32, device="cuda")
        dist = dbuf[doff:].view(torch.int16).view(n + 2, 2, S, S)
        rc = tv.nat.lib().tron_reach_codes(C.c_void_p(codes.data_ptr()), n, S, C.c_void_p(counts.data_ptr() + 32),
                                           C.c_void_p(dist.data_ptr() + 4 * S * S), tv.nat.stream_ptr())
        torch.cuda.synchronize()
        assert rc == tv.nat.OK
        check_guarded(counts, dist, n, exp)
        assert (rs.np_(dbuf[:doff]) == 0x77).all() and np.array_equal(rs.np_(codes), boards)
        got = tv.reach_codes(codes, want_dist=True)
        same((rs.np_(got[0]), rs.np_(got[1])), exp, (W, off), REACH)


def test_refused_arguments_write_nothing(mods):
    tv, torch = mods
    nat = tv.nat
    n, S = 8, 12
    boards = rch.boards(10)[:n]
    codes = dev(torch, boards)
    cases = [(nat.ptr(codes), -1, S, nat.ERR_BAD_ARG), (nat.ptr(codes), 2 ** 31, S, nat.ERR_BAD_ARG), (None, n, S, nat.ERR_BAD_ARG),
             (nat.ptr(codes), n, 5, nat.ERR_UNSUPPORTED), (nat.ptr(codes), n, 35, nat.ERR_UNSUPPORTED),
             (None, 0, S, nat.OK), (nat.ptr(codes), 0, S, nat.OK)]
    for cp, nn, side, want in cases:
        counts, dist = guarded(torch, n, S)
        assert raw(mods, cp, nn, side, counts, dist) == want, (nn, side)
        check_guarded(counts, dist, n, None, False, False)
    # the planes start at an even address and are not the boards; bad arguments are told before an unsupported side
    counts, dist = guarded(torch, n, S)
    keep = codes.clone()
    for side in (S, 40):
        for dp in (C.c_void_p(dist.data_ptr() + 4 * S * S + 1), nat.ptr(codes)):
            rc = nat.lib().tron_reach_codes(nat.ptr(codes), n, side, C.c_void_p(counts.data_ptr() + 32), dp, nat.stream_ptr())
            torch.cuda.synchronize()
            assert rc == nat.ERR_BAD_ARG
    assert torch.equal(codes, keep)
    check_guarded(counts, dist, n, None, False, False)
    assert raw(mods, nat.ptr(codes), n, S, None, None) == nat.OK      # both outputs NULL: nothing to do
    with pytest.raises(ValueError):
        tv.reach_codes(codes.to(torch.int32))
    with pytest.raises(nat.TronNativeError):
        tv.reach_codes(codes.cpu())


# ---- judge="fill" ----------------------------------------------------------------------------------------------------------
def judged(winner, codes):
    """(the model's winners with -1 replaced by the model's fill verdict of the model's last position, how many of those
    verdicts are not the territory verdict)."""
    verdict = rch.winner(rch.model(codes)[0])
    other = terr.winner(terr.model(codes)[0])
    assert (verdict[winner == -1] >= 0).all()
    return np.where(winner == -1, verdict, winner).astype(np.int8), int(((winner == -1) & (verdict != other)).sum())


@pytest.mark.parametrize("W", JUDGE_WIDTHS)
def test_playout_codes_judge(mods, W):
    """k_steps 0, 1 and 7 on the soup, drawn moves and the mixed tape: steps and codes as without the judge, the winner the
    model playout's with every -1 replaced by the fill verdict, which is not the territory verdict at VERDICTS_DIFFER_AT."""
    tv, torch = mods
    boards = ps.soup_boards(W)
    codes = dev(torch, boards)
    for name in ("none", "mixed"):
        tape = ps.soup_tapes(W)[name]
        tape = None if tape is None else tape[:7]
        model = ps.playout(boards, tape, ks=(0, 1, 7), **ps.SOUP_KEY)
        for k in (0, 1, 7):
            (steps, winner, final), _ = model[k]
            exp, differ = judged(winner, final)
            assert differ >= 1 or k not in VERDICTS_DIFFER_AT[W], (W, name, k)
            for want_codes in (False, True):
                got = tv.playout_codes(codes, None if tape is None else dev(torch, tape), k, want_codes=want_codes, judge="fill",
                                       **ps.SOUP_KEY)
                assert np.array_equal(rs.np_(got[0]), steps) and np.array_equal(rs.np_(got[1]), exp), (W, name, k)
                assert got[1].dtype == torch.int8
                assert (got[2] is None) if not want_codes else np.array_equal(rs.np_(got[2]), final)


@pytest.mark.parametrize("W", JUDGE_WIDTHS)
def test_playout_values_judge(mods, W):
    """k_steps = 1: the counts are the model's fill verdicts of the 16 successor positions x copies.  k_steps = W * W: the
    counts are the unjudged ones wherever nothing is unfinished, the steps everywhere."""
    tv, torch = mods
    boards, copies = pv.boards(W), 3
    n = len(boards)
    fanned, tape = ps.fan_out(boards, 1, copies)
    (steps, winner, final), _ = ps.playout(fanned, tape, k_steps=1, **pv.KEY)[1]
    exp, differ = judged(winner, final)
    counts, total = ps.tally(steps, exp, n, copies)
    assert (differ >= 1 or W not in VALUE_VERDICTS_DIFFER_AT) and counts[..., 3].sum() == 0
    for want_actions in (True, False):
        got = tv.playout_values(dev(torch, boards), 1, copies, want_actions=want_actions, judge="fill", **pv.KEY)
        assert np.array_equal(rs.np_(got[0]), counts) and np.array_equal(rs.np_(got[1]), total)
        assert (got[2] is None) if not want_actions else np.array_equal(rs.np_(got[2]), ps.pick(counts))
    codes, K = dev(torch, boards), W * W
    plain = [rs.np_(t) for t in tv.playout_values(codes, K, copies, **pv.KEY)]
    got = [rs.np_(t) for t in tv.playout_values(codes, K, copies, judge="fill", **pv.KEY)]
    done = plain[0][..., 3] == 0
    assert done.mean() > 0.5 and np.array_equal(got[0][done], plain[0][done]) and np.array_equal(got[1], plain[1])
    assert (got[0][..., 3] == 0).all() and np.array_equal(got[0].sum(-1), plain[0].sum(-1))


def test_env_methods_and_the_other_judges(mods):
    """VecTron.reach and the env's judge="fill" calls against the functions on the env's codes; judge=None and
    judge="territory" are what they are without this judge: the plain call, and the territory verdict composed by hand."""
    tv, torch = mods
    W, N = 10, 96
    codes = dev(torch, ps.soup_boards(W)[:N])
    plain = tv.playout_codes(codes, None, 7, want_codes=True, **ps.SOUP_KEY)
    for a, b in zip(plain, tv.playout_codes(codes, None, 7, want_codes=True, judge=None, **ps.SOUP_KEY)):
        assert torch.equal(a, b)
    terr_judged = tv.playout_codes(codes, None, 7, want_codes=True, judge="territory", **ps.SOUP_KEY)
    verdict = tv.territory_winner(tv.territory_codes(plain[2])[0])
    assert torch.equal(terr_judged[0], plain[0]) and torch.equal(terr_judged[2], plain[2]) and (plain[1] == -1).any()
    assert torch.equal(terr_judged[1], torch.where(plain[1] == -1, verdict, plain[1]))
    for bad in ("voronoi", True, 1, ["fill"]):
        with pytest.raises(ValueError):
            tv.playout_codes(codes, None, 7, judge=bad)
        with pytest.raises(ValueError):
            tv.playout_values(codes, 7, judge=bad)

    env = tv.VecTron(N, W, seed=0xABE, rank=1)
    env.reset()
    env.rollout_actions(rs.make_tape(N, 5, salt=2), rs.new_totals())
    before = env.grid().clone()
    p1 = env._p1_codes().clone()
    counts, dist = env.reach(want_dist=True)
    exp = rch.model(rs.np_(p1))
    assert np.array_equal(rs.np_(counts), exp[0]) and np.array_equal(rs.np_(dist), exp[1]) and env.reach()[1] is None
    key = dict(seed=env.seed, stream_id=env.rank, call=6)
    for a, b in zip(env.playout(k_steps=3, copies=2, call=6, judge="fill"),
                    tv.playout_codes(p1.repeat_interleave(2, dim=0), None, 3, judge="fill", **key)):
        assert (a is None and b is None) or torch.equal(a, b)
    vals = tv.playout_values(p1, 3, 2, judge="fill", **key)
    for a, b in zip(env.playout_values(3, 2, call=6, judge="fill"), vals):
        assert torch.equal(a, b)
    for player in (1, 2):
        assert torch.equal(env.montecarlo_actions(player, k_steps=3, copies=2, call=6, judge="fill"), vals[2][:, player - 1])
    assert torch.equal(env.grid(), before)
    env.close()
