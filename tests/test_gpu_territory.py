"""tron_territory_codes / tron.vec.territory_codes / territory_winner / VecTron.territory, tron_values_pick and judge="territory"
on the playout calls, on the GPU, against the host model of tests/territory_support.py.  Every comparison is exact.
tests/test_territory_model_cpu.py shows, without a GPU, that the model equals a literal BFS on the boards used here and that
these boards tell every wrong model from the right one."""
import ctypes as C

import numpy as np
import pytest

from playout_gpu_support import TERRITORY, mods, dev, run_territory, same  # noqa: F401 (mods is a fixture)
import playout_support as ps
import playout_values_support as pv
import rollout_support as rs
import territory_support as terr

pytestmark = pytest.mark.gpu

COUNT_FILL, OWNER_FILL = 0x5A5A5A5A, 0x77


@pytest.mark.parametrize("W", terr.WIDTHS)
def test_counts_and_owner_equal_the_model(mods, W):
    """The soup, the early boards and the planted boards of the width, rejected boards included."""
    boards, exp = terr.boards(W), terr.expected(W)
    same(run_territory(mods, boards), exp, W, TERRITORY)
    counts, owner = run_territory(mods, boards, want_owner=False)
    assert owner is None and np.array_equal(counts, exp[0])
    tv, torch = mods
    assert np.array_equal(rs.np_(tv.territory_winner(dev(torch, exp[0]))), terr.winner(exp[0]))


def hand_boards(S):
    """Boards of one side: arenas with the heads in corners and side by side, an arena split by a wall row with and
    without a door (above the wall only player 1 reaches the last interior column, below it only player 2), the
    serpentine, the same with a ring of ones, and rejected boards."""
    out = [terr.arena(S, (1, 1), (S - 2, S - 2)), terr.arena(S, (S - 2, S - 2), (1, 1)), terr.arena(S, (1, S - 2), (S - 2, 1)),
           terr.arena(S, (S // 2, S // 2 - 1), (S // 2, S // 2)), terr.arena(S, (1, S - 2), (2, S - 2))]
    split = terr.arena(S, (1, S - 2), (S - 2, S - 2))
    split[S // 2, 1:-1] = -2
    door = split.copy()
    door[S // 2, S - 2] = 1
    out += [split, door, terr.serpentine(S), terr.serpentine(S).T.copy()]
    out += [terr.ring_of_ones(b) for b in list(out)]
    no_head, on_border = out[0].copy(), out[0].copy()
    no_head[1, 1] = 1
    on_border[1, 1], on_border[0, 1] = 1, 10
    return np.stack(out + [no_head, on_border])


@pytest.mark.parametrize("S", (6, 8, 9, 16, 17, 32, 33, 34))
def test_hand_built_boards_at_the_instantiation_boundaries(mods, S):
    """8, 16 and 32 rows per board with 32-bit masks up to side 32, 64 rows and 64-bit masks at sides 33 and 34: either side
    of every boundary.  At sides 33 and 34 the split arena's cells in the last interior column (bit 31 / bit 32) belong to
    one player each, and the ring of ones sets the mask bits 32 / 33 in the data."""
    boards = hand_boards(S)
    exp = terr.model(boards)
    for i, b in enumerate(boards):
        lc, lo = terr.literal(b)
        assert list(exp[0][i]) == lc and np.array_equal(exp[1][i], lo), (S, i)
    split = exp[1][5]
    assert (split[2:S // 2, S - 2] == 1).all() and (split[S // 2 + 1:S - 2, S - 2] == 2).all()
    assert exp[0][5][4] + exp[0][5][5] == exp[0][5][:3].sum()        # separated
    same(run_territory(mods, boards), exp, S, TERRITORY)


@pytest.mark.parametrize("S", (8, 16, 32, 34))
def test_serpentine_next_to_empty_arenas(mods, S):
    """One long corridor (555 levels at side 34) among empty arenas that finish after a few levels.  Sides 8, 16 and 32 put
    8, 4 and 2 boards in a wave, so the corridor and the arenas share one; at side 34 a board has a wave to itself and
    they share the block."""
    snake, plain = terr.serpentine(S), terr.arena(S, (1, 1), (S - 2, S - 2))
    boards = np.stack([snake if i in (1, 6, 19) else plain for i in range(21)])
    exp = terr.model(boards)
    assert exp[0][1][0] == exp[0][1][4] == (snake == 1).sum() and exp[0][1][5] == 0
    same(run_territory(mods, boards), exp, S, TERRITORY)


@pytest.mark.parametrize("W", (4, 10, 24))
def test_a_ring_of_ones_between_ordinary_boards(mods, W):
    """Every other board of a wave (8, 4, 2 boards per wave at sides 6, 12, 26) has a border ring of all 1: it counts as the
    same board with a wall ring, and its neighbours' rows are what they are without it."""
    boards = ps.soup_boards(W)[:96]
    assert (terr.ring_of_ones(boards) != boards).any() and (boards[:, 0, :] != 1).all()
    exp = terr.model(boards)
    mixed = boards.copy()
    mixed[1::2] = terr.ring_of_ones(boards[1::2])
    same(run_territory(mods, mixed), exp, W, TERRITORY)
    mixed = boards.copy()
    mixed[0::2] = terr.ring_of_ones(boards[0::2])
    same(run_territory(mods, mixed), exp, W, TERRITORY)


def raw(mods, codes_ptr, n, side, counts, owner, row=1):
    """The C entry on raw pointers; counts / owner are the guarded buffers or None, the outputs start at their row `row`."""
    tv, torch = mods
    nat = tv.nat
    cp = None if counts is None else C.c_void_p(counts.data_ptr() + row * 6 * 4)
    op = None if owner is None else C.c_void_p(owner.data_ptr() + row * side * side)
    rc = nat.lib().tron_territory_codes(codes_ptr, n, side, cp, op, nat.stream_ptr())
    torch.cuda.synchronize()
    return rc


def guarded(torch, n, side):
    counts = torch.full((n + 2, 6), COUNT_FILL, dtype=torch.int32, device="cuda")
    owner = torch.full((n + 2, side, side), OWNER_FILL, dtype=torch.int8, device="cuda")
    return counts, owner


def check_guarded(counts, owner, n, exp, want_counts=True, want_owner=True):
    c, o = rs.np_(counts), rs.np_(owner)
    assert (c[0] == COUNT_FILL).all() and (c[n + 1] == COUNT_FILL).all() and (o[0] == OWNER_FILL).all() and (o[n + 1] == OWNER_FILL).all()
    assert np.array_equal(c[1:n + 1], exp[0][:n]) if want_counts else (c == COUNT_FILL).all()
    assert np.array_equal(o[1:n + 1], exp[1][:n]) if want_owner else (o == OWNER_FILL).all()


@pytest.mark.parametrize("W", (5, 10, 32))
def test_batch_sizes_and_null_outputs(mods, W):
    """n of 1, 63, 64, 65 and 203 (a last wave partly empty at every side: 8, 4 and 1 boards per wave here), sentinel rows
    round both outputs, each output NULL in turn."""
    tv, torch = mods
    S = W + 2
    boards = terr.boards(W)[1000:1203]
    exp = terr.model(boards)
    codes = dev(torch, boards)
    for n in (1, 63, 64, 65, 203):
        for want_counts, want_owner in ((True, True), (True, False), (False, True)):
            counts, owner = guarded(torch, n, S)
            rc = raw(mods, tv.nat.ptr(codes), n, S, counts if want_counts else None, owner if want_owner else None)
            assert rc == tv.nat.OK
            check_guarded(counts, owner, n, exp, want_counts, want_owner)


@pytest.mark.parametrize("W", (5, 10, 32))
def test_misaligned_boards_at_the_end_of_the_allocation(mods, W):
    """codes (and the owner plane) as slices that start 1, 5 and 15 bytes past a 16-byte boundary, the last board ending
    with the allocation."""
    tv, torch = mods
    S, n = W + 2, 37
    boards = terr.boards(W)[1040:1040 + n]
    exp = terr.model(boards)
    for off in (1, 5, 15):
        buf = torch.empty(off + n * S * S, dtype=torch.int8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        codes = buf[off:].view(n, S, S)
        codes.copy_(dev(torch, boards))
        obuf = torch.full((off + (n + 2) * S * S,), OWNER_FILL, dtype=torch.int8, device="cuda")
        counts = torch.full((n + 2, 6), COUNT_FILL, dtype=torch.int32, device="cuda")
        owner = obuf[off:].view(n + 2, S, S)
        rc = tv.nat.lib().tron_territory_codes(C.c_void_p(codes.data_ptr()), n, S, C.c_void_p(counts.data_ptr() + 24),
                                               C.c_void_p(owner.data_ptr() + S * S), tv.nat.stream_ptr())
        torch.cuda.synchronize()
        assert rc == tv.nat.OK
        check_guarded(counts, owner, n, exp)
        assert (rs.np_(obuf[:off]) == OWNER_FILL).all() and np.array_equal(rs.np_(codes), boards)
        got = tv.territory_codes(codes, want_owner=True)
        same((rs.np_(got[0]), rs.np_(got[1])), exp, (W, off), TERRITORY)


def test_refused_arguments_write_nothing(mods):
    tv, torch = mods
    nat = tv.nat
    n, S = 8, 12
    boards = terr.boards(10)[:n]
    codes = dev(torch, boards)
    cases = [(nat.ptr(codes), -1, S, nat.ERR_BAD_ARG), (nat.ptr(codes), 2 ** 31, S, nat.ERR_BAD_ARG), (None, n, S, nat.ERR_BAD_ARG),
             (nat.ptr(codes), n, 5, nat.ERR_UNSUPPORTED), (nat.ptr(codes), n, 35, nat.ERR_UNSUPPORTED),
             (None, 0, S, nat.OK), (nat.ptr(codes), 0, S, nat.OK)]
    for cp, nn, side, want in cases:
        counts, owner = guarded(torch, n, S)
        assert raw(mods, cp, nn, side, counts, owner) == want, (nn, side)
        check_guarded(counts, owner, n, None, False, False)
    # the owner plane may not be the boards; bad arguments are told before an unsupported side
    counts, _ = guarded(torch, n, S)
    keep = codes.clone()
    for side in (S, 40):
        rc = nat.lib().tron_territory_codes(nat.ptr(codes), n, side, C.c_void_p(counts.data_ptr() + 24), nat.ptr(codes), nat.stream_ptr())
        torch.cuda.synchronize()
        assert rc == nat.ERR_BAD_ARG
    assert torch.equal(codes, keep) and (rs.np_(counts) == COUNT_FILL).all()
    assert raw(mods, nat.ptr(codes), n, S, None, None) == nat.OK      # both outputs NULL: nothing to do
    with pytest.raises(ValueError):
        tv.territory_codes(codes.to(torch.int32))
    with pytest.raises(nat.TronNativeError):
        tv.territory_codes(codes.cpu())


# ---- judge="territory" -----------------------------------------------------------------------------------------------------
def judged(winner, codes):
    """The model's winners with -1 replaced by the model's verdict of the model's last position."""
    verdict = terr.winner(terr.model(codes)[0])
    assert (verdict[winner == -1] >= 0).all()
    return np.where(winner == -1, verdict, winner).astype(np.int8)


@pytest.mark.parametrize("W", terr.WIDTHS)
def test_playout_codes_judge(mods, W):
    """k_steps 0, 1 and 7 on the soup, drawn moves and the mixed tape: steps and codes as without the judge, the winner the
    model playout's with every -1 replaced."""
    tv, torch = mods
    boards = ps.soup_boards(W)
    codes = dev(torch, boards)
    for name in ("none", "mixed"):
        tape = ps.soup_tapes(W)[name]
        tape = None if tape is None else tape[:7]
        model = ps.playout(boards, tape, ks=(0, 1, 7), **ps.SOUP_KEY)
        for k in (0, 1, 7):
            (steps, winner, final), _ = model[k]
            exp = judged(winner, final)
            assert k > 1 or ((winner == -1) & (exp > 0)).any()
            for want_codes in (False, True):
                got = tv.playout_codes(codes, None if tape is None else dev(torch, tape), k, want_codes=want_codes, judge="territory",
                                       **ps.SOUP_KEY)
                assert np.array_equal(rs.np_(got[0]), steps) and np.array_equal(rs.np_(got[1]), exp), (W, name, k)
                assert got[1].dtype == torch.int8
                assert (got[2] is None) if not want_codes else np.array_equal(rs.np_(got[2]), final)


@pytest.mark.parametrize("W", pv.WIDTHS)
def test_playout_values_judge_full_length(mods, W):
    """k_steps = W * W: wherever tron_playout_values reports no unfinished playout, the judged composition's counts are
    its counts; the steps are its steps everywhere; the picks agree on the boards with nothing unfinished."""
    tv, torch = mods
    codes, copies, K = dev(torch, pv.boards(W)), 3, W * W
    plain = [rs.np_(t) for t in tv.playout_values(codes, K, copies, **pv.KEY)]
    got = [rs.np_(t) for t in tv.playout_values(codes, K, copies, judge="territory", **pv.KEY)]
    for g, p in zip(got, plain):
        assert g.dtype == p.dtype and g.shape == p.shape
    done = plain[0][..., 3] == 0
    assert done.mean() > 0.5
    assert np.array_equal(got[0][done], plain[0][done]) and np.array_equal(got[1], plain[1])
    assert (got[0][..., 3] == 0).all() and np.array_equal(got[0].sum(-1), plain[0].sum(-1))
    whole = done.all((1, 2))
    assert whole.any() and np.array_equal(got[2][whole], plain[2][whole])
    assert np.array_equal(got[2], ps.pick(got[0]))


@pytest.mark.parametrize("W", pv.WIDTHS)
def test_playout_values_judge_one_step(mods, W):
    """k_steps = 1: the counts are the model's verdicts of the 16 successor positions x copies (the model playout's
    endings where the first step ends the game)."""
    tv, torch = mods
    boards, copies = pv.boards(W), 3
    n = len(boards)
    fanned, tape = ps.fan_out(boards, 1, copies)
    (steps, winner, final), _ = ps.playout(fanned, tape, k_steps=1, **pv.KEY)[1]
    counts, total = ps.tally(steps, judged(winner, final), n, copies)
    assert (winner == -1).any() and counts[..., 3].sum() == 0
    for want_actions in (True, False):
        got = tv.playout_values(dev(torch, boards), 1, copies, want_actions=want_actions, judge="territory", **pv.KEY)
        assert np.array_equal(rs.np_(got[0]), counts) and np.array_equal(rs.np_(got[1]), total)
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.int32
        assert (got[2] is None) if not want_actions else np.array_equal(rs.np_(got[2]), ps.pick(counts))


def test_values_pick_equals_playout_values_actions(mods):
    tv, torch = mods
    nat = tv.nat
    for W in (5, 10):
        codes = dev(torch, ps.soup_boards(W))
        n = len(codes)
        counts, _, actions = tv.playout_values(codes, 7, 3, **pv.KEY)
        out = torch.full((n + 2, 2), 0x55, dtype=torch.int8, device="cuda")
        assert nat.lib().tron_values_pick(nat.ptr(counts), n, C.c_void_p(out.data_ptr() + 2), nat.stream_ptr()) == nat.OK
        torch.cuda.synchronize()
        assert torch.equal(out[1:n + 1], actions) and (rs.np_(out[[0, n + 1]]) == 0x55).all()
        assert (rs.np_(actions) == -1).any() and np.array_equal(rs.np_(actions), ps.pick(rs.np_(counts)))
    fill = out.clone()
    assert nat.lib().tron_values_pick(None, n, nat.ptr(out), nat.stream_ptr()) == nat.ERR_BAD_ARG
    assert nat.lib().tron_values_pick(nat.ptr(counts), n, None, nat.stream_ptr()) == nat.ERR_BAD_ARG
    assert nat.lib().tron_values_pick(nat.ptr(counts), -1, nat.ptr(out), nat.stream_ptr()) == nat.ERR_BAD_ARG
    assert nat.lib().tron_values_pick(nat.ptr(counts), 2 ** 31, nat.ptr(out), nat.stream_ptr()) == nat.ERR_BAD_ARG
    assert nat.lib().tron_values_pick(None, 0, None, nat.stream_ptr()) == nat.OK
    torch.cuda.synchronize()
    assert torch.equal(out, fill)


def test_judge_none_is_todays_call_and_the_env_methods(mods):
    tv, torch = mods
    W, N = 10, 96
    codes = dev(torch, ps.soup_boards(W)[:N])
    for a, b in zip(tv.playout_codes(codes, None, 7, want_codes=True, **ps.SOUP_KEY),
                    tv.playout_codes(codes, None, 7, want_codes=True, judge=None, **ps.SOUP_KEY)):
        assert torch.equal(a, b)
    assert (tv.playout_codes(codes, None, 7, judge=None, **ps.SOUP_KEY)[1] == -1).any()
    for a, b in zip(tv.playout_values(codes, 7, 2, **pv.KEY), tv.playout_values(codes, 7, 2, judge=None, **pv.KEY)):
        assert torch.equal(a, b)
    for bad in ("voronoi", True, 1):
        with pytest.raises(ValueError):
            tv.playout_codes(codes, None, 7, judge=bad)
        with pytest.raises(ValueError):
            tv.playout_values(codes, 7, judge=bad)

    env = tv.VecTron(N, W, seed=0xABE, rank=1)
    env.reset()
    tape = rs.make_tape(N, 5, salt=2)
    env.rollout_actions(tape, rs.new_totals())
    before = env.grid().clone()
    p1 = env._p1_codes().clone()
    counts, owner = env.territory(want_owner=True)
    exp = terr.model(rs.np_(p1))
    assert np.array_equal(rs.np_(counts), exp[0]) and np.array_equal(rs.np_(owner), exp[1]) and env.territory()[1] is None
    key = dict(seed=env.seed, stream_id=env.rank, call=6)
    for a, b in zip(env.playout(k_steps=3, copies=2, call=6, judge="territory"),
                    tv.playout_codes(p1.repeat_interleave(2, dim=0), None, 3, judge="territory", **key)):
        assert (a is None and b is None) or torch.equal(a, b)
    for a, b in zip(env.playout(k_steps=3, call=6), env.playout(k_steps=3, call=6, judge=None)):
        assert (a is None and b is None) or torch.equal(a, b)
    vals = tv.playout_values(p1, 3, 2, judge="territory", **key)
    for a, b in zip(env.playout_values(3, 2, call=6, judge="territory"), vals):
        assert torch.equal(a, b)
    for player in (1, 2):
        assert torch.equal(env.montecarlo_actions(player, k_steps=3, copies=2, call=6, judge="territory"), vals[2][:, player - 1])
        assert torch.equal(env.montecarlo_actions(player, k_steps=3, copies=2, call=6),
                           env.montecarlo_actions(player, k_steps=3, copies=2, call=6, judge=None))
    assert torch.equal(env.grid(), before)
    env.close()
