"""tron_playout_weighted_codes / tron_playout_weighted_values, weights= on tron.vec.playout_codes / playout_values and on
VecTron.playout / playout_values / montecarlo_actions, and play.rating's mc_weights on the GPU, against the host model of
tests/playout_support.py, the existing entries and hand-built boards.  Every comparison is exact.
tests/test_playout_weighted_model_cpu.py shows, without a GPU, that the inputs used here meet every kind of drawn move and
that a kernel which ignored the weights would fail here."""
import numpy as np
import pytest

from playout_gpu_support import mods, dev, run, same, changed_cells, composed  # noqa: F401 (mods is a fixture)
import playout_support as ps
import playout_slide_support as pss
import playout_values_support as pv
import playout_weighted_support as pw
import rollout_support as rs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("W", pw.WIDTHS)
@pytest.mark.parametrize("weights", pw.WEIGHTED)
def test_soups_against_the_model(mods, W, weights):
    """1 573 boards per width — the soup's 1 061 mid-game and rejected ones and 512 early positions with a planted dead end —
    under mode None's rule and under sliding rates, every move drawn and
    under the mixed tape (scripted and drawn bytes in one step), at k_steps 0, 1, 7 and W^2."""
    for rule in pw.RULES:
        for tape in pw.TAPES:
            boards, rates, actions = pw.soup_inputs(W, rule, tape)
            model = pw.soup_model(W, weights, rule, tape)
            for k in ps.soup_ks(W):
                same(run(mods, boards, actions, k, rates=rates, weights=weights, **pw.KEY), model[k][0], (W, weights, rule, tape, k))


@pytest.mark.parametrize("W", pw.WIDTHS)
def test_equal_weights_are_the_existing_entries(mods, W):
    """(1,1,1,1), (0,0,0,0), (7,7,7,7), (255,255,255,255): every output of tron_playout_codes, and of
    tron_playout_slide_codes with and without a uniforms tape, bit for bit."""
    tv, torch = mods
    boards, tapes, _ = ps.soup(W)
    codes, rates = dev(torch, boards), dev(torch, pss.soup_rates(W))
    u = torch.from_numpy(np.random.RandomState(40 + W).random_sample((W * W, len(boards), 2)).astype(np.float32)).cuda()
    for name in pw.TAPES:
        tape = dev(torch, tapes[name])
        for k in ps.soup_ks(W):
            for kw in ({}, dict(rates=rates), dict(rates=rates, uniforms=u)):
                plain = tv.playout_codes(codes, tape, k, want_codes=True, **kw, **ps.SOUP_KEY)
                for weights in pw.UNIFORM_EQUAL:
                    got = tv.playout_codes(codes, tape, k, want_codes=True, weights=weights, **kw, **ps.SOUP_KEY)
                    assert all(torch.equal(a, b) for a, b in zip(plain, got)), (W, name, k, sorted(kw), weights)
    for copies in (1, 3):
        for kw in ({}, dict(rates=rates[:67])):
            plain = tv.playout_values(codes[:67], W * W, copies, **kw, **pv.KEY)
            for weights in ((1, 1, 1, 1), (0, 0, 0, 0), (255, 255, 255, 255)):
                got = tv.playout_values(codes[:67], W * W, copies, weights=weights, **kw, **pv.KEY)
                assert all(torch.equal(a, b) for a, b in zip(plain, got)), (W, copies, sorted(kw), weights)


def test_dead_end_or_open(mods):
    """A head with exactly two safe moves, a dead end (room 0) and an open cell (room 3): (1,0,0,0) takes the dead end and
    (0,0,0,1) the open cell whatever the draw — for either player, in all eight orientations, under several calls and
    under both rules; nothing but the two old and the two new head cells changes."""
    boards, player, dead, opened = pw.dead_end_boards()
    m = len(boards)
    never = np.full((m, 2), -1.0)
    head_code = np.where(player == 1, 10, -10)
    for weights, move in (((1, 0, 0, 0), dead), ((0, 0, 0, 1), opened)):
        for call in (0, 1, 2, (5 << 32) | 3, 77):
            for rates in (None, never):
                steps, winner, final = run(mods, boards, None, 1, rates=rates, weights=weights, seed=9, stream_id=1, call=call)
                assert (steps == 1).all() and (winner == -1).all(), (weights, call)
                for i in range(m):
                    r, c = np.argwhere(boards[i] == head_code[i])[0]
                    tr, tc = r + ps.DR[move[i]], c + ps.DC[move[i]]
                    assert final[i, tr, tc] == head_code[i] and final[i, r, c] == (-2 if player[i] == 1 else -3), (weights, call, i)
                    assert len(changed_cells(boards[i], final[i])) == 4, (weights, call, i)
                same((steps, winner, final), ps.playout(boards, k_steps=1, seed=9, stream_id=1, call=call, rates=rates, weights=weights)[1][0],
                     (weights, call))
    # the dead end is the end: one step later its taker has no safe move, goes UP and dies
    steps, winner, _ = run(mods, boards, None, 2, rates=None, weights=(1, 0, 0, 0), seed=9, stream_id=1, call=0)
    assert (steps == 2).all() and (winner == np.where(player == 1, 2, 1)).all()


def test_borders_corners_and_a_second_wave(mods):
    """Width 4, the head in each corner and against each border — the targets that are not safe are border cells whose
    neighbours lie off the image — and two boards with EMPTY cells on the border ring: the model's result at k_steps 1, 3
    and 16 under both rules (an exact comparison of final_codes, so no stray write passes), and, counted by hand after one
    step, no cell changes but the heads' old and new cells and, under the sliding rule, the two slide tiles.  65 boards, so that a second wave of one playout runs; and the same boards from a
    tensor that starts at an odd address."""
    tv, torch = mods
    boards = pw.border_boards()
    boards = np.concatenate([boards] * (65 // len(boards) + 1))[:65]
    assert ps.decode(boards)[2].all()
    key = dict(seed=31, stream_id=2, call=(1 << 32) | 5)
    for weights in ((1, 0, 0, 0), (0, 0, 0, 1), (1, 8, 4, 2), (0, 255, 0, 1)):
        for rates in (None, np.full((65, 2), 0.5)):
            exp = ps.playout(boards, ks=(1, 3, 16), rates=rates, weights=weights, **key)
            for k in (1, 3, 16):
                got = run(mods, boards, None, k, rates=rates, weights=weights, **key)
                same(got, exp[k][0], (weights, rates is None, k))
                if k == 1:
                    assert all(len(changed_cells(b, f)) <= (4 if rates is None else 6) for b, f in zip(boards, got[2]))
            assert exp[16][1]["room0"] > 0 and exp[16][1]["no_candidate"] > 0
    raw = torch.zeros(boards.size + 3, dtype=torch.int8, device="cuda")
    odd = raw[3:].view(65, 6, 6)
    odd.copy_(dev(torch, boards))
    out = tv.playout_codes(odd, None, 16, want_codes=True, weights=(1, 8, 4, 2), **key)
    same(tuple(rs.np_(t) for t in out), ps.playout(boards, ks=(16,), weights=(1, 8, 4, 2), **key)[16][0], "odd address")
    assert np.array_equal(rs.np_(odd), boards) and not rs.np_(raw[:3]).any()


@pytest.mark.parametrize("W", pw.WIDTHS)
@pytest.mark.parametrize("weights", [(1, 8, 4, 2), (0, 255, 0, 1)])
def test_values(mods, W, weights):
    """38 boards at copies 1, 3 and 5, mode None and sliding: counts, steps and actions are the values model's at k_steps 0,
    1, 7 and W^2, and at W^2 those of the weighted codes entry at the defined launch indices."""
    tv, torch = mods
    boards = pw.values_boards(W)
    codes = dev(torch, boards)
    names = ("counts", "steps", "actions")
    for rule in pw.RULES:
        rates = pw.values_rates(W) if rule == "slide" else None
        kw = {} if rates is None else dict(rates=dev(torch, rates))
        for copies in (1, 3, 5):
            model = pw.values_soup_model(W, weights, rule, copies)
            for k in pv.ks(W):
                got = tuple(rs.np_(t) for t in tv.playout_values(codes, k, copies, weights=weights, **kw, **pw.KEY))
                same(got, model[k], (W, weights, rule, copies, k), names)
            got = tuple(rs.np_(t) for t in tv.playout_values(codes, W * W, copies, weights=weights, **kw, **pw.KEY))
            same(got, composed(mods, boards, W * W, copies, rates=rates, weights=weights, **pw.KEY), (W, weights, rule, copies), names)
        plain = tuple(rs.np_(t) for t in tv.playout_values(codes, W * W, 5, **kw, **pw.KEY))
        assert not np.array_equal(plain[0], got[0])                    # the weights are looked at


def test_argument_checks(mods):
    tv, torch = mods
    nat = tv.nat                                                       # the ctypes binding
    L = nat.lib()
    c = torch.ones(4, 35, 35, dtype=torch.int8, device="cuda")
    r = torch.zeros(4, 2, dtype=torch.float64, device="cuda")
    u = torch.zeros(3, 4, 2, dtype=torch.float32, device="cuda")
    out = torch.full((4, 4, 4, 4), 77, dtype=torch.int32, device="cuda")
    w = pw.packed((1, 8, 4, 2))

    def codes(codes, n, side, k, rates=None, uniforms=None, out_codes=None):
        return L.tron_playout_weighted_codes(nat.ptr(codes), n, side, k, None, nat.ptr(rates), nat.ptr(uniforms), w, 1, 2, 3,
                                             None, None, nat.ptr(out_codes), nat.stream_ptr())

    def values(codes, n, side, k, copies=1, rates=None, out=out):
        return L.tron_playout_weighted_values(nat.ptr(codes), n, side, k, copies, nat.ptr(rates), w, 1, 2, 3, nat.ptr(out), None,
                                              None, nat.stream_ptr())

    assert codes(c, 4, 12, 3, uniforms=u) == nat.ERR_BAD_ARG           # uniforms without rates
    for call in (codes, values):
        for rates in (None, r):
            assert call(c, 4, 5, 3, rates=rates) == nat.ERR_UNSUPPORTED and call(c, 4, 35, 3, rates=rates) == nat.ERR_UNSUPPORTED
            assert call(c, -1, 12, 3, rates=rates) == nat.ERR_BAD_ARG and call(c, 4, 12, -1, rates=rates) == nat.ERR_BAD_ARG
            assert call(None, 4, 12, 3, rates=rates) == nat.ERR_BAD_ARG
            assert call(c, 0, 12, 3, rates=rates) == nat.OK and call(None, 0, 12, 3, rates=rates) == nat.OK
    assert codes(c, 4, 12, 3, out_codes=c) == nat.ERR_BAD_ARG          # out_codes may not alias codes
    assert values(c, 4, 12, 3, copies=0) == nat.ERR_BAD_ARG and values(c, 1 << 27, 12, 3) == nat.ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == 77).all())                                     # no call above wrote anything
    # every output NULL is accepted, as in the existing entries, and writes nothing
    assert codes(c, 4, 12, 3) == nat.OK and codes(c, 4, 12, 3, rates=r, uniforms=u) == nat.OK
    assert values(c, 4, 12, 3, out=None) == nat.OK and values(c, 4, 12, 3, rates=r, out=None) == nat.OK
    torch.cuda.synchronize()
    b = c[:4, :12, :12].contiguous()
    steps, winner, final = tv.playout_codes(b[:0], k_steps=3, want_codes=True, weights=(1, 8, 4, 2))
    assert steps.numel() == 0 and winner.numel() == 0 and final.numel() == 0
    with pytest.raises(ValueError):
        tv.playout_codes(b, k_steps=3, uniforms=u, weights=(1, 8, 4, 2))
    with pytest.raises(ValueError):
        tv.playout_codes(b, k_steps=3, weights=(1, 8, 4))
    with pytest.raises(TypeError):
        tv.playout_values(b, 3, weights=(1, 8, 4, 2.5))
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", [None, "ice"])
def test_vectron(mods, mode):
    """VecTron.playout, playout_values and montecarlo_actions with weights= give what tron.vec's functions give on the
    env's codes and slide_rates(); weights=None gives what it gave; the env is left as it was."""
    tv, torch = mods
    N, W, copies, K = 200, 10, 2, 30
    a, b = (tv.VecTron(N, W, mode=mode, seed=0xABD, rank=3) for _ in range(2))
    tape = rs.make_tape(N, 6, salt=3)
    for env in (a, b):
        if mode == "ice":
            env.set_slide(torch.linspace(0.0, 0.6, N, dtype=torch.float64, device="cuda"))
        env.reset()
        for t in range(len(tape)):
            env.step(tape[t], autoreset=False)
    sliding = {} if mode is None else dict(rates=True)
    weights = tv.HUG_WEIGHTS
    got = a.playout(k_steps=K, copies=copies, call=4, want_codes=True, weights=weights, **sliding)
    values = a.playout_values(K, copies, call=4, weights=weights, **sliding)
    mc = [a.montecarlo_actions(p, K, copies, call=4, weights=weights, **sliding) for p in (1, 2)]
    none = a.playout_values(K, copies, call=4, weights=None, **sliding)
    default = a.playout_values(K, copies, call=4, **sliding)
    mc_default = a.montecarlo_actions(2, K, copies, call=4, **sliding)
    rs.check_against_twin(rs.pull(a), rs.pull(b), "after the playouts")
    boards = tv.encode_codes(a.grid(), 1)
    assert torch.equal(boards, a.obs[:, 0])
    key = dict(seed=0xABD, stream_id=3, call=4)
    rates = {} if mode is None else dict(rates=a.slide_rates())
    fork_rates = {} if mode is None else dict(rates=a.slide_rates().repeat_interleave(copies, dim=0))
    fork = boards.repeat_interleave(copies, dim=0)
    for x, y in zip(got, tv.playout_codes(fork, k_steps=K, want_codes=True, weights=weights, **fork_rates, **key)):
        assert torch.equal(x, y)
    exp = ps.playout(rs.np_(fork), k_steps=K, rates=rs.np_(fork_rates["rates"]) if fork_rates else None, weights=weights, **key)[K][0]
    same(tuple(rs.np_(t) for t in got), exp, "model")
    for x, y in zip(values, tv.playout_values(boards, K, copies, weights=weights, **rates, **key)):
        assert torch.equal(x, y)
    for x, y, z in zip(none, default, tv.playout_values(boards, K, copies, **rates, **key)):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert not torch.equal(values[0], default[0])
    for p in (0, 1):
        assert mc[p].dtype == torch.int8 and torch.equal(mc[p], values[2][:, p])
    assert torch.equal(mc_default, default[2][:, 1])
    with pytest.raises(ValueError):
        a.montecarlo_actions(2, weights=(1, 2, 3), **sliding)
    a.close()
    b.close()


def test_rating(mods):
    """play.rating hands mc_weights to both Monte-Carlo seats: the usual record, the same on a second call, and
    mc_weights=None is the call without it."""
    tv, torch = mods
    import play

    class Up:
        def act(self, x, env=None):
            return torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)

    games = 64
    args = dict(n_games=games, slides=[0.0], width=10, gamemode=None, verbose=False, max_steps=12)
    first, second = (play.rating(Up(), "montecarlo", mc_weights=tv.HUG_WEIGHTS, **args) for _ in range(2))
    assert first == second and [r["slide"] for r in first] == [0.0]
    for r in first:
        assert sorted(r) == ["draw", "p1_rate", "p1_win", "p2_win", "slide"]
        assert r["p1_win"] + r["p2_win"] + r["draw"] == games and min(r["p1_win"], r["p2_win"], r["draw"]) >= 0
    assert first[0]["p2_win"] > 0
    assert play.rating(Up(), "montecarlo", mc_weights=None, **args) == play.rating(Up(), "montecarlo", **args)
    ice = play.rating(Up(), "montecarlo-slide", mc_weights=(1, 8, 4, 2), **dict(args, gamemode="ice", slides=[0.3]))
    assert ice[0]["p1_win"] + ice[0]["p2_win"] + ice[0]["draw"] == games
    with pytest.raises(ValueError):
        play.rating(Up(), "montecarlo", mc_weights=(1, 8, 4, 2), **dict(args, gamemode="ice"))
