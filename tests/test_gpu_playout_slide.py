"""tron_playout_slide_codes / tron_playout_slide_values, tron.vec.playout_codes / playout_values with rates, VecTron's
rates= keyword and play.rating's "montecarlo-slide" seat on the GPU, against the recorded sliding episodes, the host
model of tests/playout_support.py and the mode-None entries.  Every comparison is exact.
tests/test_playout_slide_model_cpu.py shows, without a GPU, that the model reproduces the recorded episodes and that the
inputs used here meet every class of step and ending."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from playout_gpu_support import mods, dev, run, same, composed  # noqa: F401 (mods is a fixture)
import playout_support as ps
import playout_slide_support as pss
import playout_values_support as pv
import rollout_support as rs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["episodes_ice_4", "episodes_temper_4"])
def test_recorded_suffixes(mods, name):
    """Every suffix of every recorded sliding episode in one launch, under the recorded uniforms and rates: the remaining
    length, the recorded winner and final_obs1."""
    boards, tape, u, rates, length, winner, final = pss.suffixes(load_golden(name))
    same(run(mods, boards, tape, len(tape), rates=rates, uniforms=u), (length, winner, final), name)


@pytest.mark.parametrize("name", ["episodes_ice_4", "episodes_ice_10", "episodes_ice_24", "episodes_temper_4",
                                  "episodes_temper_10", "episodes_temper_24"])
def test_recorded_episodes_from_the_start(mods, name):
    boards, tape, u, rates, length, winner, final = pss.starts(load_golden(name))
    same(run(mods, boards, tape, len(tape), rates=rates, uniforms=u), (length, winner, final), name)


@pytest.mark.parametrize("W", ps.SOUP_WIDTHS)
def test_soups_against_the_model(mods, W):
    """1 061 mid-game and rejected boards per width, rates over -1, 0, 0.03, 0.15, 0.5, 1, 1.5, NaN and random ones per
    player, Philox uniforms, under a full tape, no tape and a mixed tape at k_steps 0, 1, 7 and W^2."""
    boards, tapes, rates, model = pss.soup(W)
    for name, tape in tapes.items():
        for k in ps.soup_ks(W):
            exp, tally = model[name][k]
            if name == "none" and k in (1, 7):
                assert tally["unfinished"] > 0 and tally["slide"] > 0     # out_codes of an unfinished playout with slide tiles
            same(run(mods, boards, tape, k, rates=rates, **ps.SOUP_KEY), exp, (W, name, k))


def test_hand_built_boards(mods):
    """The orderings of one step, forced: player 2's slide tile on player 1's new cell, player 1's on player 2's target,
    both onto the border, a slide onto a trail — the endings worked out by hand, under a tape and under uniforms of 0."""
    boards, tape, rates, steps, winner, final = pss.hand_built()
    same(run(mods, boards, tape, 1, rates=rates), (steps, winner, final), "drawn uniforms")
    same(run(mods, boards, tape, 1, rates=rates, uniforms=np.zeros((1, 4, 2), np.float32)), (steps, winner, final), "taped uniforms")
    # ... and a uniform above every rate of 1 slides nowhere: mode None's step
    plain = ps.playout(boards, tape, k_steps=1)[1][0]
    same(run(mods, boards, tape, 1, rates=rates, uniforms=np.full((1, 4, 2), 1.25, np.float32)), plain, "no slide")


@pytest.mark.parametrize("W", [5, 24])
def test_never_sliding_is_mode_none(mods, W):
    """Rates all -1: every output of both sliding entries equals tron_playout_codes' / tron_playout_values' on the same
    inputs."""
    tv, torch = mods
    boards, tapes, _ = ps.soup(W)
    codes = dev(torch, boards)
    rates = torch.full((len(boards), 2), -1.0, dtype=torch.float64, device="cuda")
    for name, tape in tapes.items():
        for k in (1, 7, W * W):
            plain = tv.playout_codes(codes, dev(torch, tape), k, want_codes=True, **ps.SOUP_KEY)
            slide = tv.playout_codes(codes, dev(torch, tape), k, want_codes=True, rates=rates, **ps.SOUP_KEY)
            assert all(torch.equal(a, b) for a, b in zip(plain, slide)), (W, name, k)
    for copies in (1, 3):
        plain = tv.playout_values(codes[:67], W * W, copies, **pv.KEY)
        slide = tv.playout_values(codes[:67], W * W, copies, rates=rates[:67], **pv.KEY)
        assert all(torch.equal(a, b) for a, b in zip(plain, slide)), (W, copies)


def test_draw_keying(mods):
    """The draws — moves and slide uniforms — belong to (index, step, player, seed, stream_id, call) and to nothing else."""
    W, m = 10, 65
    boards, _, rates, _ = pss.soup(W)
    twice, rates2 = np.concatenate([boards[:m], boards[:m]]), np.concatenate([rates[:m], rates[:m]])
    K = W * W
    # with drawn moves and uniforms each index follows its own draws, under every key
    base = ps.playout(twice, None, k_steps=K, rates=rates2, **ps.SOUP_KEY)[K][0]
    assert not np.array_equal(base[0][:m], base[0][m:])
    same(run(mods, twice, None, K, rates=rates2, **ps.SOUP_KEY), base, "own index")
    # ... scripted moves leave the slide uniforms to the index
    tape = np.concatenate([ps.soup(W)[1]["full"][:, :m]] * 2, 1)
    scripted = ps.playout(twice, tape, k_steps=K, rates=rates2, **ps.SOUP_KEY)[K][0]
    assert not np.array_equal(scripted[2][:m], scripted[2][m:])
    same(run(mods, twice, tape, K, rates=rates2, **ps.SOUP_KEY), scripted, "scripted moves")
    # ... and a uniforms tape leaves nothing to it
    u = np.concatenate([np.random.RandomState(5).random_sample((K, m, 2)).astype(np.float32)] * 2, 1)
    got = run(mods, twice, tape, K, rates=rates2, uniforms=u, **ps.SOUP_KEY)
    same([g[:m] for g in got], [g[m:] for g in got], "same tapes")
    same(got, ps.playout(twice, tape, k_steps=K, rates=rates2, uniforms=u, **ps.SOUP_KEY)[K][0], "taped")
    for change in (dict(call=ps.SOUP_KEY["call"] + 1), dict(call=ps.SOUP_KEY["call"] + (1 << 32)), dict(seed=1),
                   dict(stream_id=6)):
        key = dict(ps.SOUP_KEY, **change)
        exp = ps.playout(twice, tape, k_steps=K, rates=rates2, **key)[K][0]
        assert not np.array_equal(exp[2], scripted[2]), change         # the moves are scripted: only the slides differ
        same(run(mods, twice, tape, K, rates=rates2, **key), exp, change)
    # a launch of the first half agrees with the launch of the whole on its rows
    same(run(mods, twice[:m], None, K, rates=rates2[:m], **ps.SOUP_KEY), [g[:m] for g in base], "half")


@pytest.mark.parametrize("W", [5, 24])
def test_output_discipline(mods, W):
    """Every subset of NULL outputs; guard rows before and behind each output stay as they were; the boards and the
    outputs start at addresses that are no multiple of 16 (or of 4), the rates one row into their buffer."""
    tv, torch = mods
    nat = tv.nat                                                       # the ctypes binding
    boards, tapes, rates_h, model = pss.soup(W)
    n, S, K = len(boards), W + 2, 7
    G, guard = S * S, 3
    exp = model["mixed"][K][0]
    raw = torch.zeros(n * G + 1, dtype=torch.int8, device="cuda")
    codes = raw[1:].view(n, S, S)                                      # an odd base address
    codes.copy_(dev(torch, boards))
    rates = torch.full((n + 1, 2), 1.0, dtype=torch.float64, device="cuda")[1:]
    rates.copy_(dev(torch, rates_h))
    tape = dev(torch, tapes["mixed"])
    key = ps.SOUP_KEY
    for subset in range(8):
        outs = [torch.full((n + 2 * guard,) + shape, 77, dtype=dtype, device="cuda")
                for shape, dtype in (((), torch.int32), ((), torch.int8), ((S, S), torch.int8))]
        ptrs = [C.c_void_p(o[guard:].data_ptr()) if (subset >> j) & 1 else None for j, o in enumerate(outs)]
        nat.check(nat.lib().tron_playout_slide_codes(nat.ptr(codes), n, S, K, nat.ptr(tape), nat.ptr(rates), None, key["seed"],
                                                     key["stream_id"], key["call"], *ptrs, nat.stream_ptr()),
                  "tron_playout_slide_codes")
        torch.cuda.synchronize()
        for j, o in enumerate(outs):
            o = rs.np_(o)
            assert (o[:guard] == 77).all() and (o[-guard:] == 77).all(), (subset, j)
            if (subset >> j) & 1:
                assert np.array_equal(o[guard:-guard], exp[j]), (subset, j)
            else:
                assert (o == 77).all(), (subset, j)
    assert np.array_equal(rs.np_(codes), boards)                       # the inputs are only read
    assert np.array_equal(rs.np_(rates), rates_h, equal_nan=True)


@pytest.mark.parametrize("W", [4, 10, 24])
def test_values_are_the_composition(mods, W):
    """67 boards at copies 1 and 3 — 1 072 and 3 216 playouts, no multiple of 64, waves that straddle boards: counts,
    steps and actions are those of tron_playout_slide_codes at the same indices; a playable board's rows sum to copies, a
    rejected board gets zeros and -1; every subset of NULL outputs between guard rows."""
    tv, torch = mods
    nat = tv.nat                                                       # the ctypes binding
    n, K = 67, W * W
    boards, rates = pss.soup(W)[0][:n], pss.soup(W)[2][:n]
    rejected = np.zeros(n, bool)
    rejected[[5, 58]] = True
    for copies in (1, 3):
        exp = composed(mods, boards, K, copies, rates=rates, **pv.KEY)
        got = tuple(rs.np_(t) for t in tv.playout_values(dev(torch, boards), K, copies, rates=dev(torch, rates), **pv.KEY))
        same(got, exp, (W, copies), ("counts", "steps", "actions"))
        assert (got[0][~rejected].sum(3) == copies).all() and (got[0][rejected] == 0).all()
        assert (got[1][rejected] == 0).all() and (got[2][rejected] == -1).all() and (got[2][~rejected] >= 0).all()
        assert got[0][..., 3].sum() == 0 and all((got[0][..., c] > 0).any() for c in range(3))
    plain = tuple(rs.np_(t) for t in tv.playout_values(dev(torch, boards), K, 3, **pv.KEY))
    assert not np.array_equal(plain[0], got[0])                        # the rates are looked at
    guard, key = 3, pv.KEY
    raw = torch.zeros(n + 1, 2, dtype=torch.float64, device="cuda")
    raw[1:] = dev(torch, rates)
    codes = dev(torch, boards)
    for subset in range(8):
        outs = [torch.full((n + 2 * guard,) + shape, 77, dtype=dtype, device="cuda")
                for shape, dtype in (((4, 4, 4), torch.int32), ((4, 4), torch.int32), ((2,), torch.int8))]
        ptrs = [C.c_void_p(o[guard:].data_ptr()) if (subset >> j) & 1 else None for j, o in enumerate(outs)]
        nat.check(nat.lib().tron_playout_slide_values(nat.ptr(codes), n, W + 2, K, 3, nat.ptr(raw[1:]), key["seed"],
                                                      key["stream_id"], key["call"], *ptrs, nat.stream_ptr()),
                  "tron_playout_slide_values")
        torch.cuda.synchronize()
        for j, o in enumerate(outs):
            o = rs.np_(o)
            assert (o[:guard] == 77).all() and (o[-guard:] == 77).all(), (subset, j)
            assert np.array_equal(o[guard:-guard], got[j]) if (subset >> j) & 1 else (o == 77).all(), (subset, j)


@pytest.mark.parametrize("mode", ["ice", "temper"])
def test_vectron(mods, mode):
    """slide_rates() is the slide / oracle.get_rate; playout(rates=True), playout_values and montecarlo_actions read the
    env's boards under them and leave the env as it was (its twin, which ran none of them, stays its twin); without rates
    a sliding env still refuses."""
    tv, torch = mods
    import oracle
    N, W, copies, K = 300, 10, 2, 20
    a, b = (tv.VecTron(N, W, mode=mode, seed=0xABC, rank=2) for _ in range(2))
    slide = torch.linspace(0.0, 0.6, N, dtype=torch.float64, device="cuda")
    tape = rs.make_tape(N, 6, salt=1)
    for env in (a, b):
        env.set_slide(slide)
        env.reset()
        for t in range(len(tape)):
            env.step(tape[t], autoreset=False)
    st = {k: rs.np_(v) for k, v in a.state().items()}
    if mode == "ice":
        exp_rates = np.repeat(rs.np_(slide)[:, None], 2, 1)
    else:
        exp_rates = np.array([[oracle.get_rate(d, w) for w in ws] for d, ws in zip(st["degree"], st["weight"])])
        assert len(np.unique(exp_rates)) > 50
    rates = a.slide_rates()
    assert rates.dtype == torch.float64 and rates.is_contiguous() and np.array_equal(rs.np_(rates), exp_rates)
    got = a.playout(k_steps=K, copies=copies, call=4, want_codes=True, rates=True)
    values = a.playout_values(K, copies, call=4, rates=True)
    mc = [a.montecarlo_actions(p, K, copies, call=4, rates=True) for p in (1, 2)]
    half = a.playout_values(K, copies, call=4, rates=rates * 0.5)      # the caller's rates
    rs.check_against_twin(rs.pull(a), rs.pull(b), "after the playouts")
    boards = tv.encode_codes(a.grid(), 1)
    assert torch.equal(boards, a.obs[:, 0])
    key = dict(seed=0xABC, stream_id=2, call=4)
    got = tuple(rs.np_(t) for t in got)
    fork, fork_rates = boards.repeat_interleave(copies, dim=0), rates.repeat_interleave(copies, dim=0)
    same(tuple(rs.np_(t) for t in tv.playout_codes(fork, k_steps=K, want_codes=True, rates=fork_rates, **key)), got, "playout_codes")
    same(got, ps.playout(rs.np_(fork), None, k_steps=K, rates=rs.np_(fork_rates), **key)[K][0], "model")
    assert (got[1] >= 0).any() and (got[1] == -1).any()
    for x, y in zip(values, tv.playout_values(boards, K, copies, rates=rates, **key)):
        assert torch.equal(x, y)
    for x, y in zip(half, tv.playout_values(boards, K, copies, rates=rates * 0.5, **key)):
        assert torch.equal(x, y)
    assert not torch.equal(half[0], values[0])
    for p in (0, 1):
        assert mc[p].dtype == torch.int8 and torch.equal(mc[p], values[2][:, p])
    for call in (lambda: a.playout(k_steps=3), lambda: a.playout_values(3), lambda: a.montecarlo_actions(2),
                 lambda: a.playout(k_steps=3, rates=rates[:5])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        a.playout(k_steps=3, rates=0.5)
    tape2 = rs.make_tape(N, 10, salt=2)
    for env in (a, b):
        for t in range(len(tape2)):
            env.step(tape2[t], autoreset=False)
    rs.check_against_twin(rs.pull(a), rs.pull(b), "after further steps")
    a.close()
    b.close()


def test_vectron_mode_none_rates(mods):
    """Mode None's slide_rates() are -1, and rates=True plays what rates=None plays."""
    tv, torch = mods
    env = tv.VecTron(64, 10, seed=3)
    env.reset()
    assert bool((env.slide_rates() == -1.0).all()) and env.slide_rates().shape == (64, 2)
    for x, y in zip(env.playout_values(30, 2, call=1), env.playout_values(30, 2, call=1, rates=True)):
        assert torch.equal(x, y)
    env.close()


def test_rating(mods):
    """play.rating seats the sliding Monte-Carlo opponent in the ice sweep: the winners are a partition of the games per
    slide value, and a second call returns the same dicts."""
    tv, torch = mods
    import play

    class Up:
        def act(self, x, env=None):
            return torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)

    games = 48
    args = dict(n_games=games, slides=[0.0, 0.3], width=10, gamemode="ice", verbose=False)
    first, second = play.rating(Up(), "montecarlo-slide", **args), play.rating(Up(), "montecarlo-slide", **args)
    assert first == second and [r["slide"] for r in first] == [0.0, 0.3]
    for r in first:
        assert r["p1_win"] + r["p2_win"] + r["draw"] == games and min(r["p1_win"], r["p2_win"], r["draw"]) >= 0
    assert sum(r["p2_win"] for r in first) > 0


def test_errors(mods):
    tv, torch = mods
    nat = tv.nat                                                       # the ctypes binding
    L = nat.lib()
    c = torch.ones(4, 35, 35, dtype=torch.int8, device="cuda")
    r = torch.zeros(4, 2, dtype=torch.float64, device="cuda")
    out = torch.full((4, 4, 4, 4), 77, dtype=torch.int32, device="cuda")

    def codes(codes, n, side, k, rates=r, out_codes=None):
        return L.tron_playout_slide_codes(nat.ptr(codes), n, side, k, None, nat.ptr(rates), None, 1, 2, 3, None, None,
                                          nat.ptr(out_codes), nat.stream_ptr())

    def values(codes, n, side, k, copies=1, rates=r):
        return L.tron_playout_slide_values(nat.ptr(codes), n, side, k, copies, nat.ptr(rates), 1, 2, 3, nat.ptr(out), None, None,
                                           nat.stream_ptr())

    for call in (codes, values):
        assert call(c, 4, 12, 3, rates=None) == nat.ERR_BAD_ARG        # NULL rates
        assert call(c, 4, 5, 3) == nat.ERR_UNSUPPORTED and call(c, 4, 35, 3) == nat.ERR_UNSUPPORTED
        assert call(c, -1, 12, 3) == nat.ERR_BAD_ARG and call(c, 4, 12, -1) == nat.ERR_BAD_ARG
        assert call(None, 4, 12, 3) == nat.ERR_BAD_ARG
        assert call(c, 0, 12, 3) == nat.OK and call(None, 0, 12, 3, rates=None) == nat.OK
    assert codes(c, 4, 12, 3, out_codes=c) == nat.ERR_BAD_ARG          # out_codes may not alias codes
    assert values(c, 4, 12, 3, copies=0) == nat.ERR_BAD_ARG and values(c, 1 << 27, 12, 3) == nat.ERR_BAD_ARG
    assert values(c, 4, 12, 1 << 30, copies=2) == nat.ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == 77).all())                                     # no call above wrote anything
    b = c[:4, :12, :12].contiguous()
    steps, winner, final = tv.playout_codes(b[:0], k_steps=3, want_codes=True, rates=r[:0])
    assert steps.numel() == 0 and winner.numel() == 0 and final.numel() == 0
    u = torch.zeros(3, 4, 2, dtype=torch.float32, device="cuda")
    for bad in (dict(rates=r.float()), dict(rates=r, uniforms=u.double()), dict(rates=[[0.0, 0.0]] * 4)):
        with pytest.raises(TypeError):
            tv.playout_codes(b, k_steps=3, **bad)
    for bad in (dict(rates=r[:3]), dict(rates=r.view(2, 4)), dict(rates=r.cpu()), dict(rates=r.repeat(1, 2)[:, ::2]),
                dict(uniforms=u), dict(rates=r, uniforms=u[:, :3]), dict(rates=r, uniforms=u.cpu()),
                dict(rates=r, uniforms=u.repeat(1, 1, 2)[:, :, ::2]), dict(rates=r, uniforms=u[:2])):
        with pytest.raises(ValueError):
            tv.playout_codes(b, k_steps=3, **bad)
    with pytest.raises(TypeError):
        tv.playout_values(b, 3, rates=r.float())
    for bad in (r[:3], r.cpu(), r.repeat(1, 2)[:, ::2]):
        with pytest.raises(ValueError):
            tv.playout_values(b, 3, rates=bad)
    assert tv.playout_codes(b, rates=r, uniforms=u)[0].shape == (4,)   # k_steps from the uniforms tape
    torch.cuda.synchronize()
