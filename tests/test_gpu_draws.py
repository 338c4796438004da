"""The DDQN loop's random draws and its loss's tie rule against their definitions, bit for bit: tron_eps_greedy,
the replay sampler (tron_replay_sample / tron_replay_sample_codes + tron_replay_indices, and both gathers on rows that are
no multiple of four bytes) and tron_ddqn_td_loss against the numpy models of tests/draws_support.py, which
tests/test_draws_model_cpu.py ties to the oracle's Philox."""
import math

import numpy as np
import pytest

import draws_support as ds

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import tron.vec as tv  # noqa: E402

nat = tv.nat                                                            # the ctypes binding of the library


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- epsilon-greedy -----------------------------------------------------------------------------------------------------
def eps_greedy(greedy, eps, seed, stream, call, n=None):
    out = torch.full_like(greedy, 9)
    e = dev(np.array([eps], np.float32))
    nat.check(nat.lib().tron_eps_greedy(nat.ptr(greedy), greedy.numel() if n is None else n, nat.ptr(e), seed, stream, call,
                                        nat.ptr(out), nat.stream_ptr()), "tron_eps_greedy")
    return out


@pytest.mark.parametrize("n,eps_name,call,key", ds.eps_cases())
def test_eps_greedy_equals_the_model(n, eps_name, call, key):
    eps = ds.EPSILONS[eps_name]
    greedy = np.random.RandomState(n % 1000).randint(0, 4, n).astype(np.int8)
    want = ds.eps_greedy_model(greedy, eps, *key, call)
    if n == ds.EPS_BIG_N and eps_name == "2^-17":                      # the boundary case must have something at the boundary
        assert np.any((ds.eps_greedy_words(n, *key, call) >> 16) == 0)
    g = dev(greedy)
    got = eps_greedy(g, eps, *key, call)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(g.cpu(), torch.from_numpy(greedy))              # the input is read, not written


def test_eps_greedy_boundary_explores_exactly_the_zero_draws():
    """epsilon = 2^-17 = u(h == 0): exactly the observations whose 16 deciding bits are zero explore (about 64 of the
    4 194 309), one ulp below none does.  The greedy action 4 cannot be drawn, so every explored entry shows."""
    n, key, call = ds.EPS_BIG_N, (11, 3), 2 ** 32 + 1
    zero_h = (ds.eps_greedy_words(n, *key, call) >> 16) == 0
    assert zero_h.sum() >= 1
    g = torch.full((n,), 4, dtype=torch.int8, device="cuda")
    at = eps_greedy(g, ds.EPSILONS["2^-17"], *key, call).cpu().numpy()
    assert np.array_equal(at != 4, zero_h)
    below = eps_greedy(g, ds.EPSILONS["below 2^-17"], *key, call)
    assert bool((below == 4).all())


def test_eps_greedy_of_nothing_writes_nothing():
    g = torch.zeros(8, dtype=torch.int8, device="cuda")
    out = eps_greedy(g, 1.0, 1, 2, 3, n=0)
    assert bool((out == 9).all())
    e = torch.ones(1, device="cuda")
    assert nat.lib().tron_eps_greedy(nat.ptr(g), -1, nat.ptr(e), 1, 2, 3, nat.ptr(out), nat.stream_ptr()) == nat.ERR_BAD_ARG
    assert bool((out == 9).all())


def test_act_batch_counts_its_calls_from_one():
    """DDQN.Agent.act_batch draws under key (seed, rank) with the call counter incremented BEFORE each launch: a fresh
    agent's calls are 1, 2, ...; a restored counter goes on from where it stood, past 2^32 too.  It hands the kernel a
    buffer of its own: the greedy actions are not overwritten (no in-place use to test)."""
    import DDQN
    brain = DDQN.Agent(10, 3, device="cuda", make_memory=False, seed=11, rank=3)
    n = 999
    vals = torch.tensor([1, -1, -2, -3, 10, -10], dtype=torch.int8, device="cuda")
    torch.manual_seed(3)
    obs = vals[torch.randint(0, 6, (n, 12, 12), device="cuda")]
    greedy = brain.qnetwork_local.infer(obs, codes=True, greedy=True).cpu().numpy()
    assert greedy.dtype == np.int8 and greedy.shape == (n,)
    eps = torch.full((1,), 0.3, device="cuda")
    assert brain._eps_calls == 0
    for call in (1, 2):
        got = brain.act_batch(obs, eps, codes=True)
        assert brain._eps_calls == call
        assert np.array_equal(got.cpu().numpy(), ds.eps_greedy_model(greedy, 0.3, 11, 3, call))
    brain._eps_calls = 2 ** 32 - 1                                      # what load_checkpoint restores
    for call in (2 ** 32, 2 ** 32 + 1):
        got = brain.act_batch(obs, eps, codes=True)
        assert brain._eps_calls == call
        assert np.array_equal(got.cpu().numpy(), ds.eps_greedy_model(greedy, 0.3, 11, 3, call))


# ---- the replay sampler -------------------------------------------------------------------------------------------------
def ring(capacity, cells, seed, rank, rows=None, states=None, next_states=None):
    """A DeviceReplay with `rows` (default: all) transitions pushed: zeros, or the given code rows; row i has action
    i % 4, reward i and done i % 2."""
    rb = tv.DeviceReplay(capacity, cells, seed=seed, rank=rank)
    n = capacity if rows is None else rows
    z = torch.zeros(n, cells, dtype=torch.int8, device="cuda")
    i = torch.arange(n, device="cuda")
    rb.add(z if states is None else dev(states), (i % 4).to(torch.int8), i.float(), z if next_states is None else dev(next_states),
           (i % 2).to(torch.int8))
    return rb


def draw(rb, batch, codes=False, channels=3, plane4=0.0):
    """One tron_replay_sample (or _sample_codes) into buffers sized by the ring's own `cells` -> (the five outputs, indices)."""
    shape = (batch, rb.cells) if codes else (batch, channels, rb.cells)
    st = torch.full(shape, 77, dtype=torch.int8 if codes else torch.float32, device="cuda")
    s2 = torch.full_like(st, 77)
    a = torch.empty(batch, dtype=torch.int64, device="cuda")
    r, d = torch.empty(batch, device="cuda"), torch.empty(batch, device="cuda")
    L = nat.lib()
    if codes:
        rc = L.tron_replay_sample_codes(rb._h, batch, nat.ptr(st), nat.ptr(a), nat.ptr(r), nat.ptr(s2), nat.ptr(d), nat.stream_ptr())
    else:
        rc = L.tron_replay_sample(rb._h, batch, channels, float(plane4), nat.ptr(st), nat.ptr(a), nat.ptr(r), nat.ptr(s2), nat.ptr(d),
                                  nat.stream_ptr())
    nat.check(rc, "tron_replay_sample")
    return (st, a, r, s2, d), rb.last_indices(batch).cpu().numpy()


@pytest.mark.parametrize("size,batch", ds.SAMPLER_CASES)
def test_sampler_indices_equal_the_model(size, batch):
    cells = 1 + size % 16 if size < 5000 else 1                        # 1 ... 16; the large rings stay at a byte per row
    seed, rank = 1000 + size, size % 3
    rb = ring(size, cells, seed, rank)
    for call in range(3):
        (st, a, r, s2, d), idx = draw(rb, batch, codes=bool(call & 1))
        want = ds.sample_indices_model(size, batch, seed, rank, call)
        assert np.array_equal(idx, want), (size, batch, call)
        assert rb.cursor() == (0, size, call + 1)
        assert np.array_equal(r.cpu().numpy(), want.astype(np.float32))     # row i's reward is i: the gather read those slots
        assert np.array_equal(a.cpu().numpy(), want % 4) and np.array_equal(d.cpu().numpy(), (want % 2).astype(np.float32))
    rb.close()


def test_sampler_on_a_partly_filled_ring_and_its_call_counter():
    """size is the fill level, not the capacity; sample and sample_codes share one counter; a refused sample consumes
    no call; the counter wraps at 2^32; get_cursor reports it after every draw."""
    cap, rows, cells, seed, rank = 1000, 300, 9, 77, 2
    rb = ring(cap, cells, seed, rank, rows=rows)
    assert rb.cursor() == (rows, rows, 0)
    for call, (batch, codes) in enumerate([(300, False), (17, True), (300, True), (1, False), (64, False), (64, True)]):
        _, idx = draw(rb, batch, codes=codes)
        assert np.array_equal(idx, ds.sample_indices_model(rows, batch, seed, rank, call)), call
        assert rb.cursor() == (rows, rows, call + 1)
    for codes in (False, True):                                         # batch > size: refused, nothing drawn
        with pytest.raises(nat.TronNativeError):
            draw(rb, rows + 1, codes=codes)
        assert rb.cursor() == (rows, rows, 6)
    _, idx = draw(rb, 300)
    assert np.array_equal(idx, ds.sample_indices_model(rows, 300, seed, rank, 6))
    nat.check(nat.lib().tron_replay_set_cursor(rb._h, rows, rows, 0xFFFFFFFE), "tron_replay_set_cursor")
    for k, call in enumerate((0xFFFFFFFE, 0xFFFFFFFF, 0)):
        _, idx = draw(rb, 256, codes=bool(k & 1))
        assert np.array_equal(idx, ds.sample_indices_model(rows, 256, seed, rank, call)), hex(call)
        assert rb.cursor() == (rows, rows, (call + 1) & 0xFFFFFFFF)
    rb.close()


def test_sampler_streams():
    a, b, c = (ring(500, 4, 9, rank) for rank in (0, 1, 0))
    ia, ib, ic = (draw(rb, 400)[1] for rb in (a, b, c))
    assert np.array_equal(ia, ic) and not np.array_equal(ia, ib)
    assert np.array_equal(ia, ds.sample_indices_model(500, 400, 9, 0, 0)) and np.array_equal(ib, ds.sample_indices_model(500, 400, 9, 1, 0))
    for rb in (a, b, c):
        rb.close()


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("cells", [1, 9, 121])
def test_gather_on_rows_that_are_no_multiple_of_four_bytes(cells, channels):
    """k_sample_gather's and k_sample_gather_codes's byte-wise branch: sample == the host expansion of the rows at the
    model's indices, sample_codes == the raw rows.  The ring holds the six observation codes and a few bytes that are
    none (0, 2, -128, 127: empty cells in every plane)."""
    rs = np.random.RandomState(cells)
    vals = np.array([1, -1, -2, -3, 10, -10, 0, 2, -128, 127], np.int8)
    rows = 37
    s, s2 = vals[rs.randint(0, 10, (rows, cells))], vals[rs.randint(0, 10, (rows, cells))]
    s[:10, 0], s2[:10, 0] = vals, vals[::-1]                            # every byte value occurs, whatever `cells`
    seed, rank = 21, 1
    rb = ring(50, cells, seed, rank, rows=rows, states=s, next_states=s2)
    for call, batch in enumerate((rows, 5)):
        (st, a, r, st2, d), idx = draw(rb, batch, channels=channels, plane4=5.0)
        want = ds.sample_indices_model(rows, batch, seed, rank, call)
        assert np.array_equal(idx, want)
        assert np.array_equal(st.cpu().numpy(), ds.expand_codes(s[want], channels, 5.0))
        assert np.array_equal(st2.cpu().numpy(), ds.expand_codes(s2[want], channels, 5.0))
        assert np.array_equal(r.cpu().numpy(), want.astype(np.float32)) and np.array_equal(a.cpu().numpy(), want % 4)
        assert np.array_equal(d.cpu().numpy(), (want % 2).astype(np.float32))
    (st, a, r, st2, d), idx = draw(rb, rows, codes=True)
    want = ds.sample_indices_model(rows, rows, seed, rank, 2)
    assert np.array_equal(idx, want)
    assert np.array_equal(st.cpu().numpy(), s[want]) and np.array_equal(st2.cpu().numpy(), s2[want])
    assert np.array_equal(r.cpu().numpy(), want.astype(np.float32)) and np.array_equal(a.cpu().numpy(), want % 4)
    rb.close()


def test_expand_codes_is_pop_up():
    """The host expansion the gather is held to is the project's pop_up (tron_pop_up) on the observation codes."""
    vals = np.array([1, -1, -2, -3, 10, -10], np.int8)
    codes = vals[np.random.RandomState(0).randint(0, 6, (20, 11, 11))]
    got = tv.pop_up_planes(dev(codes)).cpu().numpy()
    assert np.array_equal(got.reshape(20, 3, 121), ds.expand_codes(codes.reshape(20, 121), 3, 0.0))


# ---- the TD loss --------------------------------------------------------------------------------------------------------
NEG_INF = -math.inf
PLANTS = ([1.5, 1.5, 1.5, 1.5],                                         # all four equal
          [2.0, -1.0, 0.5, 2.0], [-1.0, 2.0, 0.5, 2.0], [-1.0, 0.5, 2.0, 2.0],   # equal maxima at (0, 3), (1, 3), (2, 3)
          [0.0, -0.0, -1.0, -2.0], [-0.0, 0.0, -1.0, -2.0],               # the two zeros compare equal: the earlier one wins
          [NEG_INF] * 4)                                                # nothing is greater than the first


def td_inputs(B, seed):
    rs = np.random.RandomState(seed)
    f = np.float32
    q, ql, qt = (rs.randn(B, 4).astype(f) for _ in range(3))
    a = rs.randint(0, 4, B).astype(np.int64)
    r = rs.randn(B).astype(f)
    d = (rs.rand(B) < 0.3).astype(f)
    plants = np.array(PLANTS, f)
    if B >= 14:                                                         # every planted row in the first and in the last 64 rows
        first = rs.permutation(min(B // 2, 64))[:7]
        last = B - 1 - rs.permutation(min(B // 2, 64))[:7]
        where = np.concatenate([first, last])
    else:
        where = rs.permutation(B)[:7]                                   # B = 7: one of each; B = 1: see the test
    ql[where] = plants[np.arange(len(where)) % 7]
    d[where] = 0.0                                                      # the arg-max matters only where the game goes on
    assert len(np.unique(where)) == len(where)
    return q, a, r, d, ql, qt


def td_launch(q, a, r, d, ql, qt, gamma):
    t = [dev(v) for v in (q, a, r, d, ql, qt)]
    loss = torch.full((1,), -1.0, device="cuda")
    grad = torch.full((q.shape[0], 4), 7.0, device="cuda")
    nat.check(nat.lib().tron_ddqn_td_loss(*[nat.ptr(v) for v in t], float(gamma), q.shape[0], nat.ptr(loss), nat.ptr(grad),
                                          nat.stream_ptr()), "tron_ddqn_td_loss")
    return loss.cpu().numpy(), grad.cpu().numpy()


def td_check(inputs, gamma):
    """grad_q bit for bit; the loss within (ceil(B / 1024) + 24) 2^-24 relative of the float64 sum of the exact e^2 — the
    longest chain of roundings in the kernel (a square, the thread's adds, six shuffle steps, sixteen partials, one
    multiply by the rounded 1 / B) over non-negative terms; the same bits from a second launch."""
    B = inputs[0].shape[0]
    want_loss, want_grad, _ = ds.td_model(*inputs, gamma)
    loss, grad = td_launch(*inputs, gamma)
    assert np.array_equal(grad.view(np.int32), want_grad.view(np.int32))
    bound = (math.ceil(B / 1024) + 24) * 2.0 ** -24
    err = abs(float(loss[0]) - want_loss)
    print(f"td loss B {B} gamma {gamma}: {float(loss[0])!r} vs {want_loss!r}, relative error {err / want_loss:.3g} (bound {bound:.3g})")
    assert math.isfinite(want_loss) and want_loss > 0 and err <= bound * want_loss
    loss2, grad2 = td_launch(*inputs, gamma)
    assert np.array_equal(loss2.view(np.int32), loss.view(np.int32)) and np.array_equal(grad2.view(np.int32), grad.view(np.int32))


@pytest.mark.parametrize("gamma", [0.0, 0.95, 1.0])
@pytest.mark.parametrize("B", [1, 7, 1023, 1024, 1025, 2049])
def test_td_loss_equals_the_model(B, gamma):
    if B > 1:
        inputs = td_inputs(B, B)
        planted = sum(int(np.array_equal(row.view(np.int32), np.array(p, np.float32).view(np.int32))) for row in inputs[4] for p in PLANTS)
        assert planted == (14 if B >= 14 else 7)
        assert set(inputs[3].tolist()) == {0.0, 1.0} or B == 7
        td_check(inputs, gamma)
        return
    for k, plant in enumerate(PLANTS):                                  # one row: each planted row in turn, both values of done
        q, a, r, d, ql, qt = td_inputs(1, k)
        ql[0] = np.array(plant, np.float32)
        for done in (0.0, 1.0):
            d[0] = done
            td_check((q, a, r, d, ql, qt), gamma)


def test_td_loss_through_the_autograd_function():
    import DDQN
    B, gamma = 1025, 0.95
    q, a, r, d, ql, qt = td_inputs(B, 5)
    want_loss, want_grad, _ = ds.td_model(q, a, r, d, ql, qt, gamma)
    tq = dev(q).requires_grad_(True)
    ta, tr, td_, tql, tqt = dev(a).reshape(B, 1), dev(r).reshape(B, 1), dev(d).reshape(B, 1), dev(ql), dev(qt)
    assert DDQN._td_fusable(tq, ta, tr, td_, tql, tqt)
    loss = DDQN._TDLoss.apply(tq, ta, tr, td_, tql, tqt, gamma)
    loss.backward()
    assert np.array_equal(tq.grad.cpu().numpy().view(np.int32), want_grad.view(np.int32))
    assert abs(loss.item() - want_loss) <= (math.ceil(B / 1024) + 24) * 2.0 ** -24 * want_loss
