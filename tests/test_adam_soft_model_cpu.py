"""tests/adam_soft_support.py held to account without a GPU: step64 is optim.Adam in double followed by the soft update, every
mutant leaves the bounds in the cell the support module names for it, and optim.Adam in float32 stays inside them in every cell."""
import numpy as np
import pytest
import torch

import adam_soft_support as S


@pytest.mark.parametrize("hyper", [dict(S.DEFAULT), dict(lr=3e-2, b1=0.5, b2=0.9, eps=1e-3), dict(lr=5e-5, b1=0.0, b2=0.99, eps=1e-12)],
                         ids=["default", "loose", "b1zero"])
def test_step64_is_double_adam_then_soft_update(hyper):
    """50 steps on float64 parameters: step64 iterated against torch.optim.Adam(foreach=False) on double tensors and the soft
    update written as DDQN.py writes it, within 1e-13 of each tensor's largest value (a few float64 ulps per step)."""
    tau, sizes = 0.01, (1, 5, 300)
    rs = np.random.RandomState(3)
    w = [rs.standard_normal(n) * 0.05 for n in sizes]
    t = [rs.standard_normal(n) * 0.05 for n in sizes]
    m, v = [np.zeros(n) for n in sizes], [np.zeros(n) for n in sizes]
    ps = [torch.nn.Parameter(torch.tensor(x, dtype=torch.float64)) for x in w]
    ts = [torch.tensor(x, dtype=torch.float64) for x in t]
    opt = torch.optim.Adam(ps, lr=hyper["lr"], betas=(hyper["b1"], hyper["b2"]), eps=hyper["eps"], foreach=False)
    for step in range(1, 51):
        for k, p in enumerate(ps):
            g = rs.standard_normal(sizes[k]) * 10.0 ** rs.uniform(-7, 0)
            p.grad = torch.tensor(g, dtype=torch.float64)
            w[k], m[k], v[k], t[k] = S.step64(w[k], g, m[k], v[k], t[k], step, tau=tau, **hyper)
        opt.step()
        with torch.no_grad():
            for p, x in zip(ps, ts):
                x.copy_(tau * p + (1.0 - tau) * x)
    for k, p in enumerate(ps):
        for mine, ref in ((w[k], p.detach()), (t[k], ts[k]), (m[k], opt.state[p]["exp_avg"]), (v[k], opt.state[p]["exp_avg_sq"])):
            ref = ref.numpy()
            assert np.abs(mine - ref).max() <= 1e-13 * np.abs(ref).max(), (k, step)


def test_step64_without_gradient_or_target():
    w, g, m, v, t = S.cell_inputs("unit", "warm", 50, 1)
    w1, m1, v1, t1 = S.step64(w, None, None, None, t, 0, tau=0.25)
    assert np.array_equal(w1, w) and m1 is None and v1 is None and np.array_equal(t1, S.soft64(w, t, 0.25))
    w1, m1, v1, t1 = S.step64(w, g, m, v, None, 3)
    assert t1 is None and not np.array_equal(w1, w)
    assert S.tolerances(w, None, None, None, t, 0, tau=0.25)[:3] == (None, None, None)
    assert S.tolerances(w, g, m, v, None, 3)[3] is None


def test_step64_sends_nonfinite_where_ieee_does():
    w, g, m, v, t = S.cell_inputs("unit", "warm", 8, 2)
    g[1], g[3], g[5] = np.nan, np.inf, -np.inf
    w1, m1, v1, t1 = S.step64(w, g, m, v, t, 4, tau=S.TAU)
    bad = np.zeros(8, bool)
    bad[[1, 3, 5]] = True
    for x in (w1, m1, v1, t1):
        assert np.array_equal(~np.isfinite(x), bad)
    assert np.isnan(m1[1]) and m1[3] == np.inf and m1[5] == -np.inf and v1[3] == np.inf and v1[5] == np.inf and np.isnan(w1[3])


@pytest.mark.parametrize("name", sorted(S.mutants))
def test_every_mutant_leaves_the_bounds_in_its_cell(name):
    """The GPU test can fail: in the cell MUTANT_CELLS names, on the GPU test's own inputs, the mutant is further than 4x the
    bound from step64 in the output named — and the cell is one of the matrix."""
    (kind, state, step), outputs = S.MUTANT_CELLS[name]
    assert kind in S.KINDS and state in S.STATES and step in S.STEPS
    ratios = dict.fromkeys("wmvt", 0.0)
    for k, n in enumerate(S.NUMELS):
        x = S.cell_inputs(kind, state, n, 100 * k)
        got = S.mutants[name](*x, step, tau=S.TAU, **S.DEFAULT)
        want = S.step64(*x, step, tau=S.TAU, **S.DEFAULT)
        tol = S.tolerances(*x, step, tau=S.TAU, **S.DEFAULT)
        for key, a, b, c in zip("wmvt", got, want, tol):
            ratios[key] = max(ratios[key], S.worst_ratio(a, b, c))
    print(name, ratios)
    for key in outputs:
        assert ratios[key] > 4.0, (name, ratios)


def test_mutant_table_is_complete():
    assert set(S.MUTANT_CELLS) == set(S.mutants) and len(S.mutants) >= 8


def _torch_f32_step(w, g, m, v, step, hyper):
    p = torch.nn.Parameter(torch.tensor(w))
    opt = torch.optim.Adam([p], lr=hyper["lr"], betas=(hyper["b1"], hyper["b2"]), eps=hyper["eps"], foreach=False)
    opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.tensor(m), "exp_avg_sq": torch.tensor(v)}
    p.grad = torch.tensor(g)
    opt.step()
    assert float(opt.state[p]["step"]) == step
    return p.detach().numpy(), opt.state[p]["exp_avg"].numpy(), opt.state[p]["exp_avg_sq"].numpy()


@pytest.mark.parametrize("state", S.STATES)
@pytest.mark.parametrize("kind", S.KINDS)
def test_float32_adam_stays_inside_the_bounds(kind, state):
    """A correct float32 implementation passes with room to spare: optim.Adam in float32 on the CPU, one step from the cell's
    float32 state, at every step count of the matrix (the worst ratios are in the support module's docstring)."""
    worst = dict.fromkeys("wmv", 0.0)
    for step in S.STEPS:
        for k, n in enumerate(S.NUMELS):
            w, g, m, v, _ = S.cell_inputs(kind, state, n, 100 * k)
            got = _torch_f32_step(w, g, m, v, step, S.DEFAULT)
            want = S.step64(w, g, m, v, None, step, **S.DEFAULT)
            tol = S.tolerances(w, g, m, v, None, step, **S.DEFAULT)
            for key, a, b, c in zip("wmv", got, want, tol):
                worst[key] = max(worst[key], S.worst_ratio(a, b, c))
    print(kind, state, worst)
    assert max(worst.values()) <= 1.0, worst
