"""tron_adam_soft_update (csrc/tron_dqn.hip::k_adam_soft: Adam's step of every tensor and the target net's soft update in one
launch) against tests/adam_soft_support.py's float64 model, one step at a time from identical float32 state under bounds that
count the kernel's roundings, and over a 300-step run against what optim.Adam in float32 loses over the same run.  The kernel
tests call the C entry point; every tensor is a slice of one flat device buffer that starts at an odd element offset between
64 sentinel floats, and every test ends by comparing the sentinels bit for bit.  tests/test_adam_soft_model_cpu.py shows that
each of nine wrong models leaves these bounds in a cell of the matrix below.

Observed on an MI355X, error / bound at the worst element of the whole single-step matrix: w' 0.997 (1e-10, fresh, step 10) and
m' 0.99 (logmix, warm, step 1) — the last rounding alone reaches the bound just above a power of two —, v' 0.98 (1e-20, warm,
step 1: subnormal v; 0.69 at normal sizes), t' 0.73 (1e-3, fresh, step 2).
Observed over the 300-step run, the kernel's deviation from float64 / optim.Adam-f32's, worst tensor and step: w 1.00, m 1.00,
v 1.09, target 1.05 (bound: 2).
The kernel these tests were first run against formed 1 - beta as 1.0f - (float)beta on the device (1.3e-5 off 0.001 for beta2).
It is the support module's `one_minus_beta_in_f32` model: one step from fresh moments puts its v' at 54 times the bound and its w'
at 8 times, and a numpy float32 evaluation of the 300-step run puts it up to 775 (v), 11 (m) and 51 (w) times further from
float64 than optim.Adam-f32, the ulp taken off."""
import ctypes as C
import functools

import numpy as np
import pytest

import adam_soft_support as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import tron.vec as tv  # noqa: E402

nat = tv.nat                                                            # the ctypes binding of the library

PAD = 64


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


class Arena:
    """One flat float32 buffer: add() reserves a slice at an odd offset with PAD sentinels (distinct NaN patterns) either side."""

    def __init__(self):
        self.slices, self.size = [], 0

    def add(self, data):
        start = self.size + PAD
        start += 1 - start % 2
        self.slices.append((start, np.ascontiguousarray(data, np.float32)))
        self.size = start + len(data) + PAD
        return len(self.slices) - 1

    def upload(self):
        host = (0x7FC00000 | (np.arange(self.size, dtype=np.int64) & 0xFFFFF)).astype(np.uint32).view(np.float32).copy()
        self.guard = np.ones(self.size, bool)
        for start, d in self.slices:
            host[start:start + len(d)] = d
            self.guard[start:start + len(d)] = False
        self.host0 = host.copy()
        self.dev = torch.from_numpy(host).cuda()
        return self

    def ptr(self, h):
        return self.dev.data_ptr() + 4 * self.slices[h][0]

    def view(self, h):
        start, d = self.slices[h]
        return self.dev[start:start + len(d)]

    def download(self):
        torch.cuda.synchronize()
        self.out = self.dev.cpu().numpy()

    def get(self, h):
        start, d = self.slices[h]
        return self.out[start:start + len(d)]

    def sentinels_intact(self):
        return np.array_equal(_bits(self.out)[self.guard], _bits(self.host0)[self.guard])

    def unchanged(self):
        return _same_bits(self.out, self.host0)


def job(w, g, m, v, t, step):
    """One tensor of a launch: float32 arrays; g None = target-only (m, v may be None too), t None = a null targets[k]."""
    return dict(w=w, g=g, m=m, v=v, t=t, step=step)


def launch(jobs, hyper=S.DEFAULT, tau=S.TAU, whole_targets=True):
    """Lays the jobs out in an Arena, calls tron_adam_soft_update once and downloads: (status, arena, handles)."""
    ar, hs = Arena(), []
    for j in jobs:
        hs.append({k: ar.add(j[k]) for k in "wgmvt" if j[k] is not None})
    ar.upload()
    n = len(jobs)
    P, G, M, V, T = ((C.c_void_p * n)() for _ in range(5))
    numel, steps = (C.c_int64 * n)(), (C.c_double * n)()
    for k, (j, h) in enumerate(zip(jobs, hs)):
        for arr, key in ((P, "w"), (G, "g"), (M, "m"), (V, "v"), (T, "t")):
            if key in h:
                arr[k] = ar.ptr(h[key])
        numel[k], steps[k] = len(j["w"]), float(j["step"])
    rc = nat.lib().tron_adam_soft_update(n, P, G, M, V, T if whole_targets else None, numel, steps, hyper["lr"], hyper["b1"],
                                         hyper["b2"], hyper["eps"], float(tau), nat.stream_ptr())
    ar.download()
    return rc, ar, hs


def verify(jobs, ar, hs, hyper=S.DEFAULT, tau=S.TAU, whole_targets=True):
    """Every job against step64 under tolerances(); what a job must not write bit-unchanged; the sentinels.  Returns the worst
    error / bound per output."""
    worst = dict.fromkeys("wmvt", 0.0)
    for k, (j, h) in enumerate(zip(jobs, hs)):
        soft = whole_targets and j["t"] is not None
        t_in = j["t"] if soft else None
        if j["g"] is not None:
            assert _same_bits(ar.get(h["g"]), j["g"]), (k, "g")
        if j["g"] is None:                                               # target-only: w, m, v as they were
            for key in "wmv":
                assert key not in h or _same_bits(ar.get(h[key]), j[key]), (k, key, "written without a gradient")
            got = dict(t=ar.get(h["t"])) if soft else {}
            want = S.step64(j["w"], None, None, None, t_in, j["step"], tau=tau, **hyper)
            tol = S.tolerances(j["w"], None, None, None, t_in, j["step"], tau=tau, **hyper)
        else:
            got = {key: ar.get(h[key]) for key in ("wmvt" if soft else "wmv")}
            want = S.step64(j["w"], j["g"], j["m"], j["v"], t_in, j["step"], tau=tau, **hyper)
            tol = S.tolerances(j["w"], j["g"], j["m"], j["v"], t_in, j["step"], tau=tau, **hyper)
        if not soft and "t" in h:
            assert _same_bits(ar.get(h["t"]), j["t"]), (k, "target written without a soft update")
        for key, b, c in zip("wmvt", want, tol):
            if key in got:
                assert S.same_class(got[key], b), (k, key, "non-finite elements differ")
                r = S.worst_ratio(got[key], b, c)
                assert r <= 1.0, (k, key, len(j["w"]), j["step"], r)
                worst[key] = max(worst[key], r)
    assert ar.sentinels_intact()
    return worst


@functools.lru_cache(maxsize=None)
def _cell(kind, state, numels=S.NUMELS):
    return tuple(S.cell_inputs(kind, state, n, 100 * k) for k, n in enumerate(numels))


@pytest.mark.parametrize("step", S.STEPS)
@pytest.mark.parametrize("state", S.STATES)
@pytest.mark.parametrize("kind", S.KINDS)
def test_single_step_matches_float64(kind, state, step):
    """One launch of eight tensors (1 .. 70 001 elements: below, at and past the 1 024-element chunk) at default hyper-parameters
    and tau = 0.001: w', m', v', t' elementwise within the counted bounds of step64."""
    jobs = [job(*x, step) for x in _cell(kind, state)]
    rc, ar, hs = launch(jobs)
    assert rc == 0
    print("single-step", kind, state, step, verify(jobs, ar, hs))


_HYPER = ([("lr", dict(S.DEFAULT, lr=lr), S.TAU) for lr in (1e-2, 5e-5)]
          + [("betas", dict(S.DEFAULT, b1=b1, b2=b2), S.TAU) for b1, b2 in ((0.0, 0.0), (0.5, 0.9), (0.9, 0.999))]
          + [("eps", dict(S.DEFAULT, eps=e), S.TAU) for e in (0.0, 1e-8, 1e-3)]
          + [("tau", dict(S.DEFAULT), tau) for tau in (0.0, 0.001, 0.5, 1.0)])


@pytest.mark.parametrize("state", S.STATES)
@pytest.mark.parametrize("what,hyper,tau", _HYPER, ids=[f"{w}-{h['lr']}-{h['b1']}-{h['b2']}-{h['eps']}-{t}" for w, h, t in _HYPER])
def test_hyperparameters(what, hyper, tau, state):
    """The logmix cell (no zero gradient, so eps = 0 divides by no zero) at step 10 under other hyper-parameters; tau = 0 leaves
    the targets' bits, tau = 1 makes them the new weights' bits."""
    cell = _cell("logmix", state, (1, 7, 1023, 1025, 4097))
    assert all((x[1] != 0).all() for x in cell)
    jobs = [job(*x, 10) for x in cell]
    rc, ar, hs = launch(jobs, hyper, tau)
    assert rc == 0
    print("hyper", what, hyper, tau, state, verify(jobs, ar, hs, hyper, tau))
    for j, h in zip(jobs, hs):
        if tau == 0.0:
            assert _same_bits(ar.get(h["t"]), j["t"])
        if tau == 1.0:
            assert _same_bits(ar.get(h["t"]), ar.get(h["w"]))


def test_per_tensor_step_counts():
    """steps[k] is per tensor: four tensors with the same state and gradients at counts 1, 3, 1 000 and 1e6 each match step64
    at their own count (eps-sized gradients on warm state: both bias corrections are first-order there)."""
    x = S.cell_inputs("eps", "warm", 1025, 7)
    jobs = [job(*x, step) for step in (1, 3, 1000, 1000000)]
    rc, ar, hs = launch(jobs)
    assert rc == 0
    verify(jobs, ar, hs)
    ws = [ar.get(h["w"]) for h in hs]
    assert all(not np.array_equal(ws[a], ws[b]) for a in range(4) for b in range(a))
    assert all(_same_bits(ar.get(h["m"]), ar.get(hs[0]["m"])) and _same_bits(ar.get(h["v"]), ar.get(hs[0]["v"])) for h in hs)


def _layout(name):
    """(jobs, whole_targets) of one launch layout: `full` a stepped tensor with a target, `tonly` no gradient, `notarget` a null
    targets[k]; sizes <= 3 000, some of them multiples of the chunk."""
    rs = np.random.RandomState(len(name))
    whole = True

    def make(n, role="full", seed=0):
        w, g, m, v, t = S.cell_inputs("1e-3", "warm", n, 1000 + seed)
        if role == "tonly":
            return job(w, None, m if seed % 2 else None, v if seed % 2 else None, t, 0)
        if role == "idle":                                               # neither gradient nor target: the entry point skips it
            return job(w, None, None, None, None, 0)
        return job(w, g, m, v, None if role == "notarget" else t, 1 + seed % 7)

    def sizes(count):
        s = rs.randint(1, 3001, count)
        s[::5] = rs.choice([1024, 2048, 1, 3000, 1023, 1025], len(s[::5]))
        return [int(x) for x in s]

    if name.startswith("count"):
        jobs = [make(n, seed=k) for k, n in enumerate(sizes(int(name[5:])))]
    elif name == "zeros":
        jobs = [make(n, seed=k) for k, n in enumerate([0, 5, 0, 1024, 0, 0, 7, 2048, 0])]
    elif name == "zeros_across_seam":                                     # 40 entries, 33 of them non-empty: the second launch starts after skipped ones
        jobs = [make(0 if k % 6 == 5 or k == 0 else n, seed=k) for k, n in enumerate(sizes(40))]
        jobs.append(make(0, seed=99))
    elif name == "target_only_between":
        jobs = [make(n, "tonly" if k % 2 else "full", seed=k) for k, n in enumerate(sizes(9))]
    elif name == "null_targets_k":
        jobs = [make(n, "notarget" if k % 3 == 1 else "full", seed=k) for k, n in enumerate(sizes(10))]
    elif name == "targets_null":
        jobs, whole = [make(n, "tonly" if k == 2 else "full", seed=k) for k, n in enumerate(sizes(6))], False
    elif name == "all_target_only":
        jobs = [make(n, "tonly", seed=k) for k, n in enumerate(sizes(35))]
    elif name == "mixed":
        roles = ["full", "tonly", "notarget", "idle", "full", "full", "tonly"]
        jobs = [make(0 if k % 11 == 3 else n, roles[k % 7], seed=k) for k, n in enumerate(sizes(70))]
    elif name == "65x1024":
        jobs = [make(1024, seed=k) for k in range(65)]
    return jobs, whole


@pytest.mark.parametrize("name", ["count1", "count31", "count32", "count33", "count64", "count65", "zeros", "zeros_across_seam",
                                  "target_only_between", "null_targets_k", "targets_null", "all_target_only", "mixed", "65x1024"])
def test_launch_layouts(name):
    """Job lists around TRON_ADAM_MAX_TENSORS = 32 per launch, with empty, target-only and target-less tensors in every position."""
    jobs, whole = _layout(name)
    rc, ar, hs = launch(jobs, whole_targets=whole)
    assert rc == 0
    verify(jobs, ar, hs, whole_targets=whole)
    stepped = [k for k, j in enumerate(jobs) if j["g"] is not None and len(j["w"])]
    assert all(not np.array_equal(ar.get(hs[k]["w"]), jobs[k]["w"]) for k in stepped)      # (and the launch did run)


def test_launch_of_no_tensors():
    assert nat.lib().tron_adam_soft_update(0, None, None, None, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.5, nat.stream_ptr()) == 0
    torch.cuda.synchronize()


def test_nonfinite_gradients_stay_in_their_element():
    """One NaN, one +Inf and one -Inf gradient among 5 000: those three elements of w', m', v', t' are non-finite in step64's
    class (verify() compares the classes), every other element is inside its bound."""
    w, g, m, v, t = S.cell_inputs("unit", "warm", 5000, 3)
    g[17], g[1024], g[4999] = np.nan, np.inf, -np.inf
    jobs = [job(w, g, m, v, t, 4)]
    rc, ar, hs = launch(jobs)
    assert rc == 0
    verify(jobs, ar, hs)
    bad = np.zeros(5000, bool)
    bad[[17, 1024, 4999]] = True
    for key in "wmvt":
        assert np.array_equal(~np.isfinite(ar.get(hs[0][key])), bad), key


@pytest.mark.parametrize("state", S.STATES)
def test_zero_gradient_elements(state):
    """90 % exact zeros: where g == 0 the moments only decay (m' = b1 m, v' = b2 v, within their bounds) and, on fresh state,
    the weight keeps its bits."""
    n = 6000
    w, g, m, v, t = S.cell_inputs("sparse", state, n, 5)
    zero = g == 0
    assert 0.85 * n < zero.sum() < 0.95 * n
    jobs = [job(w, g, m, v, t, 3)]
    rc, ar, hs = launch(jobs)
    assert rc == 0
    verify(jobs, ar, hs)
    tol_w, tol_m, tol_v, tol_t = S.tolerances(w, g, m, v, t, 3, tau=S.TAU, **S.DEFAULT)
    m1, v1, w1 = (ar.get(hs[0][k]).astype(np.float64) for k in "mvw")
    assert (np.abs(m1 - S.DEFAULT["b1"] * m.astype(np.float64)) <= tol_m)[zero].all()
    assert (np.abs(v1 - S.DEFAULT["b2"] * v.astype(np.float64)) <= tol_v)[zero].all()
    if state == "fresh":
        assert _same_bits(ar.get(hs[0]["w"])[zero], w[zero]) and not (m1[zero] != 0).any() and not (v1[zero] != 0).any()
    else:
        assert (w1[zero] != w[zero]).mean() > 0.5                        # warm moments still move the weight


def _params_in_arena(arrays, extra=()):
    """Parameters (and further tensors) that are views of one Arena buffer."""
    ar = Arena()
    hs = [ar.add(a) for a in list(arrays) + list(extra)]
    ar.upload()
    return ar, hs


def test_trajectory_tracks_float64():
    """300 steps of AdamSoft.step(targets, tau = 0.001) on four tensors, gradients shrinking from 1e-2 to 1e-7: at steps 1, 10,
    100 and 300 the kernel's largest deviation from step64 iterated in float64 is at most twice that of optim.Adam(foreach=False)
    in float32 on the CPU (plus the reference soft update) fed the same gradients, plus one float32 ulp of the tensor's largest
    value — per tensor, for w, m, v and the target.  The bound is the reference implementation's own loss, not the kernel's;
    the 2 allows another, equally valid order of roundings.  Observed ratios: see the module docstring."""
    import DDQN
    sizes, tau, marks = (1, 1023, 4097, 20000), S.TAU, (1, 10, 100, 300)
    w0 = [S.weights(n, 10 + k) for k, n in enumerate(sizes)]
    t0 = [(np.random.RandomState(20 + k).standard_normal(n) * 0.05).astype(np.float32) for k, n in enumerate(sizes)]
    ar, hs = _params_in_arena(w0, t0 + [np.zeros(n, np.float32) for n in sizes])
    ps = [torch.nn.Parameter(ar.view(h)) for h in hs[:4]]
    ts, gs = [ar.view(h) for h in hs[4:8]], [ar.view(h) for h in hs[8:]]
    mine = DDQN.AdamSoft(ps)
    qs = [torch.nn.Parameter(torch.tensor(w)) for w in w0]
    us = [torch.tensor(t) for t in t0]
    ref = torch.optim.Adam(qs, foreach=False)
    D = [dict(w=w.astype(np.float64), m=np.zeros(len(w)), v=np.zeros(len(w)), t=t.astype(np.float64)) for w, t in zip(w0, t0)]
    rs = np.random.RandomState(5)
    worst = {}
    for step in range(1, 301):
        scale = 10.0 ** (-2.0 - 5.0 * (step - 1) / 299.0)
        for k, n in enumerate(sizes):
            g = (rs.standard_normal(n) * scale).astype(np.float32)
            gs[k].copy_(torch.from_numpy(g))
            ps[k].grad = gs[k]
            qs[k].grad = torch.from_numpy(g)
            d = D[k]
            d["w"], d["m"], d["v"], d["t"] = S.step64(d["w"], g, d["m"], d["v"], d["t"], step, tau=tau, **S.DEFAULT)
        assert mine.step(targets=ts, tau=tau) is True
        ref.step()
        with torch.no_grad():
            for q, u in zip(qs, us):
                u.copy_(tau * q + (1.0 - tau) * u)
        if step in marks:
            for k in range(4):
                K = dict(w=ps[k], m=mine.state[ps[k]]["exp_avg"], v=mine.state[ps[k]]["exp_avg_sq"], t=ts[k])
                T = dict(w=qs[k], m=ref.state[qs[k]]["exp_avg"], v=ref.state[qs[k]]["exp_avg_sq"], t=us[k])
                for key in "wmvt":
                    want = D[k][key]
                    dev_k = np.abs(K[key].detach().cpu().numpy() - want).max()
                    dev_t = np.abs(T[key].detach().numpy() - want).max()
                    ulp = float(np.spacing(np.float32(np.abs(want).max())))
                    print(f"trajectory step {step} numel {sizes[k]} {key}: kernel {dev_k:.3e} adam-f32 {dev_t:.3e} ulp {ulp:.1e}")
                    if dev_t > 0:
                        worst[key] = max(worst.get(key, 0.0), dev_k / dev_t)
                    assert dev_k <= 2.0 * dev_t + ulp, (step, sizes[k], key, dev_k, dev_t, ulp)
    print("trajectory kernel / adam-f32, worst:", worst)
    assert float(mine.state[ps[0]]["step"]) == 300.0
    ar.download()
    assert ar.sentinels_intact()


def test_entry_point_arguments():
    """Every refused call returns TRON_ERR_BAD_ARG and has written nothing — the bad tensor is number 40 of 48, past the first
    launch of 32, so a check made launch by launch would have updated the first 32 already."""
    n, bad = 48, 40
    cells = [S.cell_inputs("1e-3", "warm", 40 + 29 * k, k) for k in range(n)]
    ar = Arena()
    hs = [{key: ar.add(x) for key, x in zip("wgmvt", c)} for c in cells]
    ar.upload()

    def call(n_=n, null=(), hyper=None, tau=S.TAU, **at_bad):
        arrs = {key: (C.c_void_p * n)() for key in "wgmvt"}
        numel, steps = (C.c_int64 * n)(), (C.c_double * n)()
        for k, h in enumerate(hs):
            for key in "wgmvt":
                arrs[key][k] = ar.ptr(h[key])
            numel[k], steps[k] = len(cells[k][0]), 3.0
        for key, val in at_bad.items():
            if key == "numel":
                numel[bad] = val
            elif key == "steps":
                steps[bad] = val
            else:
                arrs[key][bad] = val                                     # (None: a null pointer)
        hy = dict(S.DEFAULT, **(hyper or {}))
        args = [None if key in null else arrs[key] for key in "wgmvt"] + [None if "numel" in null else numel, None if "steps" in null else steps]
        rc = nat.lib().tron_adam_soft_update(n_, *args, hy["lr"], hy["b1"], hy["b2"], hy["eps"], float(tau), nat.stream_ptr())
        ar.download()
        return rc

    nan = float("nan")
    refused = [("n < 0", dict(n_=-1))]
    refused += [(f"null {key} array", dict(null=(key,))) for key in ("w", "g", "m", "v", "numel", "steps")]
    refused += [(f"{key} = {val}", dict(hyper={key: val})) for key, val in (("b1", 1.0), ("b1", -0.1), ("b2", 1.0), ("b2", -0.1), ("eps", -1e-8),
                                                                             ("lr", nan), ("b1", nan), ("b2", nan), ("eps", nan))]
    refused += [(f"tau = {tau}", dict(tau=tau)) for tau in (-0.1, 1.1, nan)]
    refused += [("steps[k] = 0 with a gradient", dict(steps=0.0)), ("null exp_avg[k] with a gradient", dict(m=None)),
                ("null exp_avg_sq[k] with a gradient", dict(v=None)), ("null params[k]", dict(w=None)), ("numel[k] < 0", dict(numel=-1)),
                ("numel[k] = 2^31 - 1024", dict(numel=2 ** 31 - 1024))]
    for what, kw in refused:
        assert call(**kw) == nat.ERR_BAD_ARG, what
        assert ar.unchanged(), what + ": a refused call wrote to a buffer"
    assert call(null=("t",)) == 0                                        # (a null targets array is no error) ...
    jobs = [job(*c, 3.0) for c in cells]
    verify(jobs, ar, hs, whole_targets=False)                            # ... and the same arguments, accepted, are one good step


def test_wrapper_refusals():
    """What DDQN.AdamSoft refuses before it calls the kernel, and the two ways a step count reaches it that are not the plain one."""
    import DDQN
    dev = "cuda"
    P = lambda *shape: torch.nn.Parameter(torch.randn(*shape, device=dev) * 0.05)

    def one_step(opt, params, **kw):
        for p in params:
            p.grad = torch.full_like(p, 1e-3)
        return opt.step(**kw)

    p = torch.nn.Parameter((torch.randn(6, 8, device=dev) * 0.05).t())                   # non-contiguous
    with pytest.raises(TypeError):
        one_step(DDQN.AdamSoft([p]), [p])
    p = torch.nn.Parameter(torch.randn(5, device=dev, dtype=torch.float64))
    with pytest.raises(TypeError):
        one_step(DDQN.AdamSoft([p]), [p])
    p = P(4, 3)
    with pytest.raises(TypeError):
        one_step(DDQN.AdamSoft([p]), [p], targets=[torch.zeros(3, 4, device=dev)], tau=0.1)
    with pytest.raises(ValueError):
        one_step(DDQN.AdamSoft([p]), [p], targets=[torch.zeros(4, 3, device=dev)] * 2, tau=0.1)
    q = P(2)
    with pytest.raises(NotImplementedError):
        one_step(DDQN.AdamSoft([{"params": [p]}, {"params": [q], "lr": 1e-2}]), [p, q])
    for kw in (dict(weight_decay=1e-2), dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(NotImplementedError):
            one_step(DDQN.AdamSoft([p], **kw), [p])

    # a checkpoint of the fused form keeps `step` on the device: accepted, brought to the host, counted on
    w, g, m, v, t = S.cell_inputs("1e-6", "warm", 1025, 11)
    ar, hs = _params_in_arena([w, g, t])
    p = torch.nn.Parameter(ar.view(hs[0]))
    opt = DDQN.AdamSoft([p])
    opt.state[p] = {"step": torch.tensor(5.0, device=dev), "exp_avg": torch.tensor(m, device=dev), "exp_avg_sq": torch.tensor(v, device=dev)}
    p.grad = ar.view(hs[1])
    assert opt.step(targets=[ar.view(hs[2])], tau=S.TAU) is True
    st = opt.state[p]
    assert not st["step"].is_cuda and float(st["step"]) == 6.0
    ar.download()
    got = (ar.get(hs[0]), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy(), ar.get(hs[2]))
    want, tol = S.step64(w, g, m, v, t, 6, tau=S.TAU, **S.DEFAULT), S.tolerances(w, g, m, v, t, 6, tau=S.TAU, **S.DEFAULT)
    assert all(S.worst_ratio(a, b, c) <= 1.0 for a, b, c in zip(got, want, tol)) and ar.sentinels_intact()

    # a parameter whose first gradient arrives at the optimizer's third step counts from one
    w, g, _, _, t = S.cell_inputs("1e-3", "fresh", 777, 12)
    w2, g2, _, _, t2 = S.cell_inputs("1e-3", "fresh", 130, 13)
    ar, hs = _params_in_arena([w, w2, g, g2, t, t2])
    early, late = (torch.nn.Parameter(ar.view(h)) for h in hs[:2])
    opt = DDQN.AdamSoft([early, late])
    ew, em, ev, et = w, np.zeros_like(w), np.zeros_like(w), t
    lt = t2
    for step in (1, 2, 3):
        early.grad, late.grad = ar.view(hs[2]), (ar.view(hs[3]) if step == 3 else None)
        opt.step(targets=[ar.view(hs[4]), ar.view(hs[5])], tau=S.TAU)
        assert (late in opt.state and len(opt.state[late]) > 0) == (step == 3)
        ar.download()
        if step < 3:                                                     # (each step is held to float64 from the state it started at)
            assert _same_bits(ar.get(hs[1]), w2)
            want, tol = S.step64(w2, None, None, None, lt, 0, tau=S.TAU), S.tolerances(w2, None, None, None, lt, 0, tau=S.TAU)
            assert S.worst_ratio(ar.get(hs[5]), want[3], tol[3]) <= 1.0
        else:
            assert float(opt.state[late]["step"]) == 1.0 and float(opt.state[early]["step"]) == 3.0
            z = np.zeros_like(w2)
            got = (ar.get(hs[1]), opt.state[late]["exp_avg"].cpu().numpy(), opt.state[late]["exp_avg_sq"].cpu().numpy(), ar.get(hs[5]))
            want, tol = S.step64(w2, g2, z, z, lt, 1, tau=S.TAU, **S.DEFAULT), S.tolerances(w2, g2, z, z, lt, 1, tau=S.TAU, **S.DEFAULT)
            assert all(S.worst_ratio(a, b, c) <= 1.0 for a, b, c in zip(got, want, tol))
            wrong = S.step64(w2, g2, z, z, lt, 3, tau=S.TAU, **S.DEFAULT)                  # (the optimizer's own count would show)
            assert S.worst_ratio(got[0], wrong[0], tol[0]) > 4.0
        want, tol = S.step64(ew, g, em, ev, et, step, tau=S.TAU, **S.DEFAULT), S.tolerances(ew, g, em, ev, et, step, tau=S.TAU, **S.DEFAULT)
        got = (ar.get(hs[0]), opt.state[early]["exp_avg"].cpu().numpy(), opt.state[early]["exp_avg_sq"].cpu().numpy(), ar.get(hs[4]))
        assert all(S.worst_ratio(a, b, c) <= 1.0 for a, b, c in zip(got, want, tol)), step
        ew, em, ev, et = (x.copy() for x in got)
        lt = ar.get(hs[5]).copy()
    assert ar.sentinels_intact()
