"""The float64 model of tron_adam_soft_update (csrc/tron_dqn.hip::k_adam_soft; include/tron_hip.h states the formulas), the
per-element bounds a float32 evaluation of it must meet, wrong models ("mutants") that the bounds must tell from the right one,
and the inputs of tests/test_adam_soft_model_cpu.py and tests/test_gpu_adam_soft.py.  numpy only: nothing here needs a GPU.

A single step starts from the same float32 state in the model and in the kernel, so no error compounds and every bound below is
a count of roundings, with u = 2^-24 (half an ulp, relative).  torch.optim.Adam in float32 on the CPU, one step from the same
state, stays inside the bounds in every cell of the GPU test's matrix (tests/test_adam_soft_model_cpu.py asserts it); its worst
error / bound over the matrix is 0.997 for w' and 0.99 for m' (the last rounding alone reaches the bound just above a power of
two), 0.69 for v' at normal sizes and 0.98 where v' is subnormal (g = 1e-20).  It has no soft update.

The bound of w' is `u |w'| + 10 u |dw|` (eight roundings on dw, two more from v' through the square root) plus one term the flat
form lacks: the error of m', 3 u max(|m|, |g|), carried through the formula, because it is not small against m' where m and g
cancel (optim.Adam-f32 itself is up to 147 times the flat bound there).  The bound of v' is 4 u of v' itself, not of max(v, g^2):
both of its terms are non-negative.  tolerances() shows the counts."""
import functools

import numpy as np

U = 2.0 ** -24                  # unit roundoff of float32
SUBNORMAL = 2.0 ** -149         # the smallest positive float32
DEFAULT = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)                       # optim.Adam's defaults (DDQN.py:52)
TAU = 0.001                                                               # DDQN.py's TAU

KINDS = ("unit", "1e-3", "1e-6", "eps", "1e-10", "1e-20", "1e4", "logmix", "sparse")
STATES = ("fresh", "warm")
STEPS = (1, 2, 10, 1000, 100000, 10000000)
NUMELS = (1, 7, 1023, 1024, 1025, 2048, 4097, 70001)                      # one launch of the single-step matrix
_SCALE = {"unit": 1.0, "1e-3": 1e-3, "1e-6": 1e-6, "eps": 1e-8, "1e-10": 1e-10, "1e-20": 1e-20, "1e4": 1e4, "sparse": 1e-3}


def _step(w, g, m, v, t, step, lr, b1, b2, eps, tau, variant=None):
    """include/tron_hip.h's formulas in float64; `variant` names the one deliberate error of a mutant."""
    f64 = lambda x: None if x is None else np.asarray(x, np.float64)
    w, g, m, v, t = (f64(x) for x in (w, g, m, v, t))
    with np.errstate(all="ignore"):
        w0 = w
        if g is not None:
            om1, om2 = 1.0 - b1, 1.0 - b2
            if variant == "one_minus_beta_in_f32":
                om1, om2 = float(np.float32(1) - np.float32(b1)), float(np.float32(1) - np.float32(b2))
            m = b1 * m + g if variant == "m_unscaled_gradient" else m + om1 * (g - m)
            v = b2 * v + g if variant == "v_plain_gradient" else b2 * v + om2 * g * g
            s = step - 1 if variant == "step_off_by_one" else step
            step_size = lr / (1.0 - b1 ** s)
            bc2_sqrt = 1.0 if variant == "no_bias_correction2" else np.sqrt(1.0 - b2 ** s)
            if variant == "eps_inside_correction":
                denom = (np.sqrt(v) + eps) / bc2_sqrt
            elif variant == "eps_under_root":
                denom = np.sqrt(v + eps) / bc2_sqrt
            else:
                denom = np.sqrt(v) / bc2_sqrt + eps
            w = w - step_size * (m / denom)
        if t is not None:
            src = w0 if variant == "soft_reads_old_w" else w
            t = (1.0 - tau) * src + tau * t if variant == "tau_swapped" else tau * src + (1.0 - tau) * t
    return w, m, v, t


def step64(w, g, m, v, t, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, tau=0.0):
    """One tron_adam_soft_update of one tensor in float64: returns w', m', v', t'.  g is None: no Adam step (m, v are handed
    back as given); t is None: no soft update.  Elementwise, so NaN and Inf go where IEEE sends them."""
    return _step(w, g, m, v, t, step, lr, b1, b2, eps, tau)


# name -> the same signature as step64, wrong in one way
mutants = {name: functools.partial(_step, variant=name) for name in (
    "eps_inside_correction",     # eps added before the division by sqrt(1 - b2^t)
    "eps_under_root",            # sqrt(v + eps)
    "no_bias_correction2",       # sqrt(1 - b2^t) left out
    "step_off_by_one",           # b^(t-1) in both corrections
    "v_plain_gradient",          # v <- b2 v + g
    "m_unscaled_gradient",       # m <- b1 m + g
    "tau_swapped",               # target <- (1 - tau) w + tau target
    "soft_reads_old_w",          # the soft update reads w from before the step
    "one_minus_beta_in_f32",     # 1.0f - (float)beta instead of (float)(1 - beta): what the kernel did before these tests
)}

# mutant -> (gradient kind, state, step) of the single-step matrix where it is further than 4x the bound from step64, and
# the outputs ("w", "m", "v", "t") that show it there; tests/test_adam_soft_model_cpu.py holds every row.
MUTANT_CELLS = {
    "eps_inside_correction": (("eps", "fresh", 1), "w"),          # sqrt(v) / bc2 = |g| = eps: the misplaced eps is 31x too large
    "eps_under_root": (("1e-6", "warm", 1000), "w"),              # v = 1e-12 against eps = 1e-8
    "no_bias_correction2": (("unit", "fresh", 1), "w"),           # bc2 = sqrt(0.001)
    "step_off_by_one": (("1e-3", "warm", 2), "w"),                # 1 - b1^2 against 1 - b1
    "v_plain_gradient": (("1e-3", "warm", 10), "v"),
    "m_unscaled_gradient": (("1e-6", "warm", 10), "m"),
    "tau_swapped": (("unit", "warm", 1000), "t"),
    "soft_reads_old_w": (("unit", "fresh", 1), "t"),              # tau |dw| = 1e-6 against 3 u max(|w'|, |t|) = 1e-8
    "one_minus_beta_in_f32": (("unit", "fresh", 1), "vw"),        # 1.0f - 0.999f is 1.3e-5 = 216 u off 0.001, and v' = 0.001 g^2
}


def tolerances(w, g, m, v, t, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, tau=0.0):
    """Per-element bounds on |float32 result - step64| for (w', m', v', t') of one step from float32 state; None for an output
    the step does not produce.  The kernel takes 1 - beta1, beta2, 1 - beta2, eps and tau each rounded once from double (and forms
    1 - tau in float32)."""
    w1, m1, v1, t1 = step64(w, g, m, v, t, step, lr, b1, b2, eps, tau)
    tol_w = tol_m = tol_v = tol_t = None
    with np.errstate(all="ignore"):
        if g is not None:
            g, m, v = (np.asarray(x, np.float64) for x in (g, m, v))
            # m' = fma(f32(1 - b1), g - m, m): 1 - b1 rounded to f32 (1) and the subtraction g - m (1) move (1 - b1)(g - m) by
            # 2 u (1 - b1) |g - m|, the fma rounds once, u |m'|.  An unfused m + f32(1 - b1) (g - m) (optim.Adam's lerp) rounds
            # the product as well (1): 3 u (1 - b1) |g - m| + u |m'|, the bound used.  It is never above 3 u max(|m|, |g|)
            # from b1 >= 2/3; below that the fused count, (4 (1 - b1) + 1) u <= 3 u max for b1 >= 0.5 (and at b1 = 0, where 1 - b1
            # is exact), caps it.
            assert b1 == 0.0 or b1 >= 0.5
            tol_m = np.minimum(3 * U * np.maximum(np.abs(m), np.abs(g)), 3 * U * (1.0 - b1) * np.abs(g - m) + U * np.abs(m1))
            # v' = fma(f32(b2), v, (f32(1 - b2) g) g): b2 rounded (1) moves b2 v by u b2 v; 1 - b2 rounded (1) and the two
            # products (2) move (1 - b2) g^2 by 3 u (1 - b2) g^2; the fma u v'.  Both terms are >= 0, so each is <= v':
            # u (b2 v + 3 (1 - b2) g^2) + u v' <= 4 u v' — of v' itself, not of max(v, g^2), which on fresh moments is 1000 v'.
            # An unfused b2 v + .. rounds b2 v once more: u (2 b2 v + 3 (1 - b2) g^2) + u v' <= 4 u v' as well.  A product or
            # the sum that lands below 2^-126 is rounded to a multiple of 2^-149 instead: half of it each, one subnormal.
            tol_v = 4 * U * v1 + SUBNORMAL
            # w' = w - step_size (m' / (sqrt(v') / bc2_sqrt + eps)), step_size and bc2_sqrt rounded from double.  Relative to
            # dw = w - w': step_size (1), bc2_sqrt (1), eps rounded to f32 (1), sqrt (1), / bc2_sqrt (1), + eps (1), m' / denom
            # (1), step_size * (1) = 8 u |dw|; the last subtraction u |w'|; and what m' and v' bring along, carried through:
            # tol_m step_size / denom (not small against dw where m and g cancel), and the widest move of sqrt(v') / bc2_sqrt
            # that tol_v allows, as a fraction of denom: 2 u |dw| at most wherever v' is a normal number.
            step_size, bc2_sqrt = lr / (1.0 - b1 ** step), np.sqrt(1.0 - b2 ** step)
            root = np.sqrt(v1) / bc2_sqrt
            denom = root + eps
            dw = np.abs(step_size * (m1 / denom))
            droot = (np.sqrt(v1) - np.sqrt(np.maximum(v1 - tol_v, 0.0))) / bc2_sqrt       # (sqrt is concave: the downward move is the larger)
            inherited = step_size * tol_m / denom + dw * droot / np.maximum(denom - droot, np.finfo(np.float64).tiny)
            tol_w = U * np.abs(w1) + 8 * U * dw + inherited
        if t is not None:
            # t' = fma(tau, w', (1 - tau) t): the rounding of tau moves both terms, u tau (|w'| + |t|); 1 - tau in f32 and the
            # product 2 u (1 - tau) |t|; the fma u |t'|: (2 tau + 2 (1 - tau) + 1) u = 3 u of max(|w'|, |t|); and tau of w''s error.
            tol_t = 3 * U * np.maximum(np.abs(w1), np.abs(np.asarray(t, np.float64))) + tau * (0.0 if tol_w is None else tol_w)
    return tol_w, tol_m, tol_v, tol_t


def worst_ratio(got, want, tol):
    """max |got - want| / tol over the elements where `want` is finite (inf where the two differ and tol is 0); the classes of
    the non-finite elements must agree and are checked apart (same_class)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.size == 0:
        return 0.0
    fin = np.isfinite(want)
    with np.errstate(all="ignore"):
        err = np.abs(got - want)
        r = np.where(err == 0.0, 0.0, err / tol)
    r = np.where(fin, np.where(np.isfinite(got), r, np.inf), 0.0)
    return float(r.max())


def same_class(got, want):
    """NaN where NaN, +Inf where +Inf, -Inf where -Inf, finite where finite."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))
                and np.array_equal(np.isneginf(got), np.isneginf(want)))


# ---- inputs (float32, a seed each) -------------------------------------------------------------------------------------------
def grads(kind, n, seed):
    """n float32 gradients: `unit` .. `1e4` normal at that magnitude (`eps`: 1e-8, where Adam's eps is a first-order term),
    `logmix` log-uniform in [1e-12, 1e2] with random signs, `sparse` 1e-3-sized with 90 % exact zeros."""
    rs = np.random.RandomState(seed)
    if kind == "logmix":
        return (10.0 ** rs.uniform(-12.0, 2.0, n) * rs.choice([-1.0, 1.0], n)).astype(np.float32)
    g = rs.standard_normal(n) * _SCALE[kind]
    if kind == "sparse":
        g[rs.random_sample(n) < 0.9] = 0.0
    return g.astype(np.float32)


def moments(kind, state, g, seed):
    """(m, v) in float32 for gradients g of that kind: `fresh` zeros; `warm` as after many steps at the gradients' magnitude
    (each element's own under `logmix`): m of the size of g, either sign, v of the size of g^2."""
    n = g.shape[0]
    if state == "fresh":
        return np.zeros(n, np.float32), np.zeros(n, np.float32)
    rs = np.random.RandomState(seed)
    scale = np.abs(g.astype(np.float64)) if kind == "logmix" else _SCALE[kind]
    return (scale * 0.5 * rs.standard_normal(n)).astype(np.float32), (scale * scale * rs.uniform(0.5, 1.5, n)).astype(np.float32)


def weights(n, seed):
    """n float32 weights of a layer's size (0.05), a quarter of them exactly zero: there u |w'| hides nothing of the update."""
    rs = np.random.RandomState(seed)
    w = rs.standard_normal(n) * 0.05
    w[rs.random_sample(n) < 0.25] = 0.0
    return w.astype(np.float32)


def cell_inputs(kind, state, n, seed):
    """(w, g, m, v, t) of n elements for one cell of the matrix."""
    g = grads(kind, n, seed)
    m, v = moments(kind, state, g, seed + 1)
    return weights(n, seed + 2), g, m, v, (np.random.RandomState(seed + 3).standard_normal(n) * 0.05).astype(np.float32)


def soft64(w, t, tau):
    """Agent.soft_update's formula (DDQN.py:153-165) in float64."""
    return tau * np.asarray(w, np.float64) + (1.0 - tau) * np.asarray(t, np.float64)
