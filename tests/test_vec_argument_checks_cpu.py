"""The argument checks of tron/vec.py's playout, territory and tape entries that fire before the first native call: every
bad call with the exception type and the exact message it raises, on host tensors.  The last row of each entry is the
call that passes every check and is refused where the first device pointer is taken, which pins the order.  Needs
libtron_hip.so for the import alone.  No GPU."""
import pytest
import torch

import tron.vec as tv

Native = tv.nat.TronNativeError
HOST = "tron kernels take device tensors; got a CPU tensor"
B = torch.ones(2, 6, 6, dtype=torch.int8)                              # two boards of side 6
TAPE = torch.zeros(3, 2, 2, dtype=torch.int8)
U = torch.zeros(3, 2, 2, dtype=torch.float32)
R = torch.zeros(2, 2, dtype=torch.float64)
I8, F32, F64 = "torch.int8", "torch.float32", "torch.float64"


def meta(t):
    return torch.empty(t.shape, dtype=t.dtype, device="meta")


def strided(t):
    """The same shape and dtype, not contiguous."""
    return torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype)[..., ::2]


def env(n=3, mode=None):
    """A VecTron whose checks can run without a device: they read N, device and mode alone."""
    e = tv.VecTron.__new__(tv.VecTron)
    e.N, e.device, e.mode = n, torch.device("cpu"), mode
    return e


def codes(*a, **kw):
    return lambda: tv.playout_codes(B, *a, **kw)


def values(*a, **kw):
    return lambda: tv.playout_values(B, *a, **kw)


def weights_rows(what, call):
    return [
        (call(weights=5), TypeError, f"{what}: weights is None or a sequence of four ints 0..255"),
        (call(weights=(1, 2, 3)), ValueError, f"{what}: weights are four, one per room 0..3, got 3"),
        (call(weights=(1.0, 2, True, "3")), TypeError, f"{what}: weights are ints, got ['float', 'int', 'bool', 'str']"),
        (call(weights=(1, 2, 3, 256)), ValueError, f"{what}: weights are 0..255, got [1, 2, 3, 256]"),
        (call(weights=(-1, 2, 3, 4)), ValueError, f"{what}: weights are 0..255, got [-1, 2, 3, 4]"),
    ]


def rates_rows(what, call):
    return [
        (call(rates=[[0.5, 0.5]] * 2), TypeError, f"{what}: rates is None or a float64 tensor [n, 2]"),
        (call(rates=R.float()), TypeError, f"{what}: rates are float64, got {F32}"),
        (call(rates=R[:1]), ValueError, f"{what}: expected rates of shape (2, 2), got (1, 2)"),
        (call(rates=R.view(4)), ValueError, f"{what}: expected rates of shape (2, 2), got (4,)"),
        (call(rates=meta(R)), ValueError, f"{what}: rates must be on cpu, got meta"),
        (call(rates=strided(R)), ValueError, f"{what}: rates must be contiguous"),
    ]


def boards_rows(what, fn):
    return [
        (lambda: fn(B.float()), ValueError, f"{what} takes int8 boards [n, S, S], got {F32} (2, 6, 6)"),
        (lambda: fn(B[0]), ValueError, f"{what} takes int8 boards [n, S, S], got {I8} (6, 6)"),
        (lambda: fn(B[:, :5]), ValueError, f"{what} takes int8 boards [n, S, S], got {I8} (2, 5, 6)"),
    ]


CASES = (
    # ---- playout_codes, in the order its checks fire ---------------------------------------------------------------
    [(codes(k_steps=3, judge="voronoi"), ValueError, "playout_codes: judge is None or \"territory\", got 'voronoi'"),
     (lambda: tv.playout_codes(B.float(), k_steps=3, judge="x"), ValueError,
      "playout_codes: judge is None or \"territory\", got 'x'")]
    + boards_rows("playout_codes", lambda b: tv.playout_codes(b, k_steps=3, weights=5))
    + weights_rows("playout_codes", lambda **kw: codes(TAPE.float(), **kw))
    + [(codes(TAPE.float()), ValueError, f"expected an int8 tape of shape (K, 2, 2), got {F32} (3, 2, 2)"),
       (codes(TAPE[0]), ValueError, f"expected an int8 tape of shape (K, 2, 2), got {I8} (2, 2)"),
       (codes(TAPE[:, :1]), ValueError, f"expected an int8 tape of shape (K, 2, 2), got {I8} (3, 1, 2)"),
       (codes(TAPE, 4, uniforms=U), ValueError, "k_steps 4 is more than the tape's 3 rows"),
       (codes(TAPE, uniforms=U), ValueError, "uniforms belong to the sliding rule: pass rates with them"),
       (codes(k_steps=3, uniforms=[0.5], rates=5), TypeError, "uniforms is None or a float32 tensor [K, n, 2]"),
       (codes(k_steps=3, uniforms=U.double(), rates=5), TypeError, f"the uniforms are float32, got {F64}"),
       (codes(k_steps=3, uniforms=U[0], rates=5), ValueError,
        "expected a float32 uniforms tape of shape (K, 2, 2), got (2, 2)"),
       (codes(k_steps=3, uniforms=U[:, :, :1], rates=5), ValueError,
        "expected a float32 uniforms tape of shape (K, 2, 2), got (3, 2, 1)"),
       (codes(k_steps=3, uniforms=meta(U), rates=5), ValueError, "the uniforms must be on cpu, got meta"),
       (codes(k_steps=3, uniforms=strided(U), rates=5), ValueError, "the uniforms must be contiguous"),
       (codes(k_steps=4, uniforms=U, rates=5), ValueError, "k_steps 4 is more than the uniforms tape's 3 rows"),
       (codes(TAPE[:2], uniforms=U, rates=R), Native, HOST),              # k_steps is the tape's 2 rows: within the uniforms' 3
       (codes(rates=5), ValueError, "playout_codes needs k_steps when there is no tape")]
    + rates_rows("playout_codes", lambda **kw: codes(k_steps=3, **kw))
    + [(codes(uniforms=U, rates=R), Native, HOST),                        # k_steps from the uniforms tape
       (codes(TAPE, rates=R, weights=(1, 8, 4, 2), judge="territory"), Native, HOST),
       (codes(k_steps=0), Native, HOST)]
    # ---- playout_values ----------------------------------------------------------------------------------------------
    + [(values(3, judge="voronoi"), ValueError, "playout_values: judge is None or \"territory\", got 'voronoi'")]
    + boards_rows("playout_values", lambda b: tv.playout_values(b, -1, weights=5))
    + weights_rows("playout_values", lambda **kw: values(-1, **kw))
    + [(values(-1, 0), ValueError, "k_steps is at least 0"),
       (values(3, 0, rates=5), ValueError, "copies is at least 1"),
       (values(3, 2 ** 26, rates=5), ValueError, f"2 boards x 16 moves x {2 ** 26} copies do not fit the 32-bit playout index"),
       (values(2 ** 30, 2, rates=5), ValueError, f"2 copies x {2 ** 30} steps do not fit a 32-bit sum of steps")]
    + rates_rows("playout_values", lambda **kw: values(3, **kw))
    + [(values(3, rates=R, weights=(0, 4, 2, 1)), Native, HOST),
       (values(3, judge="territory"), Native, HOST)]
    # ---- territory_codes ---------------------------------------------------------------------------------------------
    + boards_rows("territory_codes", tv.territory_codes)
    + [(lambda: tv.territory_codes(B, want_owner=True), Native, HOST)]
    # ---- the two helpers on their own --------------------------------------------------------------------------------
    + weights_rows("x", lambda **kw: (lambda: tv._packed_weights(kw["weights"], "x")))
    + [(lambda: tv._checked_judge("territories", "y"), ValueError, "y: judge is None or \"territory\", got 'territories'"),
       (lambda: tv._checked_judge(0, "y"), ValueError, "y: judge is None or \"territory\", got 0")]
    # ---- VecTron.rollout_actions and its record tapes, N = 3 ---------------------------------------------------------
    + [(lambda: env().rollout_actions([[0, 1]] * 3), TypeError, "rollout_actions takes an int8 tensor [K, N, 2]"),
       (lambda: env().rollout_actions(torch.zeros(4, 3, 2)), TypeError, f"rollout_actions takes int8 actions, got {F32}"),
       (lambda: env().rollout_actions(torch.zeros(3, 2, dtype=torch.int8)), ValueError, "expected shape (K, 3, 2), got (3, 2)"),
       (lambda: env().rollout_actions(torch.zeros(4, 2, 2, dtype=torch.int8)), ValueError,
        "expected shape (K, 3, 2), got (4, 2, 2)"),
       (lambda: env().rollout_actions(torch.empty(4, 3, 2, dtype=torch.int8, device="meta")), ValueError,
        "the tape must be on cpu, got meta"),
       (lambda: env().rollout_actions(strided(torch.zeros(4, 3, 2, dtype=torch.int8))), ValueError,
        "the tape must be contiguous"),
       (lambda: env().rollout_actions(torch.zeros(4, 3, 2, dtype=torch.int8), records=5), TypeError,
        "records is None, True or a tuple (reward, done, winner)"),
       (lambda: env()._record_tapes((None, None), 4), TypeError, "records is None, True or a tuple (reward, done, winner)"),
       (lambda: env()._record_tapes(([0.0], None, None), 4), TypeError,
        f"the reward records take a {F32} tensor (4, 3, 2) or None"),
       (lambda: env()._record_tapes((None, 1, None), 4), TypeError, f"the done records take a {I8} tensor (4, 3) or None"),
       (lambda: env()._record_tapes((torch.zeros(4, 3, 2, dtype=torch.float64), None, None), 4), TypeError,
        f"the reward records are {F32}, got {F64}"),
       (lambda: env()._record_tapes((None, None, torch.zeros(4, 3)), 4), TypeError, f"the winner records are {I8}, got {F32}"),
       (lambda: env()._record_tapes((torch.zeros(4, 3), None, None), 4), ValueError,
        "expected reward records of shape (4, 3, 2), got (4, 3)"),
       (lambda: env()._record_tapes((None, torch.zeros(5, 3, dtype=torch.int8), None), 4), ValueError,
        "expected done records of shape (4, 3), got (5, 3)"),
       (lambda: env()._record_tapes((None, None, torch.empty(4, 3, dtype=torch.int8, device="meta")), 4), ValueError,
        "the winner records must be on cpu, got meta"),
       (lambda: env()._record_tapes((strided(torch.zeros(4, 3, 2)), None, None), 4), ValueError,
        "the reward records must be contiguous"),
       # the first fault in (reward, done, winner) order is the one reported
       (lambda: env()._record_tapes((None, torch.zeros(4, 3), torch.zeros(1)), 4), TypeError, f"the done records are {I8}, got {F32}")]
    # ---- VecTron's rates argument ------------------------------------------------------------------------------------
    + [(lambda: env(mode="ice")._playout_rates(None, "playout"), ValueError,
        "playout without rates plays mode None's rule; in a sliding mode pass rates=True (this env's slide_rates()) or a "
        "float64 [N, 2] tensor"),
       (lambda: env()._playout_rates(0.5, "playout_values"), TypeError, "rates is None, True or a float64 tensor [N, 2]"),
       (lambda: env()._playout_rates(torch.zeros(3), "playout"), ValueError, "expected rates of shape (3, 2), got (3,)"),
       (lambda: env(mode="ice").playout(copies=0, rates=torch.zeros(3, 2)), ValueError, "copies is at least 1")]
)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_bad_call(case):
    call, exc, message = CASES[case]
    with pytest.raises(exc) as caught:
        call()
    assert type(caught.value) is exc and str(caught.value) == message


def test_what_passes():
    """The checks hand on what they accept, unchanged: records as given or freshly allocated, an empty tape's records
    before any launch, the packed weights, rates as given."""
    e = env()
    reward, done = torch.zeros(4, 3, 2), torch.zeros(4, 3, dtype=torch.int8)
    given = (reward, done, None)
    assert e._record_tapes(given, 4) is given
    made = e._record_tapes(True, 4)
    assert [(t.dtype, tuple(t.shape)) for t in made] == [(torch.float32, (4, 3, 2)), (torch.int8, (4, 3)), (torch.int8, (4, 3))]
    empty = torch.zeros(0, 3, 2, dtype=torch.int8)
    assert e.rollout_actions(empty) is None and [tuple(t.shape) for t in e.rollout_actions(empty, records=True)] == [
        (0, 3, 2), (0, 3), (0, 3)]
    assert tv._packed_weights((1, 8, 4, 2), "x") == 0x02040801 and tv._packed_weights([0, 0, 0, 255], "x") == 0xFF000000
    assert tv._checked_judge(None, "x") is None and tv._checked_judge("territory", "x") is None
    rates = torch.zeros(3, 2, dtype=torch.float64)
    assert e._playout_rates(rates, "playout") is rates and e._playout_rates(None, "playout") is None
