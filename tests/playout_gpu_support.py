"""What the GPU tests of the playout and territory entries share (tests/test_gpu_playout*.py, tests/test_gpu_territory.py):
the `mods` fixture, the entries of tron.vec called on host arrays, the exact comparison, and the definition of the values
entries run through playout_codes.  A plain module: the fixture is imported by name."""
import numpy as np
import pytest

import playout_support as ps
import rollout_support as rs

CODES, VALUES, TERRITORY = ("steps", "winner", "codes"), ("counts", "steps", "actions"), ("counts", "owner")


@pytest.fixture(scope="module")
def mods():
    tv, _ = rs.gpu_modules()
    import torch
    assert callable(tv.territory_codes) and callable(tv.territory_winner)
    return tv, torch


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(mods, boards, tape, k_steps, rates=None, uniforms=None, weights=None, **key):
    """playout_codes with want_codes on host arrays -> (steps, winner, codes) as host arrays."""
    tv, torch = mods
    s, w, c = tv.playout_codes(dev(torch, boards), dev(torch, tape), k_steps, want_codes=True, rates=dev(torch, rates),
                               uniforms=dev(torch, uniforms), weights=weights, **key)
    torch.cuda.synchronize()
    return rs.np_(s), rs.np_(w), rs.np_(c)


def run_values(mods, boards, k_steps, copies, **key):
    """playout_values on host arrays -> (counts, steps, actions) as host arrays."""
    tv, torch = mods
    out = tv.playout_values(dev(torch, boards), k_steps, copies, **key)
    torch.cuda.synchronize()
    return tuple(rs.np_(t) for t in out)


def run_territory(mods, boards, want_owner=True):
    """territory_codes on host arrays -> (counts, owner | None) as host arrays."""
    tv, torch = mods
    counts, owner = tv.territory_codes(dev(torch, boards), want_owner=want_owner)
    torch.cuda.synchronize()
    return rs.np_(counts), (None if owner is None else rs.np_(owner))


def same(got, exp, tag, names=CODES):
    """Every array of `got` is that of `exp` in dtype, shape and every element; a failure names the first rows that differ."""
    for name, g, e in zip(names, got, exp):
        assert g.dtype == e.dtype and g.shape == e.shape, (tag, name)
        if not np.array_equal(g, e):
            bad = np.nonzero((g != e).reshape(len(g), -1).any(1))[0]
            assert False, (tag, name, bad[:5], g[bad[:1]], e[bad[:1]])


def changed_cells(before, after):
    return {tuple(rc) for rc in np.argwhere(before != after)}


def composed(mods, boards, K, copies, rates=None, weights=None, **key):
    """The definition of tron_playout_values and its slide and weighted kin, run: playout_codes on the copied boards (and
    rate rows) under the constructed tape at the defined launch indices, tallied on the host."""
    tv, torch = mods
    n, per = len(boards), 16 * copies
    fanned, tape = ps.fan_out(boards, K, copies)
    kw = {} if rates is None else dict(rates=dev(torch, rates).repeat_interleave(per, dim=0))
    steps, winner, _ = tv.playout_codes(dev(torch, fanned), dev(torch, tape), K, weights=weights, **kw, **key)
    counts, total = ps.tally(rs.np_(steps), rs.np_(winner), n, copies)
    return counts, total, ps.pick(counts)
