"""One SHA-256 per cached input and model output that the playout and territory tests request, CPU only:
    python scripts/playout_model_digests.py [CHECKOUT] > digests.txt
CHECKOUT (default: this one) is the tree whose tests/ and oracle are imported, so the same script digests a parent
checkout and the result; profiles/r30_playout_model_digests.txt holds both columns side by side."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))) if len(sys.argv) < 2 else sys.argv[1]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import playout_support as ps
import playout_slide_support as pss
import playout_values_support as pv
import playout_weighted_support as pw
import territory_support as terr


def digest(x):
    """SHA-256 over every array of a nest of tuples, lists and dicts (dtype, shape and bytes; dict keys sorted)."""
    h = hashlib.sha256()

    def walk(x):
        if isinstance(x, dict):
            for k in sorted(x, key=str):
                h.update(repr(k).encode())
                walk(x[k])
        elif isinstance(x, (tuple, list)):
            for y in x:
                walk(y)
        elif x is None:
            h.update(b"None")
        else:
            a = np.ascontiguousarray(x)
            h.update(f"{a.dtype}{a.shape}".encode() + a.tobytes())
    walk(x)
    return h.hexdigest()


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def entries():
    for W in ps.SOUP_WIDTHS:
        yield f"soup({W})", ps.soup(W)
        yield f"slide soup({W})", pss.soup(W)
    for W in pw.WIDTHS:
        for rule in pw.RULES:
            for tape in pw.TAPES:
                yield f"weighted soup_inputs({W}, {rule}, {tape})", pw.soup_inputs(W, rule, tape)
                for weights in pw.WEIGHTED + ((1, 1, 1, 1),):
                    yield f"weighted soup_model({W}, {weights}, {rule}, {tape})", pw.soup_model(W, weights, rule, tape)
    for W in pv.WIDTHS:
        yield f"values boards({W})", pv.boards(W)
        yield f"values rates({W})", pw.values_rates(W)
        for copies in pv.COPIES:
            yield f"values model({W}, {copies})", pv.model(W, copies)
        for weights in ((1, 8, 4, 2), (0, 255, 0, 1)):
            for rule in pw.RULES:
                for copies in (1, 3, 5):
                    yield (f"weighted values model({W}, {weights}, {rule}, {copies})",
                           pw.values_soup_model(W, weights, rule, copies))
    for change in (dict(call=pv.KEY["call"] + 1), dict(call=pv.KEY["call"] + (1 << 32)), dict(seed=1), dict(stream_id=6)):
        yield f"values model(10, 3, {change})", pv.model(10, 3, **change)
    yield "slide hand_built", pss.hand_built()
    yield "weighted dead_end_boards", pw.dead_end_boards()
    yield "weighted border_boards", pw.border_boards()
    for name in ("none_4", "none_10"):
        yield f"suffixes({name})", ps.suffixes(golden("episodes_" + name))
    for name in ("none_4", "none_10", "none_24", "none_32", "uniform_10"):
        yield f"starts({name})", ps.starts(golden("episodes_" + name))
    for name in ("ice_4", "temper_4"):
        yield f"slide suffixes({name})", pss.suffixes(golden("episodes_" + name))
    for name in ("ice_4", "ice_10", "ice_24", "temper_4", "temper_10", "temper_24"):
        yield f"slide starts({name})", pss.starts(golden("episodes_" + name))
    for W in terr.WIDTHS:
        yield f"territory boards({W})", terr.boards(W)
        yield f"territory expected({W})", terr.expected(W)


for label, value in entries():
    print(f"{digest(value)}  {label}", flush=True)
