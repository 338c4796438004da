"""The inputs of the tron_playout_values tests (tests/test_playout_values_model_cpu.py, tests/test_gpu_playout_values.py):
38 boards of each soup, the key and the cached models.  The model is playout_support.values_model.  A plain module,
imported by name; nothing here needs a GPU."""
import playout_support as ps

WIDTHS = (4, 5, 10, 32)
COPIES = (1, 3, 4, 5)
# 38 of the soup's 1 061 boards: every 31st, and one of each kind of rejected board (no +10, two +10, a +10 on the border)
SELECT = tuple(sorted(set(range(0, ps.SOUP_N, 31)) | {5, 58, 111}))
REJECTED = (5, 58, 111)
KEY = dict(seed=0xFACADE, stream_id=9, call=(3 << 32) | 11)


def ks(W):
    return (0, 1, 7, W * W)


def boards(W):
    """The selected boards of width W, [38, S, S]."""
    return ps.soup(W)[0][list(SELECT)]


@ps.once
def model(W, copies, **change):
    """{k: (counts, steps, actions)} of boards(W) at ks(W) under KEY (with `change`)."""
    return ps.values_model(boards(W), None, copies, ks=ks(W), **dict(KEY, **change))
