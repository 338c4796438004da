"""Shared by the tests of csrc/tron_head.hip: the float64 tail of the DQN net (DQNNet.py:52-63) and the K-slice count of the head's
first product at 12x12, read through the public ABI."""

# the batches on either side of every threshold of the head's conv7 product at 12x12 ([B, 2304] x [576, 2304]^T), and the K slices
# each of them takes: 0 = no partial-sum area (the 128 x 64 tile up to 1280 rows, the 128 x 192 tile alone from 6785)
BATCHES = (1280, 1281, 2048, 3328, 3329, 6784, 6785)
SLICES = (0, 4, 4, 4, 2, 2, 0)
NARROW_ROWS = 1000                      # a batch of this many rows takes the 128 x 64 tile (it is below BATCHES[0])


def head_ref(net, x):
    """avg_pool2d(3, 2, 1) -> conv7 stride 2 pad 3 -> mish -> fc1 -> mish -> fc2 -> mish -> actor1 -> mish -> actor2 in float64."""
    import torch
    F = torch.nn.functional
    d = lambda t: t.detach().double()
    y = F.avg_pool2d(x.double(), 3, stride=2, padding=1)
    y = F.mish(F.conv2d(y, d(net.conv7.weight), d(net.conv7.bias), stride=2, padding=3)).reshape(x.shape[0], -1)
    y = F.mish(F.linear(y, d(net.fc1.weight), d(net.fc1.bias)))
    y = F.mish(F.linear(y, d(net.fc2.weight), d(net.fc2.bias)))
    return F.linear(F.mish(F.linear(y, d(net.actor1.weight), d(net.actor1.bias))), d(net.actor2.weight), d(net.actor2.bias))


def head_slices(L, B):
    """How many K slices tron_dqn_head_fwd cuts conv7's product into at batch B, side 12 (0: none), from tron_dqn_head_workspace alone.

    Every area of the workspace but one is a per-row or a fixed number of bytes rounded up to 256, so for batches that are
    multiples of 128 the size is affine in B; the exception is the partial sums of the sliced product, s * B * 576 floats.  The
    affine part is fitted at B = 128 and 256 (one and two row tiles: never sliced); what a batch asks for beyond it, in units of
    one slice (B * 2304 bytes), is s.  A ragged B adds under 4 KB of rounding against 2304 B bytes per slice."""
    ws = lambda b: int(L.tron_dqn_head_workspace(b, 12))
    per_row = (ws(256) - ws(128)) // 128
    fixed = ws(128) - 128 * per_row
    assert (ws(256) - ws(128)) % 128 == 0 and fixed > 0 and ws(384) == fixed + 384 * per_row, "the workspace is not affine at 128, 256, 384"
    extra = ws(B) - (fixed + B * per_row)
    s = round(extra / (B * 2304))
    assert abs(extra - s * B * 2304) < 4096, (B, extra)
    return s
