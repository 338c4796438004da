"""csrc/tron_head.hip, the inference head (tron_dqn_head_fwd and its PX16 and pooled entries), on every path its first product
takes.  At 12x12 conv7 runs densely as [B, 2304] x [576, 2304]^T and wide_splitk sends it to k_gemm_f16x3 (B <= 1280), to
k_gemm_wide in four K slices + k_gemm_finish (to 3328), in two (to 6784), or to k_gemm_wide alone — with an epilogue no other
caller has: one bias per nine columns, mish, split-f16 outputs.  head_support.BATCHES are the batches on both sides of every
threshold (tests/test_head_dispatch_cpu.py proves it through the workspace query, and so does the fixture below).

Also here: exact ties in k_q_head's greedy action, and the workspace contract (stays inside tron_dqn_head_workspace bytes, reads
from it only what the same call wrote, refuses bad arguments before any launch)."""
import pytest

from head_support import BATCHES, NARROW_ROWS, SLICES, head_ref, head_slices

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
TOL = 1e-5                    # Q against float64: the bound of tests/test_gpu_conv.py and tests/test_gpu_conv_ws.py on this data
PATHS = 2e-6                  # two head paths on the same values (test_head_from_px16_equals_head_from_f32)


@pytest.fixture(scope="module")
def fused():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from Net import fused
    got = tuple(head_slices(fused.nat.lib(), B) for B in BATCHES)
    assert got == SLICES, f"the dispatch thresholds moved ({dict(zip(BATCHES, got))}): move head_support.BATCHES with them"
    return fused


def _net(W=10, cin=3):
    from Net.DQNNet import Net
    return Net(cin, W).cuda()


def _rows(fused, inp, n):
    """The first n batch rows of a head input (f32 tensor, PX16 image or Pooled12 rows) as an input of its own kind."""
    if isinstance(inp, fused.Pooled12):                                  # [hi rows of the whole batch | lo rows], each half padded to 256
        B = inp.shape[0]
        out = fused.Pooled12(n, inp.buf.device)
        half, half_n = inp.buf.numel() // 2, out.buf.numel() // 2
        assert half >= B * 4608 and half_n >= n * 4608
        out.buf.zero_()
        out.buf[:n * 4608] = inp.buf[:n * 4608]
        out.buf[half_n:half_n + n * 4608] = inp.buf[half:half + n * 4608]
        return out
    if isinstance(inp, fused.PX16):                                      # images are contiguous: 4 bytes per value
        _, C, S, _ = inp.shape
        out = fused.PX16(n, C, S, inp.buf.device)
        out.buf.copy_(inp.buf[:out.buf.numel()])
        return out
    return inp[:n].contiguous()


def _inputs(fused, net, entry, B):
    """(what the entry takes, the f32 values the kernel sees ahead of the pooling) for a trunk output of randn * 1.5."""
    x = torch.randn(B, 64, 12, 12, device="cuda") * 1.5
    if entry == "f32":
        return x, x
    xp = fused.PX16.from_f32(x)                                          # tron_px16_from_f32
    if entry == "px16":
        return xp, xp.float()
    # conv6 + residual with the pooling in the same launch, and the PX16 image the two-launch path writes from the same operands
    rp = fused.PX16.from_f32(torch.randn(B, 64, 12, 12, device="cuda"))
    w = fused.ws_split_weights([net.conv6])[0]
    return fused.conv_ws_pool12(xp, net.conv6, w, rp), fused.conv_ws(xp, net.conv6, w, residual=rp).float()


@pytest.mark.parametrize("entry", ["f32", "px16", "pooled"])
@pytest.mark.parametrize("B", BATCHES)
def test_head_on_every_gemm_path_matches_float64(fused, B, entry):
    """Q within 1e-5 of the float64 tail on the values the entry sees; greedy = argmax of that Q, also from the greedy-only call;
    and the first 1000 rows run alone (the 128 x 64 tile) agree with the same rows of the whole batch to 2e-6 — not bit for bit:
    the slices change the order of the sum over K."""
    torch.manual_seed(B)
    net = _net(10, 3 if B % 2 else 4)
    inp, seen = _inputs(fused, net, entry, B)
    q, g = fused.head(net, inp, want_greedy=True)
    ref = head_ref(net, seen)
    err = (q.double() - ref).abs().max().item()
    print(f"head B={B} entry={entry}: max |q - ref| = {err:.3e}")
    assert err < TOL, err
    assert torch.equal(g.long(), q.argmax(1))
    assert torch.equal(fused.head(net, inp, want_q=False, want_greedy=True)[1], g)
    q_alone = fused.head(net, _rows(fused, inp, NARROW_ROWS))
    diff = (q_alone - q[:NARROW_ROWS]).abs().max().item()
    print(f"head B={B} entry={entry}: max |q(rows alone) - q(rows in the batch)| = {diff:.3e}")
    assert diff < PATHS, diff


# conv7 outputs (channel, pixel) — dense columns 8, 9, 287, 574 — that actor2 copies into Q: positions 0 .. 3 of k_gemm_finish's four
# columns per thread, a thread's four columns straddling two channels (8 | 9), and for every one of them col / 9 != col
PICKS = ((0, 8), (1, 0), (31, 8), (63, 7))
FC1_SCALE = 1.0 / 64.0


def _bias_ramp_net():
    """Every parameter zero but conv7.bias[c] = c + 1 and a chain of selections: fc1 row j takes conv7 output PICKS[j] times 1/64, fc2
    and actor1 pass their first rows on, actor2 copies them.  All selections are positive, where mish is increasing.  The 1/64
    keeps Q below 1: conv7's outputs reach mish(64) = 64 and are handed on with 22 bits (split f16), an error of 64 * 2^-22 = 1.5e-5
    that an identity chain would carry into Q — beyond 1e-5 without any fault; scaled it is 2.4e-7."""
    net = _net(10, 3)
    with torch.no_grad():
        for p in net.parameters():
            p.zero_()
        net.conv7.bias.copy_(torch.arange(1, 65, device="cuda").float())
        for j, (c, p) in enumerate(PICKS):
            net.fc1.weight[j, c * 9 + p] = FC1_SCALE
            net.fc2.weight[j, j] = 1.0
            net.actor1.weight[j, j] = 1.0
            net.actor2.weight[j, j] = 1.0
    return net


@pytest.mark.parametrize("B", [1281, 3329, 6785])                        # four slices, two, one
def test_head_bias_is_per_channel_on_the_wide_paths(fused, B):
    """A zero trunk output under the bias ramp: conv7's output is mish(c + 1) on all nine pixels of channel c, which bias[col]
    in place of bias[col / 9] would change (k_gemm_finish: bias[(col + r) / bias_div]); four of them read out through Q."""
    net = _bias_ramp_net()
    x = torch.zeros(B, 64, 12, 12, device="cuda")
    q = fused.head(net, x)
    ref = head_ref(net, x)
    m = torch.nn.functional.mish
    want = m(m(m(m(torch.tensor([c + 1.0 for c, _ in PICKS], dtype=torch.float64)) * FC1_SCALE)))     # mish(0) = 0 elsewhere
    assert (ref[0].cpu() - want).abs().max().item() < 1e-12 and len(set(want.tolist())) == 4
    err = (q.double() - ref).abs().max().item()
    print(f"bias ramp B={B}: max |q - ref| = {err:.3e}")
    assert err < TOL, (err, q[0].tolist(), want.tolist())
    assert torch.equal(q, q[:1].expand(B, 4))                             # every row had the same input


@pytest.mark.parametrize("B", [1281, 3329, 6785])
def test_head_rows_do_not_leak_into_their_neighbours(fused, B):
    """Only the last row (in the ragged last tile) has a non-zero trunk output: all other rows give the Q of a zero row bit for bit
    — a slice or a tile that wrote or summed into another row would show — and the last row its own, against float64."""
    torch.manual_seed(B + 1)
    net = _net(10, 3)
    x = torch.zeros(B, 64, 12, 12, device="cuda")
    x[B - 1] = torch.randn(64, 12, 12, device="cuda") * 1.5
    q = fused.head(net, x)
    assert torch.equal(q[:B - 1], q[:1].expand(B - 1, 4))
    assert not torch.equal(q[B - 1], q[0])
    ref = head_ref(net, x[B - 2:])                                        # a zero row and the last one
    assert (q[B - 2:].double() - ref).abs().max().item() < TOL


def _tie_cases(actor2):
    """(name, weight, bias, the columns of Q that tie, the greedy action) from a random actor2."""
    w, b = actor2.weight.detach().clone(), actor2.bias.detach().clone()
    low = -1000.0                                                        # |actor1's output| . |w| stays far below this
    w1 = w.clone(); w1[3] = w1[1]
    b1 = b.clone(); b1[3] = b1[1]; b1[0] = low; b1[2] = low
    w3 = w.clone(); w3[3] = w3[2]
    b3 = b.clone(); b3[3] = b3[2]; b3[0] = low; b3[1] = low
    return (("rows 1 and 3 equal, 0 and 2 below", w1, b1, (1, 3), 1),
            ("zero weight, equal biases", torch.zeros_like(w), torch.full_like(b, 0.25), (0, 1, 2, 3), 0),
            ("rows 2 and 3 equal and largest", w3, b3, (2, 3), 2))


@pytest.mark.parametrize("entry", ["f32", "px16"])
@pytest.mark.parametrize("W", [10, 24])
def test_greedy_takes_the_first_of_tied_maxima(fused, W, entry):
    """k_q_head promises the first maximum, like torch.argmax; random Q never ties, these do — bit for bit, checked."""
    torch.manual_seed(W)
    B, S = 257, W + 2
    net = _net(W, 3)
    x = torch.randn(B, 64, S, S, device="cuda") * 1.5
    inp = x if entry == "f32" else fused.PX16.from_f32(x)
    for name, w, b, tied, first in _tie_cases(net.actor2):
        with torch.no_grad():
            net.actor2.weight.copy_(w)
            net.actor2.bias.copy_(b)
        q, g = fused.head(net, inp, want_greedy=True)
        assert torch.isfinite(q).all()
        for a in tied[1:]:
            assert torch.equal(q[:, a], q[:, tied[0]]), name             # it really ties
        others = [a for a in range(4) if a not in tied]
        if others:
            assert (q[:, others].max(1).values < q[:, tied[0]]).all(), name
        assert torch.equal(g.long(), q.argmax(1)), name
        assert torch.equal(g.long(), torch.full((B,), first, device="cuda")), name
        assert torch.equal(fused.head(net, inp, want_q=False, want_greedy=True)[1], g), name


TAIL, GUARD = 4096, 0xA5


def _param_ptrs(net):
    return [t.data_ptr() for t in (net.conv7.weight, net.conv7.bias, net.fc1.weight, net.fc1.bias, net.fc2.weight, net.fc2.bias,
                                   net.actor1.weight, net.actor1.bias, net.actor2.weight, net.actor2.bias)]


@pytest.mark.parametrize("entry", ["f32", "px16"])
@pytest.mark.parametrize("S,B", [(12, 1), (12, 1281), (12, 3329), (26, 1), (26, 3), (26, 131)])
def test_head_stays_inside_its_buffers_and_reads_only_what_it_wrote(fused, S, B, entry):
    """The C ABI called directly with a workspace of tron_dqn_head_workspace bytes, Q of 16 B bytes and greedy of B bytes, each
    followed by 4096 bytes of 0xA5 that must survive; once with the workspace zeroed and once full of 0xFF (f16 and f32 NaN
    patterns): the same bits and a finite Q, so nothing read from the workspace was left over from before the call — the row
    clamps of the ragged tiles, the implicit conv7 GEMM's padding taps at 26x26 and the partial sums of the slices included."""
    nat = fused.nat
    L = nat.lib()
    torch.manual_seed(S * B)
    net = _net(S - 2, 3)
    x = torch.randn(B, 64, S, S, device="cuda") * 1.5
    if entry == "f32":
        fn, src = L.tron_dqn_head_fwd, x
    else:
        fn, src = L.tron_dqn_head_fwd_px16, fused.PX16.from_f32(x).buf
    need = int(L.tron_dqn_head_workspace(B, S))
    assert need > 0
    outs = []
    for fill in (0x00, 0xFF):
        ws = torch.full((need + TAIL,), fill, dtype=torch.uint8, device="cuda")
        ws[need:] = GUARD
        qb = torch.full((16 * B + TAIL,), GUARD, dtype=torch.uint8, device="cuda")
        gb = torch.full((B + TAIL,), GUARD, dtype=torch.uint8, device="cuda")
        assert ws.data_ptr() % 256 == 0 and qb.data_ptr() % 16 == 0
        nat.check(fn(src.data_ptr(), B, S, *_param_ptrs(net), ws.data_ptr(), qb.data_ptr(), gb.data_ptr(), nat.stream_ptr()), "head")
        torch.cuda.synchronize()
        for name, buf, used in (("workspace", ws, need), ("q_out", qb, 16 * B), ("greedy_out", gb, B)):
            assert bool((buf[used:] == GUARD).all()), f"S={S} B={B} {entry}: wrote past the end of {name}"
        outs.append((qb[:16 * B].clone(), gb[:B].clone()))
    (q0, g0), (q1, g1) = outs
    assert torch.equal(q0, q1) and torch.equal(g0, g1), "the result depends on what the workspace held before the call"
    q = q0.view(torch.float32).reshape(B, 4)
    assert torch.isfinite(q).all()
    assert torch.equal(g0.view(torch.int8).long(), q.argmax(1))


def test_head_refuses_bad_arguments_before_any_launch(fused):
    """Misaligned workspace or Q, a batch beyond the side's limit, the pooled entry at 26x26, a negative batch: the status the header
    names, and Q and greedy keep their fill (head_fwd decides all of these ahead of its first launch)."""
    nat = fused.nat
    L = nat.lib()
    net12, net26 = _net(10, 3), _net(24, 3)
    p12, p26 = _param_ptrs(net12), _param_ptrs(net26)
    x = torch.zeros(4, 64, 26, 26, device="cuda")                        # enough for 4 rows of either side, f32 or PX16
    ws = torch.zeros(max(int(L.tron_dqn_head_workspace(4, S)) for S in (12, 26)) + 16, dtype=torch.uint8, device="cuda")
    qo = torch.full((4 * 4 + 4,), 7.0, device="cuda")
    go = torch.full((4,), 9, dtype=torch.int8, device="cuda")
    xp, wp, qp, gp = x.data_ptr(), ws.data_ptr(), qo.data_ptr(), go.data_ptr()
    entries = (L.tron_dqn_head_fwd, L.tron_dqn_head_fwd_px16)
    for fn in entries + (L.tron_dqn_head_fwd_pooled,):
        assert fn(xp, 4, 12, *p12, wp + 8, qp, gp, None) == nat.ERR_BAD_ARG
        assert fn(xp, 4, 12, *p12, wp, qp + 4, gp, None) == nat.ERR_BAD_ARG
        assert fn(xp, (1 << 24) + 1, 12, *p12, wp, qp, gp, None) == nat.ERR_UNSUPPORTED
        assert fn(xp, -1, 12, *p12, wp, qp, gp, None) == nat.ERR_BAD_ARG
    for fn in entries:
        assert fn(xp, 4, 26, *p26, wp + 8, qp, gp, None) == nat.ERR_BAD_ARG
        assert fn(xp, 4, 26, *p26, wp, qp + 4, gp, None) == nat.ERR_BAD_ARG
        assert fn(xp, (1 << 22) + 1, 26, *p26, wp, qp, gp, None) == nat.ERR_UNSUPPORTED
        assert fn(xp, -1, 26, *p26, wp, qp, gp, None) == nat.ERR_BAD_ARG
    assert L.tron_dqn_head_fwd_pooled(xp, 4, 26, *p26, wp, qp, gp, None) == nat.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((qo == 7.0).all()) and bool((go == 9).all())
