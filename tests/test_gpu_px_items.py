"""The learner's persistent PX16 kernels (csrc/tron_conv_ws_train.hip, csrc/tron_conv_ws_kernel.hpp) at the smallest batches
at which every workgroup walks several work items — a second item in the other LDS buffer, a third in the first buffer again, a
ragged last round, sums and maxima carried from item to item — each kernel through the C ABI against float64 of the same
expression, with the bounds of its one-item tests in tests/test_gpu_trunk_px.py.  The batches come from the host model of the
launchers (tests/px_items_support.py) for the device the test runs on; every test first asserts that its batch loops."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional

from activation_range_support import to_px as _to_px
import test_gpu_trunk_px as trunk_px                                 # for its _grad_px (test_gpu_activation_range's copy also returns the packed values)
import px_items_support as P

_grad_px = trunk_px._grad_px


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fused():
    from Net import fused
    return fused


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count   # what device_cus() reads


def _steady(plan_fn, S, cin, cout, cus):
    B = P.steady_batch(plan_fn, S, cin, cout, cus)
    plan = plan_fn(S, cin, cout, B, cus)
    cond = plan.conditions()
    assert len(cond) == 4 and all(cond.values()), cond
    return B, plan


# ---- the weight gradient ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,cin,cout", P.SHAPES)
def test_weight_gradient_workspace_is_the_model_s(fused, cus, S, cin, cout):
    """The model of launch_wgrad_px is the code's: the workspace query answers the plan's bytes + 256 exactly."""
    nat = fused.nat                                                  # the library binding Net/ calls through
    B, _ = _steady(P.wgrad_px_plan, S, cin, cout, cus)
    for b in (1, B, 4096):
        assert int(nat.lib().tron_conv3x3_wgrad_px16_workspace(b, cin, cout, S)) == P.wgrad_px_plan(S, cin, cout, b, cus).bytes + 256


@pytest.mark.parametrize("S,cin,cout", P.SHAPES)
def test_weight_gradient_over_several_items(fused, cus, S, cin, cout):
    """tron_conv3x3_wgrad_px16 with two or three stacks per workgroup (an odd batch at 12x12: the last stack holds one image and
    is no workgroup's first item) against the float64 weight gradient, 3e-6 x max |dW| as at one item; same bits twice."""
    B, plan = _steady(P.wgrad_px_plan, S, cin, cout, cus)
    torch.manual_seed(cin + cout + S)
    x = torch.randn(B, cin, S, S, device="cuda") * 1.5
    g = torch.randn(B, cout, S, S, device="cuda")
    gw = fused.conv3x3_wgrad_px(_to_px(fused, x), _grad_px(fused, g))
    wd = torch.zeros(cout, cin, 3, 3, device="cuda", dtype=torch.float64, requires_grad=True)
    (F.conv2d(x.double(), wd, padding=1) * g.double()).sum().backward()
    scale = wd.grad.abs().max().item()
    err = (gw.double() - wd.grad).abs().max().item()
    print(f"wgrad {S}x{S} {cin}->{cout}: B {B}, workgroups per band {plan.nwg}, items (most, fewest) per band "
          f"{[plan.items(b) for b in range(plan.NB)]}, error {err / (3e-6 * scale):.3g} of the bound")
    assert err < 3e-6 * scale
    assert torch.equal(gw, fused.conv3x3_wgrad_px(_to_px(fused, x), _grad_px(fused, g)))


@pytest.mark.parametrize("S,cin,cout", P.SHAPES)
def test_weight_gradient_one_hot_in_every_item_position(fused, cus, S, cin, cout):
    """One unit gradient pixel against one input pixel of value 2, in an image whose stack is its workgroup's first, second, third
    item, the last stack of the ragged round, (12x12) the last stack's only image and the row under the stack separator; pixels at
    band edges and image corners.  Exactly one tap is 2.0, everything else 0 — with (a) every other image's input 7.0 and gradient
    zero (a stale or late activation buffer shows), (b) every other image's gradient 1.0 and input zero (a stale gradient buffer)."""
    B, plan = _steady(P.wgrad_px_plan, S, cin, cout, cus)
    for n, c in enumerate(P.wgrad_one_hot_cases(plan)):
        co, ci = (7 * n + 5) % cout, (11 * n + 3) % cin
        iy, ix = c.y + c.ky - 1, c.x + c.kx - 1
        want = torch.zeros(cout, cin, 3, 3, device="cuda")
        want[co, ci, c.ky, c.kx] = 2.0
        for fill in "ab":
            x1 = torch.full((B, cin, S, S), 7.0 if fill == "a" else 0.0, device="cuda")
            g1 = torch.full((B, cout, S, S), 0.0 if fill == "a" else 1.0, device="cuda")
            x1[c.image] = 0.0
            g1[c.image] = 0.0
            x1[c.image, ci, iy, ix] = 2.0
            g1[c.image, co, c.y, c.x] = 1.0
            got = fused.conv3x3_wgrad_px(_to_px(fused, x1), _grad_px(fused, g1))
            assert torch.equal(got, want), (c, fill, got.nonzero().tolist()[:8], got.abs().max().item())


# ---- the backward convolution -----------------------------------------------------------------------------------------------

DG = [(32, 32, False), (32, 32, True), (32, 64, False), (64, 64, False), (64, 64, True)]


@pytest.mark.parametrize("S", P.SIDES)
@pytest.mark.parametrize("cin,cout,extra", DG)
def test_input_gradient_over_several_items(fused, cus, S, cin, cout, extra):
    """tron_conv3x3_ws_dgrad with two or three items per workgroup, the gradient at a mean-reduced loss's 1e-6: output, f32 copy,
    bias sums and maxima against float64 with the bounds of test_input_gradient_with_fused_activation_backward, then with
      * the batch's largest |output| planted (one image's gradient x 8) in an image that is its workgroups' LAST item, and again in
        one that is a FIRST item: info reports it both times (the maximum is carried across items, not overwritten);
      * the gradient zero but in the images of one workgroup's second and third items: the bias sums are those images' float64
        sums (later items are accumulated, not dropped).
    The expression is linear in (gradient, extra) image by image, so one float64 reference serves every case.
    info[4 + c] bounds channel c up to what the output itself may be off by (4e-6 x scale: it is the maximum of what was written)."""
    B, plan = _steady(P.ws_bwd_plan, S, cin, cout, cus)
    imgs = P.ws_planted_images(plan)
    torch.manual_seed(cin * 3 + cout + S)
    mag = 1e-6
    W = torch.randn(cout, cin, 3, 3, device="cuda") * 0.08
    g = torch.randn(B, cout, S, S, device="cuda") * mag
    zb = torch.randn(B, cin, S, S, device="cuda") * 2.0
    ex = torch.randn(B, cin, S, S, device="cuda") * mag * 3.0 if extra else None
    rot, wn = fused._split_jobs([W], "tron_conv3x3_ws_split_weights_bwd", True)
    zpx = _to_px(fused, zb)
    xd = torch.zeros(B, cin, S, S, device="cuda", dtype=torch.float64, requires_grad=True)
    (F.conv2d(xd, W.double(), padding=1) * g.double()).sum().backward()
    zz = zb.double().requires_grad_(True)
    F.mish(zz).backward(xd.grad + (0 if ex is None else ex.double()))
    base = zz.grad
    del xd, zz
    name = f"dgrad {S}x{S} {cin}->{cout}{' + extra' if extra else ''}"
    print(f"{name}: B {B}, grid {plan.grid}, items {plan.nitems}, (most, fewest) per workgroup {plan.items()}, planted {imgs}")

    def run(f, case, want_f32=False):
        fv = f.view(-1, 1, 1, 1)
        gp = _grad_px(fused, g * fv)
        ep = None if ex is None else _grad_px(fused, ex * fv)
        out, o32, gb = fused.conv_ws_dgrad(gp, cin, rot[0], wn[0:1], zpx, extra=ep, want_f32=want_f32)
        ref = base * fv.double()
        scale = ref.abs().max().item()
        e_px = (out.float().double() - ref).abs().max().item()
        e_32 = (o32.double() - ref).abs().max().item() if want_f32 else 0.0
        sums = ref.sum((0, 2, 3))
        e_s, b_s = (gb.double() - sums).abs().max().item(), 2e-5 * sums.abs().max().item() + 2e-6 * scale
        info = out.info.cpu().numpy()
        top = info[4:4 + cin].max()
        amax = ref.abs().amax((0, 2, 3)).cpu().numpy()
        print(f"{name}, {case}: output {e_px / (4e-6 * scale):.3g}, f32 {e_32 / (4e-6 * scale):.3g}, sums {e_s / b_s:.3g}, "
              f"top {abs(top - scale) / (1e-5 * scale):.3g} of their bounds")
        assert e_px < 4e-6 * scale and e_32 < 4e-6 * scale
        assert e_s < b_s
        assert abs(top - scale) < 1e-5 * scale and 2.0 ** 5 <= top * info[0] < 2.0 ** 15
        assert (info[4:4 + cin] >= amax - 4e-6 * scale).all()
        return out, gb, ref, scale

    ones = torch.ones(B, device="cuda")
    out, gb, _, _ = run(ones, "whole batch", want_f32=True)
    out2, _, gb2 = fused.conv_ws_dgrad(_grad_px(fused, g), cin, rot[0], wn[0:1], zpx, extra=None if ex is None else _grad_px(fused, ex))
    assert torch.equal(out.buf, out2.buf) and torch.equal(gb, gb2)
    for where in ("last", "first"):
        f = ones.clone()
        f[imgs[where]] = 8.0
        _, _, ref, scale = run(f, f"maximum in a {where} item (image {imgs[where]})")
        assert ref[imgs[where]].abs().max().item() == scale          # the planted image holds the batch's maximum
        rest = torch.cat([ref[:imgs[where]], ref[imgs[where] + 1:]]).abs().max().item()
        assert rest < 0.5 * scale                                    # ... and nothing else comes near: info's top can only be its
    f = torch.zeros(B, device="cuda")
    f[imgs["sums"]] = 1.0
    _, gb, ref, _ = run(f, f"only the second and third items of one workgroup (images {imgs['sums']})")
    assert gb.abs().max().item() > 0.0 and ref[f == 0].abs().max().item() == 0.0 and ref[f != 0].abs().max().item() > 0.0


# ---- the training forward ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,cin,cout,res", [(12, 64, 64, True), (26, 32, 64, False), (34, 64, 64, True)])
def test_training_forward_over_several_items(fused, cus, S, cin, cout, res):
    """tron_conv3x3_ws_train_fwd with two or three items per workgroup: the pre-activation image and the output against float64, 1e-5."""
    B, plan = _steady(P.ws_fwd_plan, S, cin, cout, cus)
    torch.manual_seed(cin + cout + S)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1).cuda()
    x = torch.randn(B, cin, S, S, device="cuda") * 1.5
    r = torch.randn(B, cout, S, S, device="cuda") if res else None
    frag = fused._split_jobs([conv.weight], "tron_conv3x3_ws_split_weights", False)[0]
    xp, rp = _to_px(fused, x), (None if r is None else _to_px(fused, r))
    a, z = fused.conv_ws_train(xp, cout, frag, conv.bias, residual=rp)
    a32, z2 = fused.conv_ws_train(xp, cout, frag, conv.bias, residual=rp, want_f32=True)
    zref = F.conv2d(x.double(), conv.weight.double(), conv.bias.double(), padding=1) + (0 if r is None else r.double())
    aref = F.mish(zref)
    ez, ea, e32 = ((t.float().double() - ref).abs().max().item() for t, ref in ((z, zref), (a, aref), (a32, aref)))
    print(f"train fwd {S}x{S} {cin}->{cout}: B {B}, grid {plan.grid}, items {plan.nitems}, (most, fewest) per workgroup {plan.items()}, "
          f"pre-activation {ez / 1e-5:.3g}, output {ea / 1e-5:.3g}, f32 output {e32 / 1e-5:.3g} of the bound")
    assert ez < 1e-5 and ea < 1e-5 and e32 < 1e-5
    assert torch.equal(z.buf, z2.buf)


# ---- the gradient chain's entry ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [32, 64])
def test_gradient_image_entry_second_pass(fused, C):
    """tron_px16_grad_from_f32 at 1 024 + 5 images of 12x12: five workgroups walk a second image, k_wsb_finish adds its largest
    group count.  Against float64 g mish'(z) with test_gradient_image_entry's bounds, then with the gradient zero but in the second
    pass's images: the bias sums are theirs."""
    nat = fused.nat                                                  # the library binding Net/ calls through
    S, B = 12, P.GOUT_GROUPS + 5
    assert int(nat.lib().tron_px16_grad_workspace(B, C)) == 2 * P.GOUT_GROUPS * C * 4 + 256 and B > P.GOUT_GROUPS
    torch.manual_seed(S + C)
    z = torch.randn(B, C, S, S, device="cuda") * 3.0
    z[0, 0, 0, :4] = torch.tensor([25.0, -30.0, 0.0, 60.0], device="cuda")
    g = torch.randn(B, C, S, S, device="cuda")
    zpx = _to_px(fused, z)
    zd = z.double().requires_grad_(True)
    F.mish(zd).backward(torch.ones_like(zd))
    dm = zd.grad                                                     # mish'(z): the reference of any g is g * dm
    late = torch.zeros(B, device="cuda")
    late[P.GOUT_GROUPS:] = 1.0
    for case, f in (("whole batch", torch.ones(B, device="cuda")), ("second pass only", late)):
        gi = g * f.view(-1, 1, 1, 1)
        gp, gb = fused.grad_px_from_f32(gi, zpx)
        ref = gi.double() * dm
        scale = ref.abs().max().item()
        sums = ref.sum((0, 2, 3))
        e_px, e_s, b_s = (gp.float().double() - ref).abs().max().item(), (gb.double() - sums).abs().max().item(), 1e-5 * sums.abs().max().item() + 1e-6 * scale
        info = gp.info.cpu().numpy()
        top = info[4:4 + C].max()
        print(f"grad entry C {C}, {case}: image {e_px / (2e-6 * scale):.3g}, sums {e_s / b_s:.3g}, top {abs(top - scale) / (2e-6 * scale):.3g} of their bounds")
        assert e_px < 2e-6 * scale
        assert e_s < b_s
        assert info[0] * info[1] == 1.0 and abs(top - scale) <= 2e-6 * scale
        assert (info[4:4 + C] >= ref.abs().amax((0, 2, 3)).cpu().numpy() * (1 - 1e-5)).all()
        assert 2.0 ** 12 <= top * info[0] < 2.0 ** 15
    assert torch.equal(ref[:P.GOUT_GROUPS], torch.zeros_like(ref[:P.GOUT_GROUPS])) and gb.abs().max().item() > 0.0
