"""The native launches of every hand-written autograd node of Net/activations.py, by name and in order.

Every native call of Net/activations.py, Net/fused.py and Net/kfac.py goes through `tron._native.check(rc, name)`.  Each test
below replaces it with a recorder that still checks `rc`, runs one forward + backward of one node at the smallest shape that
takes the branch, and compares the recorded names with a list written out here.  The lists were recorded with this file on the
commit before the nodes' shared walkers and helpers were introduced (the hand-written, layer-by-layer nodes), so they pin what
that refactor had to keep — and the next edit that adds, drops or reorders a launch shows up as a diff of names, not as a
benchmark regression.  A case returns its outputs and gradients as well: the tests ignore them, a script that compares two trees
bit for bit can use them."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _codes(B, S, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    vals = torch.tensor([1, 1, 1, -1, -2, -3, 10, -10], dtype=torch.int8, device="cuda")
    return vals[torch.randint(0, 8, (B, S, S), device="cuda", generator=g)].contiguous()


def _nodes(t):
    """The names of the autograd nodes behind t."""
    seen, stack = set(), [t.grad_fn]
    while stack:
        f = stack.pop()
        if f is not None and f not in seen:
            seen.add(f)
            stack += [n for n, _ in f.next_functions]
    return {f.name() for f in seen}


def _backward(y, node):
    """One backward of a fixed random functional of y; `node` must be in the graph."""
    assert node + "Backward" in _nodes(y), (node, sorted(_nodes(y)))
    (y * torch.randn(y.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))).sum().backward()


def _params(net, out):
    out.update({"grad." + n: p.grad for n, p in net.named_parameters() if p.grad is not None})
    return out


# ---- the DQN net's nodes, through the net's own dispatch (Net/DQNNet.py) -------------------------------------------------
def _dqn(mp, node, width=10, B=3, planes=3, plane4=0.0, codes=True, input_grad=False, pool_fused=True, trunk_px=True, body_px=True):
    from Net import DQNNet, fused
    torch.manual_seed(width + planes)
    net = DQNNet.Net(planes, width).cuda()
    if not pool_fused:
        mp.setattr(fused, "use_pool_fused_train", False)
    if not trunk_px:
        mp.setattr(fused, "use_trunk_px", False)
    if not body_px:
        mp.setenv("TRON_BODY_PX", "0")
    S = width + 2
    if codes:
        x = _codes(B, S, 3)
        y = net.forward_codes(x, plane4)
    else:
        x = torch.randn(B, planes, S, S, device="cuda").requires_grad_(input_grad)
        y = net(x)
    _backward(y, node)
    out = _params(net, {"y": y.detach()})
    if input_grad:
        out["grad.x"] = x.grad
    return out


def body_px_12_pool_fused(mp, **kw):
    return _dqn(mp, "_BodyPX", planes=4, plane4=0.5, **kw)


def body_px_12_pool_apart(mp, **kw):
    return _dqn(mp, "_BodyPX", pool_fused=False, **kw)


def body_px_26(mp, **kw):
    return _dqn(mp, "_BodyPX", **{"width": 24, **kw})


def trunk_px_12(mp, **kw):
    return _dqn(mp, "_TrunkPX", body_px=False, **kw)


def trunk_hip_planes_12(mp, **kw):
    return _dqn(mp, "_TrunkHIP", codes=False, **kw)


def trunk_hip_codes_4_planes(mp, **kw):
    return _dqn(mp, "_TrunkHIP", planes=4, plane4=0.5, trunk_px=False, **kw)


def trunk_hip_planes_input_grad(mp, **kw):
    return _dqn(mp, "_TrunkHIP", codes=False, input_grad=True, **kw)


def trunk_hip_planes_26(mp, **kw):
    return _dqn(mp, "_TrunkHIP", codes=False, **{"width": 24, "B": 2, **kw})


# ---- the actor-critic trunk, through ACNet.Mulnet ------------------------------------------------------------------------
def _ac(mp, mode, width=10, B=3):
    from Net import ACNet, activations, kfac
    torch.manual_seed(width)
    net = ACNet.Mulnet(width).cuda()
    net.dropout.p = 0.0
    S = width + 2
    x = torch.randn(B, 3, S, S, device="cuda")
    extra = torch.rand(B, 2, device="cuda")
    acts = torch.randint(0, 4, (B, 1), device="cuda")
    if mode == "infer":                                     # the rollouts' acting: `ac_trunk_infer`
        with torch.no_grad():
            return {"trunk": net._trunk_px(x)}
    opt = None
    if mode == "kfac":
        opt = kfac.KFACOptimizer(net)
        opt.acc_stats = True
    scope = activations.GradScope()
    with activations.grad_scope(scope):
        v, logp, ent = net.evaluate_actions(x, acts, extra)
    assert "_ACTrunkPXBackward" in _nodes(v)
    scope.skip_weight_gradients = mode == "skip"
    (v.pow(2).mean() - logp.mean() - 0.01 * ent).backward()
    out = _params(net, {"v": v.detach(), "logp": logp.detach()})
    if opt is not None:
        for i, m in enumerate(opt.modules):
            out[f"m_aa.{i}"], out[f"m_gg.{i}"] = opt.m_aa[m], opt.m_gg[m]
    return out


def ac_trunk_plain(mp, **kw):
    return _ac(mp, "plain", **kw)


def ac_trunk_kfac_stats(mp, **kw):
    return _ac(mp, "kfac", **kw)


def ac_trunk_skip_weight_gradients(mp, **kw):
    return _ac(mp, "skip", **kw)


def ac_trunk_infer(mp, **kw):
    return _ac(mp, "infer", **kw)


# ---- the single-layer nodes, called directly -----------------------------------------------------------------------------
def _pool_conv7(node, S, B, input_grad):
    from Net import activations
    torch.manual_seed(S)
    pool = torch.nn.AvgPool2d(kernel_size=3, padding=1, stride=2)
    conv = torch.nn.Conv2d(64, 64, 7, padding=3, stride=2).cuda()
    x = torch.randn(B, 64, S, S, device="cuda").requires_grad_(input_grad)
    if S == 12:
        assert activations.pool_conv7_supported(pool, conv, x)
        y = activations.pool_conv7_mish(pool, conv, x)
    else:
        assert activations.pool_conv7_cl_supported(pool, conv, x)
        y = activations.pool_conv7_cl_mish(pool, conv, x)
    _backward(y, node)
    return _params(conv, {"y": y.detach(), **({"grad.x": x.grad} if input_grad else {})})


def pool_conv7_input_grad(mp):
    return _pool_conv7("_PoolConv7", 12, 3, True)


def pool_conv7_no_input_grad(mp):
    return _pool_conv7("_PoolConv7", 12, 3, False)


def pool_conv7_cl_26(mp):
    return _pool_conv7("_PoolConv7CL", 26, 2, True)


def conv3x3_hip_12(mp):
    from Net import activations
    torch.manual_seed(1)
    conv = activations.Conv3x3(32, 64, 3, padding=1).cuda()
    x = torch.randn(3, 32, 12, 12, device="cuda", requires_grad=True)
    y = conv(x)
    _backward(y, "_Conv3x3HIP")
    return _params(conv, {"y": y.detach(), "grad.x": x.grad})


def conv_bias_mish_residual(mp):
    from Net import activations
    torch.manual_seed(2)
    conv = torch.nn.Conv2d(32, 32, 3, padding=1).cuda()
    x = torch.randn(3, 32, 12, 12, device="cuda", requires_grad=True)
    r = torch.randn(3, 32, 12, 12, device="cuda", requires_grad=True)
    y = activations.conv_bias_mish(conv, x, r)
    _backward(y, "_ConvBiasMishHIP")
    return _params(conv, {"y": y.detach(), "grad.x": x.grad, "grad.r": r.grad})


def conv1_codes(mp):
    from Net import activations
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(4, 32, 3, padding=1).cuda()
    y = activations.conv1_codes_mish(conv, _codes(3, 12, 4), 0.5)
    _backward(y, "_Conv1CodesHIP")
    return _params(conv, {"y": y.detach()})


def _linear(bias):
    from Net import activations
    torch.manual_seed(4)
    layer = torch.nn.Linear(64, 32, bias=bias).cuda()
    x = torch.randn(256, 64, device="cuda", requires_grad=True)
    y = activations.linear(layer, x)
    _backward(y, "_LinearHIP")
    return _params(layer, {"y": y.detach(), "grad.x": x.grad})


def linear_hip_bias(mp):
    return _linear(True)


def linear_hip_no_bias(mp):
    return _linear(False)


def _tail(training):
    from Net import DQNNet, activations
    torch.manual_seed(6)
    net = DQNNet.Net(3, 10).cuda().train(training)
    x = torch.randn(256, net.flat, device="cuda", requires_grad=True)
    assert net.dropout.p == 0.2 and activations.tail_mlp_supported(net, x)
    y = activations.tail_mlp(net, x)
    _backward(y, "_TailMLP")
    return _params(net, {"y": y.detach(), "grad.x": x.grad})


def tail_mlp_training(mp):
    return _tail(True)


def tail_mlp_eval(mp):
    return _tail(False)


EXPECTED = {
    "body_px_12_pool_fused": [
        "tron_conv3x3_ws_split_weights", "tron_conv1_px16_train", "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd",
        "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd_pool12", "tron_conv7_dense",
        "tron_gemm_f16x3", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_bwd", "tron_mish_bwd",
        "tron_mish_bwd", "tron_mish_bwd", "tron_absmax_pow2", "tron_gemm_f16x3", "tron_gemm_f16x3", "tron_conv7_dense",
        "tron_absmax_pow2", "tron_px16_grad_from_pooled", "tron_conv3x3_ws_split_weights_bwd", "tron_conv3x3_wgrad_px16",
        "tron_conv3x3_ws_dgrad", "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_conv3x3_wgrad_px16",
        "tron_conv3x3_ws_dgrad", "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_conv3x3_wgrad_px16",
        "tron_conv3x3_ws_dgrad", "tron_conv1_wgrad_px16"],
    "body_px_12_pool_apart": [
        "tron_conv3x3_ws_split_weights", "tron_conv1_px16_train", "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd",
        "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd", "tron_pool12_px16",
        "tron_conv7_dense", "tron_gemm_f16x3", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_bwd",
        "tron_mish_bwd", "tron_mish_bwd", "tron_mish_bwd", "tron_absmax_pow2", "tron_gemm_f16x3", "tron_gemm_f16x3",
        "tron_conv7_dense", "tron_absmax_pow2", "tron_px16_grad_from_pooled", "tron_conv3x3_ws_split_weights_bwd",
        "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad",
        "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad",
        "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_conv1_wgrad_px16"],
    "body_px_26": [
        "tron_conv3x3_ws_split_weights", "tron_conv1_px16_train", "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd",
        "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd", "tron_pool_conv7_fwd_px16",
        "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_bwd", "tron_mish_bwd", "tron_mish_bwd",
        "tron_pool_conv7_bwd_pooled", "tron_absmax_pow2", "tron_px16_grad_from_pooled", "tron_conv3x3_ws_split_weights_bwd",
        "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad",
        "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad",
        "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_conv1_wgrad_px16"],
    "trunk_px_12": [
        "tron_conv3x3_ws_split_weights", "tron_conv1_px16_train", "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd",
        "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd", "tron_pool12", "tron_conv7_dense",
        "tron_gemm_f16x3", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_bwd", "tron_mish_bwd",
        "tron_mish_bwd", "tron_mish_bwd", "tron_absmax_pow2", "tron_gemm_f16x3", "tron_pool12", "tron_gemm_f16x3",
        "tron_conv7_dense", "tron_absmax_pow2", "tron_px16_grad_from_f32", "tron_conv3x3_ws_split_weights_bwd",
        "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad",
        "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad",
        "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_conv1_wgrad_px16"],
    "trunk_hip_planes_12": [
        "tron_conv3x3_split_weights", "tron_conv3x3_fwd", "tron_conv3x3_fwd", "tron_conv3x3_fwd", "tron_conv3x3_fwd",
        "tron_conv3x3_fwd", "tron_conv3x3_fwd", "tron_pool12", "tron_conv7_dense", "tron_gemm_f16x3", "tron_mish_fwd",
        "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_bwd", "tron_mish_bwd", "tron_mish_bwd", "tron_mish_bwd",
        "tron_absmax_pow2", "tron_gemm_f16x3", "tron_pool12", "tron_gemm_f16x3", "tron_conv7_dense", "tron_bias_mish_bwd",
        "tron_conv3x3_wgrad", "tron_conv3x3_dgrad_mish", "tron_conv3x3_wgrad", "tron_conv3x3_dgrad_mish", "tron_conv3x3_wgrad",
        "tron_conv3x3_dgrad_mish", "tron_conv3x3_wgrad", "tron_conv3x3_dgrad_mish", "tron_conv3x3_wgrad", "tron_conv3x3_dgrad_mish",
        "tron_conv3x3_wgrad"],
    "trunk_hip_codes_4_planes": [
        "tron_conv3x3_split_weights", "tron_conv3x3_fwd", "tron_conv3x3_fwd", "tron_conv3x3_fwd", "tron_conv3x3_fwd",
        "tron_conv3x3_fwd", "tron_conv3x3_fwd", "tron_pool12", "tron_conv7_dense", "tron_gemm_f16x3", "tron_mish_fwd",
        "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_bwd", "tron_mish_bwd", "tron_mish_bwd", "tron_mish_bwd",
        "tron_absmax_pow2", "tron_gemm_f16x3", "tron_pool12", "tron_gemm_f16x3", "tron_conv7_dense", "tron_bias_mish_bwd",
        "tron_conv3x3_wgrad", "tron_conv3x3_dgrad_mish", "tron_conv3x3_wgrad", "tron_conv3x3_dgrad_mish", "tron_conv3x3_wgrad",
        "tron_conv3x3_dgrad_mish", "tron_conv3x3_wgrad", "tron_conv3x3_dgrad_mish", "tron_conv3x3_wgrad", "tron_conv3x3_dgrad_mish",
        "tron_pop_up", "tron_conv3x3_wgrad"],
    "trunk_hip_planes_input_grad": [
        "tron_conv3x3_split_weights", "tron_conv3x3_fwd", "tron_conv3x3_fwd", "tron_conv3x3_fwd", "tron_conv3x3_fwd",
        "tron_conv3x3_fwd", "tron_conv3x3_fwd", "tron_pool12", "tron_conv7_dense", "tron_gemm_f16x3", "tron_mish_fwd",
        "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_bwd", "tron_mish_bwd", "tron_mish_bwd", "tron_mish_bwd",
        "tron_absmax_pow2", "tron_gemm_f16x3", "tron_pool12", "tron_gemm_f16x3", "tron_conv7_dense", "tron_bias_mish_bwd",
        "tron_conv3x3_wgrad", "tron_conv3x3_dgrad_mish", "tron_conv3x3_wgrad", "tron_conv3x3_dgrad_mish", "tron_conv3x3_wgrad",
        "tron_conv3x3_dgrad_mish", "tron_conv3x3_wgrad", "tron_conv3x3_dgrad_mish", "tron_conv3x3_wgrad", "tron_conv3x3_dgrad_mish",
        "tron_conv3x3_wgrad"],
    "trunk_hip_planes_26": [
        "tron_conv3x3_split_weights", "tron_conv3x3_fwd", "tron_conv3x3_fwd", "tron_conv3x3_fwd", "tron_conv3x3_fwd",
        "tron_conv3x3_fwd", "tron_conv3x3_fwd", "tron_pool_conv7_fwd", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd",
        "tron_mish_bwd", "tron_mish_bwd", "tron_mish_bwd", "tron_pool_conv7_bwd", "tron_bias_mish_bwd", "tron_conv3x3_wgrad",
        "tron_conv3x3_dgrad_mish", "tron_conv3x3_wgrad", "tron_conv3x3_dgrad_mish", "tron_conv3x3_wgrad", "tron_conv3x3_dgrad_mish",
        "tron_conv3x3_wgrad", "tron_conv3x3_dgrad_mish", "tron_conv3x3_wgrad", "tron_conv3x3_dgrad_mish", "tron_conv3x3_wgrad"],
    "ac_trunk_plain": [
        "tron_conv3x3_fwd", "tron_px16_from_f32", "tron_px16_from_f32", "tron_conv3x3_ws_split_weights",
        "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd",
        "tron_conv3x3_ws_train_fwd", "tron_pool_s2", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd",
        "tron_mish_fwd", "tron_mish_fwd", "tron_mish_bwd", "tron_mish_bwd", "tron_mish_bwd", "tron_mish_bwd", "tron_mish_bwd",
        "tron_mish_bwd", "tron_pool_s2_bwd", "tron_absmax_pow2", "tron_px16_grad_from_f32", "tron_conv3x3_ws_split_weights_bwd",
        "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad",
        "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad",
        "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_conv3x3_wgrad"],
    "ac_trunk_kfac_stats": [
        "tron_conv3x3_fwd", "tron_px16_from_f32", "tron_px16_from_f32", "tron_conv3x3_ws_split_weights",
        "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd",
        "tron_conv3x3_ws_train_fwd", "tron_kfac_patch_gram", "tron_kfac_gram_px16", "tron_kfac_gram_px16", "tron_kfac_gram_px16",
        "tron_kfac_gram_px16", "tron_kfac_gram_px16", "tron_pool_s2", "tron_kfac_patch_gram", "tron_mish_fwd", "tron_mish_fwd",
        "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd", "tron_absmax_pow2", "tron_absmax_pow2", "tron_mish_bwd",
        "tron_absmax_pow2", "tron_absmax_pow2", "tron_mish_bwd", "tron_absmax_pow2", "tron_absmax_pow2", "tron_absmax_pow2",
        "tron_absmax_pow2", "tron_mish_bwd", "tron_absmax_pow2", "tron_absmax_pow2", "tron_mish_bwd", "tron_absmax_pow2",
        "tron_absmax_pow2", "tron_absmax_pow2", "tron_absmax_pow2", "tron_mish_bwd", "tron_absmax_pow2", "tron_absmax_pow2",
        "tron_mish_bwd", "tron_absmax_pow2", "tron_absmax_pow2", "tron_kfac_patch_gram", "tron_pool_s2_bwd", "tron_absmax_pow2",
        "tron_px16_grad_from_f32", "tron_px16_to_f32", "tron_absmax_pow2", "tron_kfac_patch_gram", "tron_absmax_pow2",
        "tron_conv3x3_ws_split_weights_bwd", "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_absmax_pow2",
        "tron_kfac_patch_gram", "tron_absmax_pow2", "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_absmax_pow2",
        "tron_kfac_patch_gram", "tron_absmax_pow2", "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_absmax_pow2",
        "tron_kfac_patch_gram", "tron_absmax_pow2", "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_absmax_pow2",
        "tron_kfac_patch_gram", "tron_absmax_pow2", "tron_conv3x3_wgrad_px16", "tron_conv3x3_ws_dgrad", "tron_absmax_pow2",
        "tron_kfac_patch_gram", "tron_absmax_pow2", "tron_conv3x3_wgrad"],
    "ac_trunk_skip_weight_gradients": [
        "tron_conv3x3_fwd", "tron_px16_from_f32", "tron_px16_from_f32", "tron_conv3x3_ws_split_weights",
        "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd", "tron_conv3x3_ws_train_fwd",
        "tron_conv3x3_ws_train_fwd", "tron_pool_s2", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd",
        "tron_mish_fwd", "tron_mish_fwd", "tron_mish_bwd", "tron_mish_bwd", "tron_mish_bwd", "tron_mish_bwd", "tron_mish_bwd",
        "tron_mish_bwd", "tron_pool_s2_bwd", "tron_absmax_pow2", "tron_px16_grad_from_f32", "tron_conv3x3_ws_split_weights_bwd",
        "tron_conv3x3_ws_dgrad", "tron_conv3x3_ws_dgrad", "tron_conv3x3_ws_dgrad", "tron_conv3x3_ws_dgrad", "tron_conv3x3_ws_dgrad",
        "tron_conv3x3_wgrad"],
    "ac_trunk_infer": [
        "tron_conv3x3_fwd", "tron_px16_from_f32", "tron_conv3x3_ws_split_weights", "tron_conv3x3_ws_fwd", "tron_conv3x3_ws_fwd",
        "tron_conv3x3_ws_fwd", "tron_conv3x3_ws_fwd", "tron_conv3x3_ws_fwd"],
    "pool_conv7_input_grad": [
        "tron_pool12", "tron_conv7_dense", "tron_gemm_f16x3", "tron_mish_fwd", "tron_mish_bwd", "tron_absmax_pow2",
        "tron_gemm_f16x3", "tron_pool12", "tron_gemm_f16x3", "tron_conv7_dense"],
    "pool_conv7_no_input_grad": [
        "tron_pool12", "tron_conv7_dense", "tron_gemm_f16x3", "tron_mish_fwd", "tron_mish_bwd", "tron_absmax_pow2",
        "tron_gemm_f16x3", "tron_conv7_dense"],
    "pool_conv7_cl_26": [
        "tron_pool_conv7_fwd", "tron_pool_conv7_bwd"],
    "conv3x3_hip_12": [
        "tron_conv3x3_fwd", "tron_absmax_pow2", "tron_conv3x3_dgrad", "tron_conv3x3_wgrad"],
    "conv_bias_mish_residual": [
        "tron_conv3x3_fwd", "tron_bias_mish_bwd", "tron_conv3x3_dgrad", "tron_conv3x3_wgrad"],
    "conv1_codes": [
        "tron_conv3x3_fwd", "tron_bias_mish_bwd", "tron_pop_up", "tron_conv3x3_wgrad"],
    "linear_hip_bias": [
        "tron_linear_wgrad"],
    "linear_hip_no_bias": [
        "tron_linear_wgrad"],
    "tail_mlp_training": [
        "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd", "tron_linear_wgrad", "tron_mish_bwd", "tron_linear_wgrad",
        "tron_mish_bwd", "tron_linear_wgrad", "tron_mish_bwd", "tron_linear_wgrad"],
    "tail_mlp_eval": [
        "tron_mish_fwd", "tron_mish_fwd", "tron_mish_fwd", "tron_linear_wgrad", "tron_mish_bwd", "tron_linear_wgrad",
        "tron_mish_bwd", "tron_linear_wgrad", "tron_mish_bwd", "tron_linear_wgrad"],
}

CASES = [body_px_12_pool_fused, body_px_12_pool_apart, body_px_26, trunk_px_12, trunk_hip_planes_12, trunk_hip_codes_4_planes,
         trunk_hip_planes_input_grad, trunk_hip_planes_26, ac_trunk_plain, ac_trunk_kfac_stats, ac_trunk_skip_weight_gradients,
         ac_trunk_infer, pool_conv7_input_grad, pool_conv7_no_input_grad, pool_conv7_cl_26, conv3x3_hip_12, conv_bias_mish_residual,
         conv1_codes, linear_hip_bias, linear_hip_no_bias, tail_mlp_training, tail_mlp_eval]


def record(mp, case, **kw):
    """Run `case` with tron._native.check replaced by a recorder: (what the case returns, the names of its native calls in order)."""
    from Net import fused
    nat = fused.nat                                         # tron._native, the module object every caller looks `check` up on
    names, check = [], nat.check

    def recorder(rc, what=""):
        check(rc, what)
        names.append(what)
    mp.setattr(nat, "check", recorder)
    out = case(mp, **kw)
    torch.cuda.synchronize()
    return out, names


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_node_launches(case, monkeypatch):
    _, names = record(monkeypatch, case)
    print(case.__name__, names)
    assert names == EXPECTED[case.__name__]
