"""GPU: the fused epilogue through the layer surface.  DAUConv2d(fused_epilogue=True) adds its bias and applies its ReLU inside the
op's store: the output keeps the input's dtype (so the next layer of an autocast stack keeps its 16-bit loads and stores), for
float32 the output and every gradient that depends on dz are bit for bit the unfused layer's, and the bias gradient -- a
hierarchical fp32 sum -- lies within 2^-16 * sum |dz| of the exact sum."""
import copy
import functools
import warnings

import pytest
import torch
import torch.nn as nn

from layers import check_bias_grad as _check_bias_grad, close as _close, make_layer

pytestmark = pytest.mark.gpu


_layer = functools.partial(make_layer, activation=torch.relu)


def _pair(**kw):
    """the same parameters, unfused and fused"""
    plain = _layer(**kw)
    fused = copy.deepcopy(plain)
    fused.fused_epilogue = True
    return plain, fused


def _step(layer, x, dy):
    layer.zero_grad()
    x = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    y = layer(x)
    y.backward(dy)
    return y.detach(), x.grad, {n: p.grad.clone() for n, p in layer.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_autocast_stack_keeps_16_bit_activations(dtype):
    def net_of(fused):
        torch.manual_seed(1)
        a, b = _layer(S=16, F=16, fused_epilogue=fused), _layer(S=16, F=16, fused_epilogue=fused)
        net = nn.Sequential(nn.Conv2d(3, 16, 3, padding=1), a, b, nn.Conv2d(16, 4, 3, padding=1)).cuda()
        seen = []
        for m in (a, b):
            m.register_forward_hook(lambda m, inp, out: seen.append((inp[0].dtype, out.dtype)))
        return net, seen

    x = torch.rand(2, 3, 24, 24, device="cuda")
    for fused in (True, False):
        net, seen = net_of(fused)
        with torch.autocast("cuda", dtype=dtype):
            loss = net(x).float().pow(2).mean()
        loss.backward()
        # the default layer: 16-bit output + fp32 bias is promoted, and the second layer runs on float32
        assert seen == ([(dtype, dtype), (dtype, dtype)] if fused else [(dtype, torch.float32), (torch.float32, torch.float32)])
        for n, p in net.named_parameters():
            if p.requires_grad:
                assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all(), n
        assert all(m.bias.grad.abs().sum() > 0 for m in net if hasattr(m, "fused_epilogue"))


@pytest.mark.parametrize("S, F", [(8, 16), (128, 128)], ids=["exact", "default_128_split"])
def test_fused_layer_is_the_unfused_layer_in_fp32(S, F):
    plain, fused = _pair(S=S, F=F)
    x = torch.rand(2, S, 16, 16, device="cuda")
    dy = torch.randn(2, F, 16, 16, device="cuda")
    y0, dx0, g0 = _step(plain, x, dy)
    y1, dx1, g1 = _step(fused, x, dy)
    assert 0.2 < float((y0 == 0).float().mean()) < 0.8                  # the ReLU cuts
    assert torch.equal(y1, y0) and torch.equal(dx1.view(torch.int32), dx0.view(torch.int32))
    for n in ("weights", "mu1", "mu2"):
        assert torch.equal(g1[n].view(torch.int32), g0[n].view(torch.int32)), n
    _check_bias_grad(g1["bias"], y0, dy)
    _check_bias_grad(g0["bias"], y0, dy)                                # (torch's own sum meets the bound too)
    assert g1["bias"].dtype == torch.float32 and g1["bias"].shape == (F,)


def test_bias_only_and_relu_only():
    x = torch.rand(2, 8, 16, 16, device="cuda")
    dy = torch.randn(2, 16, 16, 16, device="cuda")
    for kw in (dict(activation=None), dict(use_bias=False)):
        plain, fused = _pair(**kw)
        y0, dx0, g0 = _step(plain, x, dy)
        y1, dx1, g1 = _step(fused, x, dy)
        assert torch.equal(y1, y0) and torch.equal(dx1.view(torch.int32), dx0.view(torch.int32)) and set(g1) == set(g0)
        for n in ("weights", "mu1", "mu2"):
            assert torch.equal(g1[n].view(torch.int32), g0[n].view(torch.int32)), n
    # a frozen bias asks for no gradient
    plain, fused = _pair()
    fused.bias.requires_grad_(False)
    _, dx1, g1 = _step(fused, x, dy)
    assert "bias" not in g1 and torch.equal(dx1, _step(plain, x, dy)[1])


def test_half_model_with_the_fused_epilogue_trains():
    """test_gpu_f16_layer.py's test_half_model_trains, fused: parameters stay float16, gradients come back float16, two SGD steps
    track the fp32 layer within that test's tolerances"""
    ref = _layer(fused_epilogue=True)
    half = copy.deepcopy(ref).half()
    w0 = half.weights.detach().clone()
    x = torch.rand(4, 8, 32, 32, device="cuda").half()
    opts = [torch.optim.SGD(m.parameters(), lr=1e-3) for m in (ref, half)]
    for it in range(2):
        for m, o, xi in ((ref, opts[0], x.float()), (half, opts[1], x)):
            o.zero_grad()
            y = m(xi)
            assert y.dtype == xi.dtype
            (y.float().pow(2).sum() * 1e-3).backward()
            if it == 0 and m is half:
                for (n, p), (_, pr) in zip(half.named_parameters(), ref.named_parameters()):
                    assert p.dtype == torch.float16, n
                    if pr.grad is not None:
                        assert p.grad is not None and p.grad.dtype == torch.float16, n
                        _close(p.grad, pr.grad, rel=2e-2)
            o.step()
    for (n, p), (_, pr) in zip(half.named_parameters(), ref.named_parameters()):
        assert p.dtype == torch.float16 and torch.isfinite(p).all(), n
        _close(p, pr, rel=5e-3)
    assert not torch.equal(half.weights, w0) and half.bias.grad is not None


def test_layers_without_a_fused_epilogue_run_unfused():
    """Two layers whose plans fall back to the direct kernels.  (a) The shape of the fallback test in test_gpu_soak.py -- 18 units per
    channel pair under kernel 33; no shape of test_gpu_layer.py falls back -- warns about its parameter gradients only: its forward
    pass stays tiled, so the plan TAKES the epilogue and the layer runs fused.  (b) A layer pinned to the direct kernels: its plan
    refuses the epilogue and the layer adds bias and ReLU in torch, with torch's type promotion.  Both give the unfused layer's results and neither raises."""
    import importlib
    from dau_conv import _capi
    dc = importlib.import_module("dau_conv.dau_conv")
    x = torch.rand(2, 4, 24, 24, device="cuda")
    dy = torch.randn(2, 8, 24, 24, device="cuda")
    for kw, falls_back in ((dict(dau_units=(6, 3), max_kernel_size=33), False), (dict(algo=_capi.ALGO_DIRECT), True)):
        dc._PLANS.clear()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            plain, fused = _pair(S=4, F=8, **kw)
            _step(plain, x, dy)                       # (leaves the plan its offset-bucket hint: the steps below run the same kernels)
            y0, dx0, g0 = _step(plain, x, dy)
            y1, dx1, g1 = _step(fused, x, dy)
        direct = [str(w.message) for w in rec if issubclass(w.category, RuntimeWarning) and "one-thread-per-output" in str(w.message)]
        plans = list(dc._PLANS.values())
        assert len(plans) == 1                        # fused and unfused share the plan
        if falls_back:
            assert plans[0].info["algo_forward"] == _capi.ALGO_DIRECT and plans[0]._epilogue_ok is False and not direct   # (a pinned algo does not warn)
        else:
            assert len(direct) == 1 and "parameter gradients" in direct[0] and "forward" not in direct[0]
            assert plans[0].info["algo_forward"] == _capi.ALGO_TILED and plans[0]._epilogue_ok is True
        assert torch.equal(y1, y0) and torch.equal(dx1, dx0)
        for n in ("weights", "mu1", "mu2"):
            assert torch.equal(g1[n], g0[n]), n
        _check_bias_grad(g1["bias"], y0, dy)


def test_channels_last_strides_and_other_activations():
    x = torch.rand(2, 8, 16, 16, device="cuda")
    dy = torch.randn(2, 16, 16, 16, device="cuda")
    # channels_last in, channels_last out, the contiguous call's bits
    plain, fused = _pair(channels_last=True)
    y0, dx0, g0 = _step(fused, x, dy)
    cl = torch.channels_last
    y1, dx1, g1 = _step(fused, x.to(memory_format=cl), dy.to(memory_format=cl))
    assert y1.is_contiguous(memory_format=cl) and not y1.is_contiguous() and dx1.is_contiguous(memory_format=cl)
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0) and torch.equal(g1["weights"], g0["weights"])
    _check_bias_grad(g1["bias"], y0, dy)
    # strides = 2: the sliced fused result
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain2, fused2 = _pair(strides=2)
    y2 = fused2(x)
    assert y2.shape == (2, 16, 8, 8) and torch.equal(y2, y0[:, :, ::2, ::2]) and torch.equal(y2, plain2(x))
    # another activation is applied after the fused bias
    plain3, fused3 = _pair(activation=torch.tanh)
    y3, dx3, g3 = _step(fused3, x, dy)
    p3 = _step(plain3, x, dy)
    assert torch.equal(y3, p3[0]) and torch.equal(dx3, p3[1])
    # nn.ReLU and the functional relu count as ReLU
    for act in (nn.ReLU(), nn.functional.relu):
        _, fused4 = _pair(activation=act)
        assert torch.equal(fused4(x), y0)


def test_functional_forms_and_conv1d():
    import dau_conv
    torch.manual_seed(0)
    x = torch.rand(2, 8, 8, 32, device="cuda").half()
    out = dau_conv.dau_conv2d(x, 8, (2, 2), 9, data_format="NCHW", scope="fused_epilogue_scope", fused_epilogue=True)
    assert out.dtype == torch.float16 and bool((out >= 0).all())       # bias and the default relu inside the op
    layer = dau_conv.get_scope_layer("fused_epilogue_scope")
    ref = torch.relu(dau_conv.dau_conv(x.float(), layer.weights, layer.mu1.clamp(-3.99, 3.99), layer.mu2.clamp(-3.99, 3.99),
                                       layer.sigma.reshape(1, 1, 1, 1).expand(layer.weights.shape), num_output=8)
                     + layer.bias.view(1, -1, 1, 1))
    assert torch.equal(out, ref.half())
    l1 = dau_conv.DAUConv1d(filters=16, dau_units=(1, 2), max_kernel_size=9, in_channels=8, activation=torch.relu, fused_epilogue=True).cuda()
    y = l1(x)
    assert y.dtype == torch.float16 and bool((y >= 0).all())


def test_process_group_at_world_size_one_matches_the_plain_backward():
    """A layer with process_group=True at world size 1 does NOT reach _data_parallel_backward (the layer takes that path from two
    ranks on): it runs the plain backward, checked first.  The hand-over of dz to the data-parallel path is then exercised directly:
    _data_parallel_backward on a one-rank RCCL group, fed the dz of epilogue_backward, against Plan.backward on the same dz and
    against the layer's own gradients."""
    import importlib
    import os
    import torch.distributed as dist
    from dau_conv import _capi
    dc = importlib.import_module("dau_conv.dau_conv")
    plain, fused = _pair(fused_epilogue=True)
    fused._dau_convolution_op.process_group = True
    x = torch.rand(2, 8, 16, 16, device="cuda")
    dy = torch.randn(2, 16, 16, 16, device="cuda")
    y0, dx0, g0 = _step(plain, x, dy)
    y1, dx1, g1 = _step(fused, x, dy)
    assert torch.equal(y1, y0) and torch.equal(dx1.view(torch.int32), dx0.view(torch.int32))
    for n in g0:
        assert torch.equal(g1[n].view(torch.int32), g0[n].view(torch.int32)), n
    # the data-parallel path itself, on dz
    w, mu1, mu2 = (p.detach().contiguous() for p in (plain.weights, plain.mu1, plain.mu2))
    sigma = torch.full_like(w, 0.5)
    plan = _capi.Plan(2, 8, 16, 4, 16, 16, max_kernel_size=9, sigma_hint=0.5, mu_learning_rate_factor=1.0)
    y = plan.forward(x, w, mu1, mu2, sigma, bias=plain.bias.detach(), relu=True)
    assert torch.equal(y, y0)
    dz, dbias = plan.epilogue_backward(dy, y, relu=True)
    want = plan.backward(x, dz, w, mu1, mu2, sigma)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29547")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        got = dc._data_parallel_backward(plan, x, dz, w, mu1, mu2, sigma, _capi.NEED_ALL, True, "mean")
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(got[0], dx0) and torch.equal(got[1], g0["weights"]) and torch.equal(dbias.view(torch.int32), g0["bias"].view(torch.int32))
