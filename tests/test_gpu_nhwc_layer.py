"""GPU: channels_last activations through the layer surface.  On a channels_last input DAUConv2d / DAUConv1d run the NHWC plan
(channels_last=True; with the default None where dau_conv._NHWC_BY_DEFAULT says so for the dtype): no copy of x, a channels_last
output, a channels_last input gradient -- and the bits of the same layer on the contiguous tensors.  Where the library has no NHWC
plan (dense_bf16 layers, shapes of the direct kernels) and with channels_last=False the layer converts and returns contiguous
tensors, as it always did."""
import functools
import sys
import warnings

import pytest
import torch
import torch.nn as nn

from layers import make_layer
from util import bits as _bits

pytestmark = pytest.mark.gpu

CL = torch.channels_last


_layer = functools.partial(make_layer, S=6, F=8, use_bias=False)


def _is_cl(t):
    return t.is_contiguous(memory_format=CL) and not t.is_contiguous()


def _step(layer, x, dy):
    """forward + backward -> (y, dx, {parameter: grad}).  dx is the tensor the layer's backward returned, caught by a hook: x.grad
    is laid out like x whatever arrives (autograd's accumulation does that)."""
    layer.zero_grad()
    x = x.detach().requires_grad_(True)
    caught = []
    x.register_hook(caught.append)
    y = layer(x)
    y.backward(dy)
    assert len(caught) == 1 and torch.equal(_bits(caught[0]), _bits(x.grad))
    return y.detach(), caught[0], {n: p.grad.clone() for n, p in layer.named_parameters() if p.grad is not None}


def _x(N=2, S=6, H=17, W=13, dtype=torch.float32):
    g = torch.Generator().manual_seed(1)
    return torch.rand(N, S, H, W, generator=g).to(dtype).cuda()


def test_channels_last_input_gives_channels_last_output_with_the_same_bits():
    layer = _layer(channels_last=True)
    x = _x()
    y = layer(x.to(memory_format=CL))
    assert _is_cl(y)                                        # (before the feature: a contiguous tensor)
    assert torch.equal(_bits(y), _bits(layer(x)))
    assert layer(x).is_contiguous()


@pytest.mark.parametrize("grad_cl", [True, False], ids=["dy_channels_last", "dy_contiguous"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_backward_gradients_are_channels_last_and_bit_equal(dtype, grad_cl):
    layer = _layer(channels_last=True)
    x = _x(dtype=dtype)
    dy = torch.randn(2, 8, 17, 13, device="cuda").to(dtype)
    y0, dx0, g0 = _step(layer, x, dy)
    y1, dx1, g1 = _step(layer, x.to(memory_format=CL), dy.to(memory_format=CL) if grad_cl else dy)
    assert y0.is_contiguous() and dx0.is_contiguous()
    assert _is_cl(y1) and _is_cl(dx1) and dx1.dtype == dtype
    assert torch.equal(_bits(y1), _bits(y0)) and torch.equal(_bits(dx1), _bits(dx0))
    assert set(g1) == set(g0) and "weights" in g0 and "mu1" in g0
    for n in g0:
        assert torch.equal(g1[n].view(torch.int32), g0[n].view(torch.int32)), n


def test_no_copy_of_a_channels_last_input():
    """the tensor saved for backward is the caller's"""
    layer = _layer(channels_last=True)
    x = _x().to(memory_format=CL).requires_grad_(True)
    y = layer(x)
    saved = [t for t in y.grad_fn.saved_tensors if t.shape == x.shape]
    assert saved and saved[0].data_ptr() == x.data_ptr()


def test_autocast_channels_last_network():
    dau = _layer(S=16, F=16, channels_last=True)
    net = nn.Sequential(nn.Conv2d(3, 16, 3, padding=1), dau, nn.Conv2d(16, 4, 3, padding=1)).cuda().to(memory_format=CL)
    seen = []
    dau.register_forward_hook(lambda m, inp, out: seen.append((inp[0].dtype, _is_cl(inp[0]), out.dtype, _is_cl(out))))
    x = torch.rand(2, 3, 24, 24, device="cuda").to(memory_format=CL)
    with torch.autocast("cuda", dtype=torch.float16):
        out = net(x)
        loss = out.float().pow(2).mean()
    loss.backward()
    assert seen == [(torch.float16, True, torch.float16, True)]
    for n, p in net.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n


def test_channels_last_false_is_the_contiguous_path():
    layer = _layer(channels_last=False)
    x = _x()
    dy = torch.randn(2, 8, 17, 13, device="cuda")
    y0, dx0, g0 = _step(layer, x, dy)
    y1, dx1, g1 = _step(layer, x.to(memory_format=CL), dy.to(memory_format=CL))
    assert y1.is_contiguous() and dx1.is_contiguous()
    assert torch.equal(_bits(y1), _bits(y0)) and torch.equal(_bits(dx1), _bits(dx0))
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_default_follows_the_measured_table(dtype):
    """channels_last=None: the NHWC plan for the dtypes where it measured faster than converting (dau_conv._NHWC_BY_DEFAULT),
    today's conversion elsewhere; the values are the same either way"""
    import dau_conv  # noqa: F401
    mod = sys.modules["dau_conv.dau_conv"]          # (the package attribute of that name is the op)
    layer = _layer()
    x = _x(dtype=dtype)
    y = layer(x.to(memory_format=CL))
    assert _is_cl(y) == mod._NHWC_BY_DEFAULT[dtype] and y.is_contiguous() != mod._NHWC_BY_DEFAULT[dtype]
    assert torch.equal(_bits(y), _bits(layer(x)))


def test_dense_bf16_layer_falls_back_to_converting():
    layer = _layer(S=8, F=16, dense_bf16=True, channels_last=True)
    x = _x(S=8, H=16, W=16, dtype=torch.bfloat16)
    dy = torch.randn(2, 16, 16, 16, device="cuda").bfloat16()
    y0, dx0, g0 = _step(layer, x, dy)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # the fall-back does not warn
        y1, dx1, g1 = _step(layer, x.to(memory_format=CL), dy.to(memory_format=CL))
    assert y1.is_contiguous() and dx1.is_contiguous()
    assert torch.equal(_bits(y1), _bits(y0)) and torch.equal(_bits(dx1), _bits(dx0))
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n


def test_direct_kernel_shape_falls_back_to_converting():
    """(2, 2, 2, 18, 16, 16) under max_kernel_size 65: no tiled gather-dot, so no NHWC plan; the layer converts as before (and warns
    about the direct kernels exactly as it does for a contiguous input)"""
    import dau_conv
    layer = _layer(S=2, F=2, dau_units=(3, 6), max_kernel_size=65, channels_last=True,
                   mu1_initializer=dau_conv.random_uniform_initializer(-20, 20),
                   mu2_initializer=dau_conv.random_uniform_initializer(-20, 20))
    x = _x(S=2, H=16, W=16)
    dy = torch.randn(2, 2, 16, 16, device="cuda")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        # (a first call leaves the plan its offset-bucket hint: the two calls compared below then run the same kernel sets --
        # under max_kernel_size 65 a call without a hint runs the static bucket's kernels, whose sums come in another order)
        _step(layer, x, dy)
        y0, dx0, g0 = _step(layer, x, dy)
        y1, dx1, g1 = _step(layer, x.to(memory_format=CL), dy.to(memory_format=CL))
    assert y1.is_contiguous() and dx1.is_contiguous()
    assert torch.equal(_bits(y1), _bits(y0)) and torch.equal(_bits(dx1), _bits(dx0))
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n


def test_one_channel_input_takes_the_nchw_plan():
    """C = 1: the strides fit both layouts; such a tensor counts as contiguous"""
    import dau_conv  # noqa: F401
    mod = sys.modules["dau_conv.dau_conv"]          # (the package attribute of that name is the op)
    layer = _layer(S=1, F=8, channels_last=True)
    x = _x(S=1).to(memory_format=CL)
    before = {k for k, p in mod._PLANS.items() if p.io_layout == "NHWC"}
    y = layer(x)
    assert y.is_contiguous()
    assert {k for k, p in mod._PLANS.items() if p.io_layout == "NHWC"} == before
    assert torch.equal(_bits(y), _bits(layer(x.contiguous())))


def test_conv1d_on_a_channels_last_input():
    import dau_conv
    layer = _layer(S=8, F=16, cls=dau_conv.DAUConv1d, dau_units=(1, 2), channels_last=True)
    x = _x(S=8, H=8, W=32)
    dy = torch.randn(2, 16, 8, 32, device="cuda")
    y0, dx0, g0 = _step(layer, x, dy)
    y1, dx1, g1 = _step(layer, x.to(memory_format=CL), dy.to(memory_format=CL))
    assert _is_cl(y1) and _is_cl(dx1)
    assert torch.equal(_bits(y1), _bits(y0)) and torch.equal(_bits(dx1), _bits(dx0))
    for n in g0:
        assert torch.equal(g1[n].view(torch.int32), g0[n].view(torch.int32)), n
