"""GPU: the fused residual add through the layer surface.  DAUConv2d(fused_epilogue=True)(x, residual=r) is the last layer of a
residual block, y = relu((dau(x) + bias) + r), with both adds and the ReLU inside the op's store: for float32 the output and every
gradient that depends on dz are bit for bit those of the composition torch.relu(layer_without_activation(x) + r), the residual's
gradient is dz itself, the output keeps the input's dtype, and any residual the kernels cannot take is added in torch."""
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
    """the same parameters: the unfused layer WITHOUT its activation (the composition applies it after the add), and the fused layer"""
    fused = _layer(fused_epilogue=True, **kw)
    plain = copy.deepcopy(fused)
    plain.fused_epilogue = False
    plain.activation = None
    return plain, fused


def _step(fn, layer, x, r, dy):
    """forward + backward of fn(x, r) -> y, x.grad, r.grad, parameter gradients"""
    layer.zero_grad()
    x = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    r = r.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    y = fn(x, r)
    y.backward(dy)
    return y.detach(), x.grad, r.grad, {n: p.grad.clone() for n, p in layer.named_parameters() if p.grad is not None}


def _data(S, F, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(2, S, 16, 16, device="cuda", generator=g)
    r = torch.randn(2, F, 16, 16, device="cuda", generator=g)
    dy = torch.randn(2, F, 16, 16, device="cuda", generator=g)
    return x, r, dy


def _i32(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("S, F", [(8, 16), (128, 128)], ids=["exact", "default_128_split"])
def test_fused_residual_is_the_composition_in_fp32(S, F):
    plain, fused = _pair(S=S, F=F)
    x, r, dy = _data(S, F)
    r = r * plain(x).detach().std()                          # the shortcut at the size of the branch: the ReLU cuts about half
    y0, dx0, dr0, g0 = _step(lambda a, b: torch.relu(plain(a) + b), plain, x, r, dy)
    y1, dx1, dr1, g1 = _step(lambda a, b: fused(a, residual=b), fused, x, r, dy)
    assert 0.2 < float((y0 == 0).float().mean()) < 0.8
    assert torch.equal(_i32(y1), _i32(y0)) and torch.equal(_i32(dx1), _i32(dx0))
    for n in ("weights", "mu1", "mu2"):
        assert torch.equal(_i32(g1[n]), _i32(g0[n])), n
    want_dr = torch.ops.aten.threshold_backward(dy, y0, 0)
    assert torch.equal(_i32(dr1), _i32(want_dr)) and torch.equal(_i32(dr0), _i32(want_dr))
    _check_bias_grad(g1["bias"], y0, dy)
    assert g1["bias"].dtype == torch.float32 and g1["bias"].shape == (F,)


def test_without_relu_the_residual_gradient_is_dy():
    x, r, dy = _data(8, 16)
    for kw in (dict(activation=None), dict(activation=None, use_bias=False)):
        plain, fused = _pair(**kw)
        y0, dx0, dr0, g0 = _step(lambda a, b: plain(a) + b, plain, x, r, dy)
        y1, dx1, dr1, g1 = _step(lambda a, b: fused(a, residual=b), fused, x, r, dy)
        assert torch.equal(_i32(y1), _i32(y0)) and torch.equal(_i32(dx1), _i32(dx0)) and set(g1) == set(g0)
        assert torch.equal(_i32(dr1), _i32(dy))
        for n in ("weights", "mu1", "mu2"):
            assert torch.equal(_i32(g1[n]), _i32(g0[n])), n


def test_only_the_residual_needs_a_gradient():
    plain, fused = _pair()
    x, r, dy = _data(8, 16)
    for p in fused.parameters():
        p.requires_grad_(False)
    rr = r.clone().requires_grad_(True)
    y = fused(x, residual=rr)
    y.backward(dy)
    assert torch.equal(_i32(rr.grad), _i32(torch.ops.aten.threshold_backward(dy, y.detach(), 0)))
    assert 0.2 < float((rr.grad == 0).float().mean()) < 0.8
    assert all(p.grad is None for p in fused.parameters())
    # nothing needs a gradient: no graph at all
    assert not fused(x, residual=r).requires_grad


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_autocast_residual_block_keeps_16_bit_activations(dtype):
    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(1)
            self.stem = nn.Conv2d(3, 16, 3, padding=1)
            self.a, self.b = _layer(S=16, F=16, fused_epilogue=True), _layer(S=16, F=16, fused_epilogue=True)
            self.head = nn.Conv2d(16, 4, 3, padding=1)

        def forward(self, x):
            h = self.stem(x)
            return self.head(self.b(self.a(h), residual=h))

    net = Block().cuda()
    seen = []
    net.a.register_forward_hook(lambda m, inp, out: seen.append((inp[0].dtype, out.dtype)))
    net.b.register_forward_hook(lambda m, inp, out: seen.append((inp[0].dtype, out.dtype)))
    x = torch.rand(2, 3, 24, 24, device="cuda")
    with torch.autocast("cuda", dtype=dtype):
        loss = net(x).float().pow(2).mean()
    loss.backward()
    assert seen == [(dtype, dtype), (dtype, dtype)]
    for n, p in net.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all(), n
    assert net.stem.weight.grad.abs().sum() > 0 and net.b.bias.grad.abs().sum() > 0


def test_residuals_the_kernels_cannot_take_are_added_in_torch():
    x, r, dy = _data(8, 16)
    # a float32 residual on a float16 input: torch's promotion, a float32 result
    plain, fused = _pair()
    want = torch.relu(plain(x.half()) + r)
    got = fused(x.half(), residual=r)
    assert got.dtype == want.dtype == torch.float32
    _close(got, want)
    # a residual that broadcasts
    rb = r[:1, :, :1, :1].contiguous()
    _close(fused(x, residual=rb), torch.relu(plain(x) + rb))
    y0, dx0, dr0, g0 = _step(lambda a, b: torch.relu(plain(a) + b), plain, x, rb, dy)
    y1, dx1, dr1, g1 = _step(lambda a, b: fused(a, residual=b), fused, x, rb, dy)
    assert dr1.shape == rb.shape
    _close(dr1, dr0)
    _close(dx1, dx0)
    # strides = 2: the residual has the sampled shape
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain2, fused2 = _pair(strides=2)
    rs = r[:, :, ::2, ::2].contiguous()
    got2 = fused2(x, residual=rs)
    assert got2.shape == (2, 16, 8, 8)
    _close(got2, torch.relu(plain2(x) + rs))
    # fused_epilogue=False: after the bias, before the activation
    unfused = copy.deepcopy(fused)
    unfused.fused_epilogue = False
    _close(unfused(x, residual=r), torch.relu(plain(x) + r))
    # another activation is applied after the fused add
    plain3, fused3 = _pair(activation=torch.tanh)
    plain3.activation = None
    assert torch.equal(fused3(x, residual=r), torch.tanh(plain3(x) + r))


def test_a_layer_without_a_residual_is_unchanged():
    import dau_conv
    _, fused = _pair()
    x, r, dy = _data(8, 16)
    assert torch.equal(_i32(fused(x)), _i32(fused(x, residual=None))) and torch.equal(_i32(fused.call(x)), _i32(fused(x)))
    default = _layer()
    assert torch.equal(_i32(default(x)), _i32(default(x, residual=None)))
    # channels_last in: the residual is brought to the plan's layout, the output is channels_last, the contiguous call's bits
    cl = torch.channels_last
    _, fcl = _pair(channels_last=True)
    y0 = fcl(x, residual=r)
    y1 = fcl(x.to(memory_format=cl), residual=r)
    y2 = fcl(x.to(memory_format=cl), residual=r.to(memory_format=cl))
    assert y1.is_contiguous(memory_format=cl) and torch.equal(y1, y0) and torch.equal(y2, y0)
    # the 1-D layer takes a residual as well
    l1 = dau_conv.DAUConv1d(filters=16, dau_units=(1, 2), max_kernel_size=9, in_channels=8, activation=torch.relu, fused_epilogue=True).cuda()
    xh = torch.rand(2, 8, 8, 32, device="cuda").half()
    rh = torch.randn(2, 16, 8, 32, device="cuda").half()
    y = l1(xh, residual=rh)
    assert y.dtype == torch.float16 and bool((y >= 0).all()) and not torch.equal(y, l1(xh))
