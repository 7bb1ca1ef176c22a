"""GPU: float16 activations through the layer surface: DAUConv2d / DAUConv1d / dau_conv2d on float16 input, torch.autocast,
GradScaler training and model.half().  The layer runs in the dtype of its input and casts nothing; parameters of any floating
dtype are used as float32 and receive their gradients in their own dtype."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

from layers import close as _close, make_layer

pytestmark = pytest.mark.gpu


_layer = functools.partial(make_layer, use_bias=False, bias_initializer=None)     # (where a test asks for the bias: zeros)


def test_layer_dtypes_and_values():
    layer = _layer()
    x32 = torch.rand(4, 8, 32, 32, device="cuda")
    x = x32.half().requires_grad_(True)
    y = layer(x)
    assert y.dtype == torch.float16
    dy = torch.randn(y.shape, device="cuda").half()
    y.backward(dy)
    assert x.grad.dtype == torch.float16
    grads16 = {n: p.grad.clone() for n, p in layer.named_parameters() if p.grad is not None}
    assert all(g.dtype == torch.float32 for g in grads16.values()) and "weights" in grads16
    layer.zero_grad()
    xr = x.detach().float().requires_grad_(True)                 # the same layer on the widened input
    yr = layer(xr)
    yr.backward(dy.float())
    _close(y, yr)
    _close(x.grad, xr.grad)
    for n, g in grads16.items():
        _close(g, dict(layer.named_parameters())[n].grad)


def test_autocast_conv_dau_conv():
    dau = _layer(S=16, F=16, use_bias=True)
    net = nn.Sequential(nn.Conv2d(3, 16, 3, padding=1), dau, nn.Conv2d(16, 4, 3, padding=1)).cuda()
    seen = []
    dau.register_forward_hook(lambda m, inp, out: seen.append((inp[0].dtype, out.dtype)))
    x = torch.rand(2, 3, 24, 24, device="cuda")
    with torch.autocast("cuda", dtype=torch.float16):
        out = net(x)
        loss = out.float().pow(2).mean()
    loss.backward()
    # the DAU layer saw float16; its f16 output plus the fp32 bias is promoted to fp32, as with bf16
    assert seen == [(torch.float16, torch.float32)]
    for n, p in net.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all(), n


def test_grad_scaler_skips_an_overflowing_step_and_takes_the_next():
    dau = _layer(S=16, F=16)
    net = nn.Sequential(nn.Conv2d(3, 16, 3, padding=1), dau, nn.Conv2d(16, 4, 3, padding=1)).cuda()
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 40)    # dy of the DAU layer overflows float16
    x = torch.rand(2, 3, 24, 24, device="cuda")

    def step():
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.float16):
            loss = net(x).float().pow(2).mean()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()

    before = [p.detach().clone() for p in net.parameters()]
    step()
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, net.parameters()))     # skipped
    assert scaler.get_scale() == 2.0 ** 39
    scaler.update(1024.0)
    step()
    assert scaler.get_scale() == 1024.0                                                   # no overflow at a sane scale
    changed = [not torch.equal(a, p.detach()) for a, p in zip(before, net.parameters()) if p.requires_grad]
    assert all(changed)
    for p in net.parameters():
        assert torch.isfinite(p).all()


def test_half_model_trains():
    ref = _layer(use_bias=True)
    half = copy.deepcopy(ref).half()
    w0 = half.weights.detach().clone()
    x = torch.rand(4, 8, 32, 32, device="cuda").half()
    opts = [torch.optim.SGD(m.parameters(), lr=1e-3) for m in (ref, half)]
    for it in range(2):
        for m, o, xi in ((ref, opts[0], x.float()), (half, opts[1], x)):
            o.zero_grad()
            y = m(xi)
            assert y.dtype == xi.dtype
            (y.float().pow(2).sum() * 1e-3).backward()             # dy = 2e-3 y: normal float16 values
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
    assert not torch.equal(half.weights, w0)                                                          # it did train


def test_conv1d_and_functional_accept_f16():
    import dau_conv
    torch.manual_seed(0)
    l1 = dau_conv.DAUConv1d(filters=16, dau_units=(1, 2), max_kernel_size=9, in_channels=8, use_bias=False).cuda()
    x = torch.rand(2, 8, 8, 32, device="cuda")
    y16 = l1(x.half())
    assert y16.dtype == torch.float16
    _close(y16, l1(x.half().float()))
    xf = x.half().requires_grad_(True)
    out = dau_conv.dau_conv2d(xf, 8, (2, 2), 9, data_format="NCHW", scope="f16_scope")
    assert out.dtype == torch.float32                 # f16 output + the fp32 bias of the functional form
    out.sum().backward()
    assert xf.grad.dtype == torch.float16 and torch.isfinite(xf.grad).all()
