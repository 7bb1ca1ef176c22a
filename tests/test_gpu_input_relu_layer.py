"""GPU: the fused input ReLU through the layer surface.  DAUConv2d(input_activation="relu")(x) is DAUConv2d(...)(torch.relu(x)) with
the ReLU inside the op -- the kernels clamp x where they load it and mask the input gradient by x in its store -- so outputs and all
gradients are equal by value (ReLU rounds nothing), for float32, under autocast to float16 and bfloat16, for contiguous and
channels_last inputs; a BatchNorm2d -> DAU stack trains with identical losses in both forms; layers whose plan cannot take the flag
(dense_bf16=True) apply torch.relu in front.  (process_group= is not covered here: the worker of test_gpu_distributed.py builds its
own layer and would have to change for it.)"""
import copy

import pytest
import torch
import torch.nn as nn

from layers import _leave_the_plan_cache_as_it_was, make_layer as _layer, same as _same  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu


def _pair(**kw):
    """the same parameters: the layer as it is (the composition applies torch.relu in front of it), and the layer with the ReLU fused"""
    fused = _layer(input_activation="relu", **kw)
    plain = copy.deepcopy(fused)
    plain.input_activation, plain._input_relu = None, False
    return plain, fused


def _step(fn, params, x, dy):
    for p in params:
        p.grad = None
    x = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    y = fn(x)
    y.backward(dy.to(y.dtype) if dy.shape == y.shape else dy)
    return y.detach(), x.grad, [None if p.grad is None else p.grad.clone() for p in params]


def _share(x):
    share = float((x <= 0).float().mean())
    assert 0.2 < share < 0.8, share


def _fused_plans():
    import importlib
    impl = importlib.import_module("dau_conv.dau_conv")
    return [p for p in impl._PLANS.values() if p.input_relu]


@pytest.mark.parametrize("channels_last", [False, True], ids=["contiguous", "channels_last"])
@pytest.mark.parametrize("mode", ["float32", "autocast_f16", "autocast_bf16"])
@pytest.mark.parametrize("S, F", [(8, 16), (128, 128)], ids=["exact", "default_128_split"])
def test_fused_is_relu_in_front(S, F, mode, channels_last):
    """a convolution in front (under autocast it hands the layer a 16-bit tensor), then the DAU layer with and without its fused ReLU;
    the gradients compared are the layer's own -- with respect to its input and its parameters -- not the convolution's, whose
    backward kernels are not the layer's and need not give the same bits twice"""
    plain, fused = _pair(S=S, F=F)
    torch.manual_seed(1)
    conv = nn.Conv2d(3, S, 1, bias=False).cuda()
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(2, 3, 16, 16, device="cuda", generator=g)
    dy = torch.randn(2, F, 16, 16, device="cuda", generator=g)
    if channels_last:
        conv = conv.to(memory_format=torch.channels_last)
        x, dy = x.contiguous(memory_format=torch.channels_last), dy.contiguous(memory_format=torch.channels_last)
    dtype = {"float32": None, "autocast_f16": torch.float16, "autocast_bf16": torch.bfloat16}[mode]

    with torch.no_grad(), torch.autocast("cuda", dtype=dtype, enabled=dtype is not None):
        h = conv(x)
    assert h.dtype == (dtype or torch.float32) and h.is_contiguous(memory_format=torch.channels_last) == channels_last
    _share(h)

    def run(layer, relu_in_front):
        def fn(a):
            with torch.autocast("cuda", dtype=dtype, enabled=dtype is not None):
                return layer(torch.relu(a) if relu_in_front else a)
        return _step(fn, list(layer.parameters()), h, dy)

    before = len(_fused_plans())
    y0, dx0, g0 = run(plain, True)
    assert len(_fused_plans()) == before
    y1, dx1, g1 = run(fused, False)
    assert _fused_plans(), "the fused layer ran no DAU_FLAG_INPUT_RELU plan"
    _same(y1, y0, "y")
    _same(dx1, dx0, "x.grad")
    assert dx1.dtype == h.dtype and len(g0) == len(g1) and all(a is not None for a in g1[:3])
    for i, (a, b) in enumerate(zip(g1, g0)):
        if b is None:
            assert a is None
            continue
        _same(a, b, "parameter gradient %d" % i)
    if channels_last:
        assert y1.is_contiguous(memory_format=torch.channels_last) == y0.is_contiguous(memory_format=torch.channels_last)


def test_every_spelling_of_relu_is_fused_and_other_callables_run_in_front():
    plain, fused = _pair()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(2, 8, 16, 16, device="cuda", generator=g)
    _share(x)
    want = plain(torch.relu(x))
    import dau_conv
    for act in ("relu", torch.relu, nn.functional.relu, nn.ReLU(), nn.ReLU(inplace=True)):
        # (the constructor's normalisation is under test: a fresh layer, the same parameters)
        fresh = dau_conv.DAUConv2d(filters=16, dau_units=(2, 2), max_kernel_size=9, in_channels=8, mu_learning_rate_factor=1.0,
                                   input_activation=act).cuda()
        fresh.load_state_dict(plain.state_dict())
        xin = x.clone()
        _same(fresh(xin), want, repr(act))
        assert torch.equal(xin, x), "the input was written (an in-place ReLU must not run)"
    other = copy.deepcopy(plain)
    other.input_activation, other._input_relu = torch.tanh, False
    _same(other(x), plain(torch.tanh(x)), "tanh in front")


def test_autograd_saves_the_raw_input():
    """the ReLU's output is never materialised: what the op keeps for backward is the tensor it was given"""
    plain, fused = _pair(use_bias=False)
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(2, 8, 16, 16, device="cuda", generator=g).requires_grad_(True)
    y = fused(x)
    saved = y.grad_fn.saved_tensors[0]
    assert saved.data_ptr() == x.data_ptr() and bool((saved < 0).any())
    y0 = plain(torch.relu(x))
    assert y0.grad_fn.saved_tensors[0].data_ptr() != x.data_ptr() and not bool((y0.grad_fn.saved_tensors[0] < 0).any())


def test_a_batchnorm_dau_stack_trains_with_identical_losses():
    import dau_conv

    def dau(S, F, fused):
        torch.manual_seed(S)
        return dau_conv.DAUConv2d(filters=F, dau_units=(2, 2), max_kernel_size=9, in_channels=S, mu_learning_rate_factor=1.0,
                                  mu1_initializer=dau_conv.random_uniform_initializer(-3, 3),
                                  mu2_initializer=dau_conv.random_uniform_initializer(-3, 3),
                                  input_activation="relu" if fused else None)

    def model(fused):
        torch.manual_seed(0)
        act = (lambda: nn.Identity()) if fused else (lambda: nn.ReLU())
        return nn.Sequential(nn.BatchNorm2d(8), act(), dau(8, 16, fused), nn.BatchNorm2d(16), act(), dau(16, 8, fused)).cuda()

    composed, fused = model(False), model(True)
    fused.load_state_dict(composed.state_dict())
    g = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn(4, 8, 16, 16, device="cuda", generator=g)
    target = torch.randn(4, 8, 16, 16, device="cuda", generator=g)
    losses = []
    for m in (composed, fused):
        opt = torch.optim.SGD(m.parameters(), lr=0.05)
        run = []
        for _ in range(4):
            opt.zero_grad()
            loss = ((m(x) - target) ** 2).mean()
            loss.backward()
            opt.step()
            run.append(float(loss.detach()))
        losses.append(run)
    dau_conv.check_pending_offsets()
    assert losses[0] == losses[1], losses
    assert len(set(losses[0])) == 4, "the stack did not train"
    for a, b in zip(composed.state_dict().values(), fused.state_dict().values()):
        assert torch.equal(a, b)


def test_dense_bf16_falls_back_to_relu_in_front():
    plain, fused = _pair(S=32, F=32, dense_bf16=True)
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(2, 32, 16, 16, device="cuda", generator=g).bfloat16()
    dy = torch.randn(2, 32, 16, 16, device="cuda", generator=g).bfloat16()
    _share(x)
    before = len(_fused_plans())
    y0, dx0, g0 = _step(lambda a: plain(torch.relu(a)), list(plain.parameters()), x, dy)
    y1, dx1, g1 = _step(lambda a: fused(a), list(fused.parameters()), x, dy)
    assert len(_fused_plans()) == before, "a dense_bf16 layer has no DAU_FLAG_INPUT_RELU plan"
    _same(y1, y0, "y")
    _same(dx1, dx0, "x.grad")
    for a, b in zip(g1, g0):
        if b is None:                                          # (sigma is not trained)
            assert a is None
            continue
        _same(a, b, "parameter gradient")


def test_conv1d_strides_and_the_output_epilogue():
    import dau_conv
    g = torch.Generator(device="cuda").manual_seed(13)
    x = torch.randn(2, 8, 16, 16, device="cuda", generator=g)
    _share(x)
    # DAUConv1d
    plain, fused = _pair(cls=dau_conv.DAUConv1d)
    dy = torch.randn(2, 16, 16, 16, device="cuda", generator=g)
    a, b = _step(lambda t: plain(torch.relu(t)), list(plain.parameters()), x, dy), _step(fused, list(fused.parameters()), x, dy)
    _same(b[0], a[0], "1d y")
    _same(b[1], a[1], "1d x.grad")
    for u, v in zip(b[2], a[2]):
        if v is not None:
            _same(u, v, "1d parameter gradient")
    # strides = 2 (the sampled stride-1 output)
    with pytest.warns(UserWarning):
        plain, fused = _pair(strides=2)
    dy2 = torch.randn(2, 16, 8, 8, device="cuda", generator=g)
    a, b = _step(lambda t: plain(torch.relu(t)), list(plain.parameters()), x, dy2), _step(fused, list(fused.parameters()), x, dy2)
    assert b[0].shape == (2, 16, 8, 8)
    _same(b[0], a[0], "strided y")
    _same(b[1], a[1], "strided x.grad")
    # fused_epilogue with a residual: ReLU in front, bias + residual + ReLU behind, one call
    plain, fused = _pair(fused_epilogue=True, activation=torch.relu)
    r = torch.randn(2, 16, 16, 16, device="cuda", generator=g)
    a = _step(lambda t: plain(torch.relu(t), residual=r), list(plain.parameters()), x, dy)
    b = _step(lambda t: fused(t, residual=r), list(fused.parameters()), x, dy)
    assert 0.2 < float((a[0] == 0).float().mean()) < 0.8
    _same(b[0], a[0], "epilogue y")
    _same(b[1], a[1], "epilogue x.grad")
    for u, v in zip(b[2], a[2]):
        if v is not None:
            _same(u, v, "epilogue parameter gradient")
