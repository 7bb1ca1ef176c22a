"""GPU: DAU layers inside torch.compile.  The compiled layer is one opaque op (torch.ops.dau_conv.conv, dau_conv/_ops.py) that runs the
kernels the eager layer runs, on the same bits: outputs and every gradient are compared with torch.equal.  backend="aot_eager" traces
through Dynamo and AOT autograd -- everything the ops' registration has to get right -- without generating code.
The smallest layer of the layer tests: N=2, 4 -> 8 channels, 8x9 maps, dau_units=(2, 2), kernel 9."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

from layers import make_layer, same as _same

pytestmark = pytest.mark.gpu

N, S, F, H, W = 2, 4, 8, 8, 9
NEED_ALL = 31


@pytest.fixture(autouse=True)
def _fresh_dynamo_and_the_plan_cache_as_it_was():
    import importlib
    import torch._dynamo
    impl = importlib.import_module("dau_conv.dau_conv")
    torch._dynamo.reset()
    before = set(impl._PLANS)
    yield
    torch._dynamo.reset()
    for key in [k for k in impl._PLANS if k not in before]:
        impl._PLANS.pop(key).last_status()      # (a pending offset error would be raised here, not lost)


_layer = functools.partial(make_layer, S=S, F=F)


def _data(seed=3, S=S, F=F, H=H, W=W, out_hw=None, dtype=torch.float32, channels_last=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(N, S, H, W, device="cuda", generator=g).to(dtype)
    dy = torch.randn((N, F) + (out_hw or (H, W)), device="cuda", generator=g).to(dtype)
    r = torch.randn((N, F) + (out_hw or (H, W)), device="cuda", generator=g).to(dtype)
    if channels_last:
        x, dy, r = (t.contiguous(memory_format=torch.channels_last) for t in (x, dy, r))
    return x, dy, r


def _step(fn, layer, x, dy, residual=None, autocast=None, x_grad=True, residual_grad=True):
    for p in layer.parameters():
        p.grad = None
    x = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(x_grad)
    args = (x,)
    if residual is not None:
        residual = residual.detach().clone(memory_format=torch.preserve_format).requires_grad_(residual_grad)
        args = (x, residual)
    with torch.autocast("cuda", dtype=autocast, enabled=autocast is not None):
        y = fn(*args)
    y.backward(dy.to(y.dtype))
    grads = {n: (None if p.grad is None else p.grad.clone()) for n, p in layer.named_parameters()}
    return y.detach(), x.grad, grads, None if residual is None else residual.grad


def _compare(eager, compiled, layers, x, dy, residual=None, autocast=None, trained=("weights", "mu1", "mu2")):
    """eager and compiled are callables over the layers (eager_layer, compiled_layer): the same parameters, the same inputs"""
    y0, dx0, g0, dr0 = _step(eager, layers[0], x, dy, residual, autocast)
    y1, dx1, g1, dr1 = _step(compiled, layers[1], x, dy, residual, autocast)
    _same(y1, y0, "y")
    assert y1.stride() == y0.stride()
    _same(dx1, dx0, "x.grad")
    assert set(g0) == set(g1)
    for name in g0:
        if g0[name] is None:
            assert g1[name] is None, name
            continue
        _same(g1[name], g0[name], name + ".grad")
    assert all(g1[n] is not None and bool((g1[n] != 0).any()) for n in trained), "a gradient is missing or all zero"
    if residual is not None:
        _same(dr1, dr0, "residual.grad")
    return y1


def _pair(**kw):
    eager = _layer(**kw)
    twin = copy.deepcopy(eager)
    return eager, twin, torch.compile(twin, fullgraph=True, backend="aot_eager")


# ----------------------------------------------------------------------------------------------
# 1. opcheck: schema, fake tensor, autograd registration, AOT dispatch
# ----------------------------------------------------------------------------------------------
def _op_args(dtype, channels_last, epilogue):
    g = torch.Generator(device="cuda").manual_seed(21)
    x, dy, r = _data(dtype=dtype, channels_last=channels_last)
    w = torch.randn(1, S, 4, F, device="cuda", generator=g) * 0.1
    mu1 = torch.rand(1, S, 4, F, device="cuda", generator=g) * 6 - 3
    mu2 = torch.rand(1, S, 4, F, device="cuda", generator=g) * 6 - 3
    sigma = torch.full((1,), 0.5, device="cuda")
    bias = torch.randn(F, device="cuda", generator=g) if epilogue else None
    return x, dy, (r if epilogue else None), w, mu1, mu2, sigma, bias


@pytest.mark.parametrize("epilogue", [False, True], ids=["plain", "bias_relu_residual"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["contiguous", "channels_last"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["float32", "float16"])
def test_opcheck(dtype, channels_last, epilogue):
    import importlib
    import dau_conv
    impl = importlib.import_module("dau_conv.dau_conv")
    x, dy, r, w, mu1, mu2, sigma, bias = _op_args(dtype, channels_last, epilogue)
    st = dau_conv._ops.encode_settings(impl._settings(sigma, sigma_hint=0.5, num_output=F, kernel_size=9))
    relu = bool(epilogue)
    for t in (x, w, mu1, mu2) + ((bias, r) if epilogue else ()):
        t.requires_grad_(True)
    torch.library.opcheck(torch.ops.dau_conv.conv.default, (x, w, mu1, mu2, sigma, bias, r, relu, True) + st)
    with torch.no_grad():
        y = torch.ops.dau_conv.conv(x, w, mu1, mu2, sigma, bias, r, relu, True, *st)
    detached = [t.detach() for t in (x, w, mu1, mu2)]
    for need, need_dbias in ((NEED_ALL, epilogue), (1, False), (NEED_ALL & ~1, epilogue)):
        torch.library.opcheck(torch.ops.dau_conv.conv_backward.default,
                              (dy, detached[0], detached[1], detached[2], detached[3], sigma, y if relu else None, relu, True, need,
                               need_dbias) + st)
    dau_conv.check_pending_offsets()


# ----------------------------------------------------------------------------------------------
# 2. the compiled layer is the eager layer, bit for bit
# ----------------------------------------------------------------------------------------------
def test_default_layer():
    eager, twin, compiled = _pair()
    x, dy, _ = _data()
    _compare(eager, compiled, (eager, twin), x, dy, trained=("weights", "mu1", "mu2", "bias"))


def test_fused_epilogue_bias_and_relu():
    eager, twin, compiled = _pair(fused_epilogue=True, activation=torch.relu)
    x, dy, _ = _data()
    y = _compare(eager, compiled, (eager, twin), x, dy, trained=("weights", "mu1", "mu2", "bias"))
    assert 0.1 < float((y == 0).float().mean()) < 0.9


@pytest.mark.parametrize("activation", [None, torch.relu], ids=["add", "add_relu"])
def test_residual(activation):
    eager, twin, compiled = _pair(fused_epilogue=True, activation=activation)
    x, dy, r = _data()
    _compare(lambda a, b: eager(a, residual=b), lambda a, b: compiled(a, residual=b), (eager, twin), x, dy, residual=r,
             trained=("weights", "mu1", "mu2", "bias"))


def test_residual_of_another_dtype_is_added_outside_the_op():
    eager, twin, compiled = _pair(fused_epilogue=True, activation=torch.relu)
    x, dy, r = _data()
    _compare(lambda a, b: eager(a, residual=b), lambda a, b: compiled(a, residual=b), (eager, twin), x.half(), dy, residual=r)


def test_input_relu():
    eager, twin, compiled = _pair(input_activation="relu")
    x, dy, _ = _data()
    assert 0.2 < float((x <= 0).float().mean()) < 0.8
    _compare(eager, compiled, (eager, twin), x, dy)


def test_strides_2():
    with pytest.warns(UserWarning):
        eager, twin, compiled = _pair(strides=2, fused_epilogue=True, activation=torch.relu)
    x, dy, _ = _data(out_hw=(4, 5))
    y = _compare(eager, compiled, (eager, twin), x, dy)
    assert y.shape == (N, F, 4, 5)


def test_channels_last_input():
    eager, twin, compiled = _pair(input_activation="relu", fused_epilogue=True, activation=torch.relu)
    x, dy, _ = _data(channels_last=True)
    y = _compare(eager, compiled, (eager, twin), x, dy)
    assert y.is_contiguous(memory_format=torch.channels_last) and not y.is_contiguous()


def test_float16_under_autocast():
    eager, twin, compiled = _pair(fused_epilogue=True, activation=torch.relu)
    x, dy, _ = _data(dtype=torch.float16)
    y = _compare(eager, compiled, (eager, twin), x, dy, autocast=torch.float16)
    assert y.dtype == torch.float16


def test_bfloat16_model():
    eager = _layer().bfloat16()
    twin = copy.deepcopy(eager)
    compiled = torch.compile(twin, fullgraph=True, backend="aot_eager")
    x, dy, _ = _data(dtype=torch.bfloat16)
    y = _compare(eager, compiled, (eager, twin), x, dy)
    assert y.dtype == torch.bfloat16 and twin.weights.grad.dtype == torch.bfloat16


def test_conv1d():
    import dau_conv
    eager, twin, compiled = _pair(cls=dau_conv.DAUConv1d)
    x, dy, _ = _data()
    _compare(eager, compiled, (eager, twin), x, dy, trained=("weights", "mu1"))


# ----------------------------------------------------------------------------------------------
# 3. one graph with its neighbours
# ----------------------------------------------------------------------------------------------
def test_a_stack_is_one_graph():
    import torch._dynamo
    from torch._dynamo.testing import CompileCounterWithBackend
    from torch._dynamo.utils import counters
    torch.manual_seed(1)
    model = nn.Sequential(nn.Conv2d(3, S, 1), nn.BatchNorm2d(S),
                          _layer(input_activation="relu", fused_epilogue=True), nn.BatchNorm2d(F), nn.ReLU()).cuda()
    twin = copy.deepcopy(model)
    counters.clear()
    cnt = CompileCounterWithBackend("aot_eager")
    compiled = torch.compile(twin, backend=cnt)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(N, 3, H, W, device="cuda", generator=g)
    dy = torch.randn(N, F, H, W, device="cuda", generator=g)
    y0 = model(x)
    y0.backward(dy)
    y1 = compiled(x)
    y1.backward(dy)
    assert cnt.frame_count == 1, cnt.frame_count
    assert not counters["graph_break"], dict(counters["graph_break"])
    assert any("dau_conv" in str(n.target) for gm in cnt.graphs for n in gm.graph.nodes), "the DAU op is not in the graph"
    # (the neighbours are torch's own kernels, which need not give the same bits twice: a tolerance here, equality in the layer tests)
    torch.testing.assert_close(y1, y0, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(twin[2].weights.grad, model[2].weights.grad, rtol=1e-4, atol=1e-5)


# ----------------------------------------------------------------------------------------------
# 4. a trainable sigma neither recompiles nor is read more often than it changes
# ----------------------------------------------------------------------------------------------
def test_training_sigma_does_not_recompile(monkeypatch):
    import dau_conv
    from torch._dynamo.testing import CompileCounterWithBackend
    eager = _layer(dau_sigma_trainable=True)
    twin = copy.deepcopy(eager)
    cnt = CompileCounterWithBackend("aot_eager")
    compiled = torch.compile(twin, backend=cnt, fullgraph=True)
    reads = []
    read = dau_conv._ops._read_sigma
    monkeypatch.setattr(dau_conv._ops, "_read_sigma", lambda s: reads.append(1) or read(s))
    x, dy, _ = _data()
    target = torch.zeros_like(dy)
    xg = x.clone().requires_grad_(True)          # (as _step's input below: requires_grad of an input is part of the graph's guards)
    for model, fn in ((eager, eager), (twin, compiled)):
        opt = torch.optim.SGD(model.parameters(), lr=1e-3)
        for _ in range(3):
            opt.zero_grad()
            ((fn(xg) - target) ** 2).mean().backward()
            opt.step()
    assert cnt.frame_count == 1, cnt.frame_count
    assert twin.sigma.grad is not None and float(twin.sigma.detach()) != 0.5, "sigma did not train"
    for a, b in zip(eager.state_dict().values(), twin.state_dict().values()):
        assert torch.equal(a, b)
    assert len(reads) == 3, "sigma moved three times and was read %d times" % len(reads)     # forward reads, backward hits
    # across a prefilter-support boundary (7 -> 9 taps): another plan inside the op, the same graph
    with torch.no_grad():
        eager.sigma.fill_(0.61)
        twin.sigma.fill_(0.61)
    _compare(eager, compiled, (eager, twin), x, dy, trained=("weights", "mu1", "mu2", "bias", "sigma"))
    assert cnt.frame_count == 1, cnt.frame_count
    import importlib
    impl = importlib.import_module("dau_conv.dau_conv")
    assert {p.info["blur_support"] for p in impl._PLANS.values() if (p.N, p.S, p.F, p.H, p.W) == (N, S, F, H, W)} >= {7, 9}


def test_a_fixed_sigma_is_read_once(monkeypatch):
    import dau_conv
    eager, twin, compiled = _pair()
    reads = []
    read = dau_conv._ops._read_sigma
    monkeypatch.setattr(dau_conv._ops, "_read_sigma", lambda s: reads.append(1) or read(s))
    x, dy, _ = _data()
    for _ in range(3):
        _step(compiled, twin, x, dy)
    assert len(reads) == 1, len(reads)


# ----------------------------------------------------------------------------------------------
# 5. plan-dependent fallbacks stay inside the op
# ----------------------------------------------------------------------------------------------
def test_dense_bf16_fallbacks_inside_the_op():
    """dense_bf16=True on bfloat16 input: no fused epilogue, no NHWC plan, no input-ReLU flag -- the op applies all three in torch"""
    import importlib
    impl = importlib.import_module("dau_conv.dau_conv")
    eager = _layer(S=32, F=32, dense_bf16=True, input_activation="relu", fused_epilogue=True, activation=torch.relu).bfloat16()
    twin = copy.deepcopy(eager)
    compiled = torch.compile(twin, fullgraph=True, backend="aot_eager")
    x, dy, _ = _data(S=32, F=32, H=16, W=16, dtype=torch.bfloat16, channels_last=True)
    y0, dx0, g0, _ = _step(eager, eager, x, dy)
    y1, dx1, g1, _ = _step(compiled, twin, x, dy)
    plans = [p for p in impl._PLANS.values() if (p.S, p.F, p.H, p.W) == (32, 32, 16, 16)]
    assert plans and all(p.io_layout == "NCHW" and not p.input_relu and not impl._epilogue_ok(p) for p in plans)
    _same(y1.contiguous(), y0.contiguous(), "y")
    _same(dx1.contiguous(), dx0.contiguous(), "x.grad")
    for name in g0:
        if g0[name] is not None:
            _same(g1[name], g0[name], name + ".grad")
    # exactly what the shape function promised: bfloat16, contiguous (DAU_FLAG_IO_NHWC excludes DAU_FLAG_DENSE_BF16)
    assert y1.dtype == torch.bfloat16 and y1.stride() == (32 * 256, 256, 16, 1)
    assert dx1.dtype == torch.bfloat16 and dx1.shape == x.shape


@pytest.mark.parametrize("with_residual", [False, True], ids=["bias_relu", "bias_relu_residual"])
def test_direct_kernel_fallbacks_inside_the_op(with_residual):
    """algo=ALGO_DIRECT on a float32 channels_last input: the direct kernels have no fused epilogue, no NHWC plan and no input-ReLU
    flag -- the op applies all three in torch, on eager's bits (float32: torch's promotion changes nothing).  The one difference is
    the documented one: eager's output is contiguous, the op's output and input gradient are channels_last, as its shape function
    promised."""
    import importlib
    from dau_conv import _capi
    impl = importlib.import_module("dau_conv.dau_conv")
    before = set(impl._PLANS)
    eager, twin, compiled = _pair(algo=_capi.ALGO_DIRECT, fused_epilogue=True, activation=torch.relu, input_activation="relu",
                                  use_bias=True)
    x, dy, r = _data(channels_last=True)
    assert 0.2 < float((x <= 0).float().mean()) < 0.8
    call = (lambda m: lambda a, b: m(a, residual=b)) if with_residual else (lambda m: m)
    y0, dx0, g0, dr0 = _step(call(eager), eager, x, dy, r if with_residual else None)
    y1, dx1, g1, dr1 = _step(call(compiled), twin, x, dy, r if with_residual else None)
    plans = [p for k, p in impl._PLANS.items() if k not in before]
    assert plans and all(p.info["algo_forward"] == _capi.ALGO_DIRECT and p.info["algo_backward"] == _capi.ALGO_DIRECT
                         and p.io_layout == "NCHW" and not p.input_relu and not impl._epilogue_ok(p) for p in plans)
    _same(y1.contiguous(), y0.contiguous(), "y")
    assert 0.1 < float((y1 == 0).float().mean()) < 0.9
    _same(dx1.contiguous(), dx0.contiguous(), "x.grad")
    assert set(g0) == set(g1) == {"weights", "mu1", "mu2", "sigma", "bias"}
    for name in ("weights", "mu1", "mu2", "bias"):
        _same(g1[name], g0[name], name + ".grad")
        assert bool((g1[name] != 0).any()), name
    assert g0["sigma"] is None and g1["sigma"] is None
    if with_residual:
        _same(dr1.contiguous(), dr0.contiguous(), "residual.grad")
    # the two promises: eager lets the NCHW plan's layout through, the op keeps what its shape function said of a channels_last x
    assert y0.is_contiguous()
    for t in (y1, dx1):
        assert t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()


@pytest.mark.parametrize("wanted", ["bias_and_residual", "residual", "x"])
def test_gradient_subsets_of_the_fused_epilogue(wanted):
    """backward's branches when only some gradients are asked for, fused bias + residual + ReLU: (a) need == 0 with the bias and the
    residual gradient wanted, (b) the residual's gradient alone (the masked grad, no DAU pass), (c) the input gradient alone"""
    eager, twin, compiled = _pair(fused_epilogue=True, activation=torch.relu)
    for layer in (eager, twin):
        for name, p in layer.named_parameters():
            p.requires_grad_(name == "bias" and wanted == "bias_and_residual")
    x, dy, r = _data()
    kw = dict(x_grad=wanted == "x", residual_grad=wanted != "x")
    y0, dx0, g0, dr0 = _step(lambda a, b: eager(a, residual=b), eager, x, dy, r, **kw)
    y1, dx1, g1, dr1 = _step(lambda a, b: compiled(a, residual=b), twin, x, dy, r, **kw)
    _same(y1, y0, "y")
    assert y1.stride() == y0.stride()
    assert 0.1 < float((y1 == 0).float().mean()) < 0.9
    got = dict(g1, x=dx1, residual=dr1)
    want = dict(g0, x=dx0, residual=dr0)
    asked = {"bias_and_residual": {"bias", "residual"}, "residual": {"residual"}, "x": {"x"}}[wanted]
    assert {n for n, t in got.items() if t is not None} == {n for n, t in want.items() if t is not None} == asked
    for name in asked:
        _same(got[name], want[name], name + ".grad")
        assert got[name].stride() == want[name].stride(), name
        assert bool((got[name] != 0).any()), name


# ----------------------------------------------------------------------------------------------
# 6. the offset checks survive
# ----------------------------------------------------------------------------------------------
def test_async_offset_check_after_a_compiled_call():
    import dau_conv
    eager, twin, compiled = _pair(check_offsets="async")
    x, dy, _ = _data()
    compiled(x)
    dau_conv.check_pending_offsets()
    with torch.no_grad():
        twin.mu1[0, 1, 2, 3] = float("nan")
    y = compiled(x)                                              # enqueued, not checked yet
    with pytest.raises(dau_conv.FailedPreconditionError):
        dau_conv.check_pending_offsets()
    assert bool(torch.isfinite(y).all())                         # a NaN offset reads as offset 0
    with torch.no_grad():
        twin.mu1[0, 1, 2, 3] = 0.0
    compiled(x)
    dau_conv.check_pending_offsets()


# ----------------------------------------------------------------------------------------------
# 7. process_group= layers leave the graph
# ----------------------------------------------------------------------------------------------
def test_process_group_layer_compiles_with_a_graph_break():
    from torch._dynamo.utils import counters
    eager = _layer(process_group=True)
    twin = copy.deepcopy(eager)
    counters.clear()
    compiled = torch.compile(twin, backend="aot_eager")
    x, dy, _ = _data()
    _compare(eager, compiled, (eager, twin), x, dy)
    assert counters["graph_break"], "a process_group= layer is documented to break the graph"
    with pytest.raises(Exception, match="process_group"):
        torch.compile(copy.deepcopy(eager), backend="aot_eager", fullgraph=True)(x)
