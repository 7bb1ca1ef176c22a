"""GPU: DAU layers inside captured graphs -- torch.cuda.graph (whole training step; forward + backward), make_graphed_callables and the
cudagraph trees of torch.compile(backend="cudagraphs").

The yardstick of a replay is the EAGER layer on the same tensors, bit for bit (torch.equal): a replay runs the kernels the eager call
runs, with their fixed summation order, and results never depend on the offset-bucket hint that a capture freezes.  The eager layer is
tested against the oracle elsewhere; the first test ties a replay to the oracle as well.

Shapes: N=4, 12 -> 24 channels, 28 x 28, 2 x 2 units, kernel 9 unless said otherwise.  Captures are single-stream (linear graphs), every
one is preceded by a synchronize, and no graph is replayed after an assertion about it has failed."""
import copy
import functools
import importlib
import warnings

import numpy as np
import pytest
import torch

import dau_conv
import layers as fixtures
from dau_conv import _capi
from oracle import dau_oracle as orc
from util import assert_parity

pytestmark = pytest.mark.gpu
dc = importlib.import_module("dau_conv.dau_conv")            # (the package attribute of that name is the op function)

N, S, F, H, W = 4, 12, 24, 28, 28


@pytest.fixture(autouse=True)
def _fresh_plan_cache():
    """Every test starts and ends without cached plans: the graphs of the test before are gone, so are their plans' pending records."""
    def clear():
        torch.cuda.synchronize()
        getattr(dc, "_PINNED", set()).clear()
        dc._PLANS.clear()
    clear()
    yield
    clear()


make_layer = functools.partial(fixtures.make_layer, S=S, F=F, mu=2.5, bias_initializer=None)       # (the layer's own zero bias)
rand_x = functools.partial(fixtures.rand_x, shape=(N, S, H, W))
rand_dy = functools.partial(fixtures.rand_dy, shape=(N, F, H, W))


def fwd_bwd(layer, x, dy, autocast=None, **fw):
    """One eager forward + backward from clean gradients -> [y, dx, the parameters' gradients]."""
    x.grad = None
    for t in fw.values():
        t.grad = None
    layer.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=autocast, enabled=autocast is not None):
        y = layer(x, **fw)
    y.backward(dy)
    return [y.detach(), x.grad] + [p.grad for p in layer.parameters() if p.requires_grad]


def capture_fwd_bwd(layer, x, dy, stream=None, autocast=None, **fw):
    """Warm the layer up where the caller has not, capture forward + backward -> (graph, the static result tensors)."""
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        outs = fwd_bwd(layer, x, dy, autocast, **fw)
    return graph, outs


def assert_equal(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), \
            "%s: tensor %d of the replay differs from the eager layer (max |diff| %.3e)" % (what, i, float((g.float() - w.float()).abs().max()))


def replay_equals_eager(graph, outs, layer, twin, x, dy, what, autocast=None, **fw):
    """Replay, then the eager twin (the layer's parameters, copies of the static inputs) -> the replay's results must be its bits."""
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in outs]
    twin.load_state_dict(layer.state_dict())
    want = fwd_bwd(twin, x.detach().clone().requires_grad_(True), dy.clone(), autocast,
                   **{k: v.detach().clone() for k, v in fw.items()})
    torch.cuda.synchronize()
    assert_equal(got, want, what)


def captured_plans():
    return [dc._PLANS[k] for k in dc._PINNED]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. a whole training step with a trainable sigma
# ---------------------------------------------------------------------------------------------------------------------------------
def test_whole_training_step_with_a_trainable_sigma():
    layer = make_layer(dau_sigma_trainable=True, fused_epilogue=True, activation=torch.relu)
    twin = copy.deepcopy(layer)
    lr = 1e-3                                                # (sigma moves, and stays far inside the support it has: (0.4, 0.6])
    opt, topt = torch.optim.SGD(layer.parameters(), lr=lr), torch.optim.SGD(twin.parameters(), lr=lr)
    target = rand_dy(77).relu()
    sx = rand_x(0).requires_grad_(True)                      # the graph's static input

    def step(model, optimizer, x):
        x.grad = None
        optimizer.zero_grad(set_to_none=True)
        y = model(x)
        loss = torch.nn.functional.mse_loss(y, target)
        loss.backward()
        optimizer.step()
        return y, loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(3):                                   # warm-up steps: they move sigma's version counter
            sx.data.copy_(rand_x(10 + i))
            step(layer, opt, sx)
    torch.cuda.current_stream().wait_stream(side)
    for i in range(3):
        step(twin, topt, rand_x(10 + i).requires_grad_(True))
    torch.cuda.synchronize()
    assert layer.sigma._version > 0
    for p, q in zip(layer.parameters(), twin.parameters()):
        assert torch.equal(p, q)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):               # today: .item() on sigma under capture
        y, loss = step(layer, opt, sx)
    for i in range(3):
        x = rand_x(20 + i)
        before = [p.detach().clone() for p in (layer.weights, layer.mu1, layer.mu2, layer.sigma, layer.bias)]
        sx.data.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        tx = x.clone().requires_grad_(True)
        ty, tloss = step(twin, topt, tx)
        torch.cuda.synchronize()
        assert torch.equal(loss, tloss) and torch.equal(y, ty), "replay %d: loss %r, eager %r" % (i, float(loss), float(tloss))
        for (name, p), q in zip(layer.named_parameters(), twin.parameters()):
            assert torch.equal(p, q), "replay %d: parameter %s differs from the eager twin's" % (i, name)
        assert torch.equal(sx.grad, tx.grad)
    dau_conv.check_pending_offsets()
    assert 0.4 < float(layer.sigma) <= 0.6
    assert len(captured_plans()) == 1 and captured_plans()[0].sigma_status() == (7, 7, 0)

    # the last replay against the oracle, at the suite's fp32 bar: y = relu(DAU + bias), and the gradients of the DAU for the error
    # that reaches it through the loss and the ReLU
    w, mu1, mu2, sigma, bias = (t.cpu().numpy() for t in before)
    xn = x.cpu().numpy()
    want_y = np.maximum(orc.forward(xn, w, mu1, mu2, float(sigma[0])) + bias.reshape(1, -1, 1, 1), 0.0)
    assert_parity(y.detach().cpu().numpy(), want_y, "replay: y")
    yn = y.detach().cpu().numpy().astype(np.float64)
    dz = (2.0 * (yn - target.cpu().numpy()) / yn.size * (yn > 0)).astype(np.float32)
    want = orc.backward(xn, dz, w, mu1, mu2, float(sigma[0]))
    got = dict(dx=sx.grad, dw=layer.weights.grad, dmu1=layer.mu1.grad, dmu2=layer.mu2.grad)
    for key, t in got.items():
        assert_parity(t.cpu().numpy(), want[key], "replay: " + key)
    # sigma is one scalar: its gradient is the sum of the units' -- the bar of each term (1e-4 of it, and 1e-6 of the largest), summed
    ds = want["dsigma"].astype(np.float64)
    tol = 1e-4 * np.abs(ds).sum() + 1e-6 * np.abs(ds).max() * ds.size
    assert abs(float(layer.sigma.grad) - ds.sum()) <= tol, (float(layer.sigma.grad), ds.sum(), tol)
    # the bias gradient: the bound include/dau_conv.h states for dau_conv_epilogue_backward, 2^-16 of the channel's sum of |dz|
    dbias = layer.bias.grad.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(dbias - dz.astype(np.float64).sum(axis=(0, 2, 3))) <= 2.0 ** -16 * np.abs(dz).astype(np.float64).sum(axis=(0, 2, 3)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the workspace of a captured call
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_capture_leaves_the_shared_workspace_alone():
    layer = make_layer()
    twin = copy.deepcopy(layer)
    x, dy = rand_x(1).requires_grad_(True), rand_dy(2)
    torch.cuda.synchronize()
    _capi._SHARED_WS.clear()                                 # (a cache: whatever earlier tests grew it to, it starts at this layer's size)
    fwd_bwd(layer, x, dy)                                    # warm-up on the current stream
    torch.cuda.synchronize()
    shared = lambda: {key: (ws.data_ptr(), ws.numel()) for key, ws in _capi._SHARED_WS.items()}
    before = shared()
    assert before
    graph, outs = capture_fwd_bwd(layer, x, dy, stream=torch.cuda.Stream())       # a NEW stream: today a new key appears
    assert shared() == before, "the capture touched the shared workspace"
    assert dc._PLANS and len(captured_plans()) == 1
    for plan in dc._PLANS.values():
        last = getattr(plan, "_last_ws", None)
        assert last is None or (last.data_ptr(), last.numel()) in before.values(), "the plan keeps a workspace of the capture"
    replay_equals_eager(graph, outs, layer, twin, x, dy, "first replay")
    # a larger layer grows (replaces) the shared workspace; the graph holds none of it
    big = make_layer(seed=1, S=48, F=48)
    fwd_bwd(big, rand_x(3, shape=(N, 48, 56, 56)).requires_grad_(True), rand_dy(4, shape=(N, 48, 56, 56)))
    torch.cuda.synchronize()
    grown = shared()
    assert any(grown[k][1] > before[k][1] for k in before), "the larger layer was meant to grow the shared workspace"
    del big
    x.data.copy_(rand_x(5))
    replay_equals_eager(graph, outs, layer, twin, x, dy, "replay after the shared workspace grew")
    dau_conv.check_pending_offsets()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. formats
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["f16_autocast", "bf16", "channels_last", "input_relu", "residual", "conv1d_line"])
def test_formats_replay_as_eager(case):
    dtype, mf, autocast, kw, fw, cls = torch.float32, torch.contiguous_format, None, {}, {}, None
    if case == "f16_autocast":
        dtype, autocast = torch.float16, torch.float16
    elif case == "bf16":
        dtype = torch.bfloat16
    elif case == "channels_last":
        mf = torch.channels_last
    elif case == "input_relu":
        kw = dict(input_activation="relu")
    elif case == "residual":
        kw = dict(fused_epilogue=True, activation=torch.relu)
        fw = dict(residual=(rand_dy(9) * 0.1).requires_grad_(True))
    elif case == "conv1d_line":
        cls, kw = dau_conv.DAUConv1d, dict(dense_line=True, dense_line_grads=True)
    kw.setdefault("use_bias", False)                         # (an unfused float32 bias would promote a 16-bit output)
    layer = make_layer(cls=cls, **kw)
    if case == "bf16":
        layer = layer.bfloat16()
    twin = copy.deepcopy(layer)
    x = rand_x(1, dtype=dtype, memory_format=mf)
    if case == "input_relu":
        x = x - 0.5
    x.requires_grad_(True)
    dy = rand_dy(2, dtype=dtype, memory_format=mf)
    fwd_bwd(layer, x, dy, autocast, **fw)                    # warm-up
    graph, outs = capture_fwd_bwd(layer, x, dy, None, autocast, **fw)
    if fw:
        outs = outs + [fw["residual"].grad]
    for i in range(2):
        if i:
            x.data.copy_(rand_x(30, dtype=dtype, memory_format=mf) - (0.5 if case == "input_relu" else 0.0))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        twin.load_state_dict(layer.state_dict())
        tfw = {k: v.detach().clone().requires_grad_(True) for k, v in fw.items()}
        want = fwd_bwd(twin, x.detach().clone().requires_grad_(True), dy.clone(), autocast, **tfw)
        if fw:
            want = want + [tfw["residual"].grad]
        torch.cuda.synchronize()
        assert_equal(got, want, "%s replay %d" % (case, i))
        assert got[0].dtype == dtype and got[0].is_contiguous(memory_format=mf)
    dau_conv.check_pending_offsets()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. offsets that move across members and buckets between replays
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,start,end", [(9, 2.5, 3.9), (17, 3.0, 7.0)])
def test_offsets_move_across_members_and_buckets_in_a_replay(kernel, start, end):
    layer = make_layer(max_kernel_size=kernel, mu=start)
    with torch.no_grad():                                    # max|mu| is exactly `start`
        for mu in (layer.mu1, layer.mu2):
            mu.mul_(start / float(mu.abs().max()))
    twin = copy.deepcopy(layer)
    x, dy = rand_x(1).requires_grad_(True), rand_dy(2)
    for _ in range(2):
        fwd_bwd(layer, x, dy)                                # warm-up: the capture's hint is the small bucket
    graph, outs = capture_fwd_bwd(layer, x, dy)
    replay_equals_eager(graph, outs, layer, twin, x, dy, "max|mu| = %g" % start)
    with torch.no_grad():
        layer.mu1.mul_(end / start)
        layer.mu2.mul_(-end / start)
    assert abs(float(layer.mu1.abs().max()) - end) < 1e-5
    replay_equals_eager(graph, outs, layer, twin, x, dy, "max|mu| = %g" % end)
    replay_equals_eager(graph, outs, layer, twin, x, dy, "max|mu| = %g, again" % end)
    dau_conv.check_pending_offsets()


def test_the_exact_tiled_gather_replays_as_eager_when_weights_and_inputs_change():
    """dense_split=False: y and dx through the exact tiled gather of bucket 4 (one offset window: the unit table is packed into a slice
    that the pass clears first), the parameter gradients through the exact gather-dot.  The table follows the weights and offsets,
    so they change between the replays as well as the input; captured after ONE ordinary call."""
    layer = make_layer(dense_split=False)
    twin = copy.deepcopy(layer)
    x, dy = rand_x(1).requires_grad_(True), rand_dy(2)
    fwd_bwd(layer, x, dy)
    graph, outs = capture_fwd_bwd(layer, x, dy)
    plan, = captured_plans()
    assert plan.info["gather_dense_split"] == 0 and plan.info["algo_forward"] == _capi.ALGO_TILED and plan.info["gather_windows"] == 1
    for i in range(4):
        if i:
            x.data.copy_(rand_x(60 + i))
            dy.copy_(rand_dy(70 + i))
            with torch.no_grad():
                layer.weights.mul_(-1.25)
                layer.mu1.mul_(0.9)
                layer.mu2.add_(0.11)
        replay_equals_eager(graph, outs, layer, twin, x, dy, "exact gather, replay %d" % i)
    dau_conv.check_pending_offsets()


def test_units_leaving_and_rejoining_the_line_in_a_replay():
    """A single-dimension layer with the line members of both passes (dense_line, dense_line_grads; dense_split=True holds them at this
    size): the backward pass counts the units off the line for its parameter-gradient table, puts the count back to zero and counts
    again for the input-gradient table.  Replays with every unit on the line, with some off it (mu2 != 0), and on it again must each
    be the eager layer's bits: a count left over from the pass before would send a pass to the wrong member."""
    layer = make_layer(dau_unit_single_dim=True, dense_line=True, dense_line_grads=True, dense_split=True, use_bias=False)
    with torch.no_grad():
        layer.mu2.zero_()
    twin = copy.deepcopy(layer)
    x, dy = rand_x(1).requires_grad_(True), rand_dy(2)
    fwd_bwd(layer, x, dy)
    graph, outs = capture_fwd_bwd(layer, x, dy)
    plan, = captured_plans()
    assert plan.info["gather_dense_split"] & (1 << 6) and plan.info["gather_dense_split"] & (1 << 8), plan.info
    for i, off_line in enumerate((False, True, False, True, True, False)):
        x.data.copy_(rand_x(80 + i))
        with torch.no_grad():
            layer.mu2.zero_()
            if off_line:
                layer.mu2[0, ::3, 1, ::5] = 1.3 + 0.1 * i
        replay_equals_eager(graph, outs, layer, twin, x, dy, "replay %d, units %s the line" % (i, "off" if off_line else "on"))
    dau_conv.check_pending_offsets()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the sigma guard
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_replay_whose_sigma_outgrows_the_plan_is_reported():
    layer = make_layer()
    twin = copy.deepcopy(layer)
    x, dy = rand_x(1).requires_grad_(True), rand_dy(2)
    fwd_bwd(layer, x, dy)
    graph, outs = capture_fwd_bwd(layer, x, dy)              # sigma 0.5: support 7
    plan, = captured_plans()
    assert plan.info["blur_support"] == 7
    with torch.no_grad():
        layer.sigma.fill_(0.55)                              # still 7 taps: the replay is the eager layer
    replay_equals_eager(graph, outs, layer, twin, x, dy, "sigma 0.55")
    assert plan.sigma_status() == (7, 7, 0)
    with torch.no_grad():
        layer.sigma.fill_(0.35)                              # 5 taps would do: reported, no error
    graph.replay()
    torch.cuda.synchronize()
    assert plan.sigma_status() == (5, 7, 0)
    dau_conv.check_pending_offsets()
    with torch.no_grad():
        layer.sigma.fill_(0.7)                               # 9 taps: more than the captured plan holds
    graph.replay()
    with pytest.raises(_capi.FailedPreconditionError) as e:
        dau_conv.check_pending_offsets()
    assert "sigma" in str(e.value) and "9" in str(e.value) and "7" in str(e.value) and "capture again" in str(e.value)
    dau_conv.check_pending_offsets()                         # sticky, and cleared by the report
    assert plan.sigma_status() == (9, 7, 0)
    # the eager layer at 0.7 plans for 9 taps
    twin.load_state_dict(layer.state_dict())
    fwd_bwd(twin, x.detach().clone().requires_grad_(True), dy)
    dau_conv.check_pending_offsets()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. a NaN offset in a replay
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("check_offsets", ["async", True])
def test_a_nan_offset_in_a_replay_is_reported(check_offsets):
    layer = make_layer(check_offsets=check_offsets)
    x, dy = rand_x(1).requires_grad_(True), rand_dy(2)
    fwd_bwd(layer, x, dy)
    graph, outs = capture_fwd_bwd(layer, x, dy)              # check_offsets=True cannot wait under capture: it runs as "async"
    graph.replay()
    dau_conv.check_pending_offsets()
    with torch.no_grad():
        layer.mu1[0, 0, 0, 0] = float("nan")
    graph.replay()
    with pytest.raises(_capi.FailedPreconditionError) as e:
        dau_conv.check_pending_offsets()
    assert "NaN" in str(e.value)
    dau_conv.check_pending_offsets()                         # reported once


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. torch.cuda.make_graphed_callables
# ---------------------------------------------------------------------------------------------------------------------------------
def test_make_graphed_callables_trains_as_eager():
    layer = make_layer()
    twin = copy.deepcopy(layer)
    opt, topt = torch.optim.SGD(layer.parameters(), lr=1e-2), torch.optim.SGD(twin.parameters(), lr=1e-2)
    target = rand_dy(77)
    torch.cuda.synchronize()
    graphed = torch.cuda.make_graphed_callables(layer, (rand_x(0).requires_grad_(True),))
    for i in range(3):
        losses = []
        for model, optimizer in ((graphed, opt), (twin, topt)):
            x = rand_x(40 + i).requires_grad_(True)
            optimizer.zero_grad(set_to_none=True)
            y = model(x)
            loss = torch.nn.functional.mse_loss(y, target)
            loss.backward()
            optimizer.step()
            torch.cuda.synchronize()
            losses.append((loss.detach().clone(), y.detach().clone(), x.grad.clone()))
        for a, b in zip(*losses):
            assert torch.equal(a, b), "step %d" % i
        for (name, p), q in zip(layer.named_parameters(), twin.parameters()):
            assert torch.equal(p, q), "step %d: parameter %s" % (i, name)
    dau_conv.check_pending_offsets()


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the cudagraph trees of torch.compile
# ---------------------------------------------------------------------------------------------------------------------------------
def test_torch_compile_cudagraphs_backend_trains_as_eager():
    import torch._dynamo
    torch._dynamo.reset()
    stack = torch.nn.Sequential(make_layer(dau_sigma_trainable=True), torch.nn.ReLU(),
                                make_layer(seed=1, S=F, dau_sigma_trainable=True))
    twin = copy.deepcopy(stack)
    opt, topt = torch.optim.SGD(stack.parameters(), lr=1e-3), torch.optim.SGD(twin.parameters(), lr=1e-3)
    target = rand_dy(77)
    compiled = torch.compile(stack, backend="cudagraphs")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for i in range(5):                                   # the trees warm up, record (today: the recording call fails) and replay
            results = []
            for model, optimizer in ((compiled, opt), (twin, topt)):
                x = rand_x(50 + i)
                optimizer.zero_grad(set_to_none=True)
                loss = torch.nn.functional.mse_loss(model(x), target)
                loss.backward()
                results.append(loss.detach().clone())
                optimizer.step()                             # outside the compiled call
                torch.cuda.synchronize()
            assert torch.equal(*results), "step %d: loss %r, eager %r" % (i, float(results[0]), float(results[1]))
            for (name, p), q in zip(stack.named_parameters(), twin.parameters()):
                assert torch.equal(p, q), "step %d: parameter %s" % (i, name)
    dau_conv.check_pending_offsets()
    assert captured_plans(), "no call was captured: the backend did not record a graph"
    pool = [str(w.message) for w in seen if any(s in str(w.message).lower() for s in ("pool", "live", "overwritten", "skipping cudagraphs"))]
    assert not pool, pool
    del compiled
    torch._dynamo.reset()


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _eager_still_works():
    torch.cuda.synchronize()
    layer = make_layer(seed=3)
    y, dx = fwd_bwd(layer, rand_x(1).requires_grad_(True), rand_dy(2))[:2]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    dau_conv.check_pending_offsets()


def test_a_first_call_under_capture_is_refused():
    layer = make_layer()
    x, dy = rand_x(1).requires_grad_(True), rand_dy(2)
    torch.cuda.synchronize()
    with pytest.raises(_capi.FailedPreconditionError) as e:
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            layer(x)
    assert "run the layer once before capturing" in str(e.value)
    # a trainable sigma that no call has read yet is refused for the same reason, before any plan is looked up
    other = make_layer(seed=2, dau_sigma_trainable=True)
    torch.cuda.synchronize()
    with pytest.raises(_capi.FailedPreconditionError) as e:
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            other(x)
    assert "run the layer once before capturing" in str(e.value)
    assert not torch.cuda.is_current_stream_capturing()
    _eager_still_works()


def test_a_process_group_layer_under_capture_is_refused():
    layer = make_layer(process_group=True)
    x, dy = rand_x(1).requires_grad_(True), rand_dy(2)
    fwd_bwd(layer, x, dy)                                    # (no process group is initialised: the layer runs locally)
    torch.cuda.synchronize()
    with pytest.raises(_capi.InvalidArgumentError) as e:
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            layer(x)
    assert "process_group" in str(e.value)
    assert not torch.cuda.is_current_stream_capturing()
    _eager_still_works()


def test_workspace_queries_after_a_captured_call_are_refused():
    plan = _capi.Plan(N, S, F, 4, H, W, max_kernel_size=9, sigma_hint=0.5)
    x, dy = rand_x(1), rand_dy(2)
    w = torch.randn(1, S, 4, F, device="cuda") * 0.1
    mu1, mu2 = torch.rand(1, S, 4, F, device="cuda") * 4 - 2, torch.rand(1, S, 4, F, device="cuda") * 4 - 2
    sigma = torch.full((1, S, 4, F), 0.5, device="cuda")
    plan.forward(x, w, mu1, mu2, sigma)
    assert plan.check_status() <= 2.0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = plan.forward(x, w, mu1, mu2, sigma)
    assert plan.captured and plan._last_ws is None
    for query in (plan.check_status, plan.outlier_status, plan.line_status, plan.dot_line_status):
        with pytest.raises(_capi.FailedPreconditionError) as e:
            query()
        assert "last_status" in str(e.value) and "sigma_status" in str(e.value)
    graph.replay()
    torch.cuda.synchronize()
    assert plan.last_status() <= 2.0 and plan.sigma_status() == (7, 7, 0)
    want = plan.forward(x, w, mu1, mu2, sigma)               # an eager call, and the queries answer again
    assert plan.check_status() <= 2.0 and torch.equal(y, want)
    _eager_still_works()
