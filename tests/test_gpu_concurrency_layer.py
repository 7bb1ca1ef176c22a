"""GPU: the Python front end with more than one call in flight.  Every layer of a shape shares one dau_conv._capi.Plan through the
cache dau_conv.dau_conv._PLANS, and every (device, stream) has one grow-only workspace in dau_conv._capi._SHARED_WS; here two layers
of one shape run on two streams, from one host thread and from two.

The yardstick is the same steps run serially -- deep copies of the layers, one stream, one call after the other -- bit for bit
(torch.equal): a call runs the kernels its own offsets need, with their fixed summation order, whatever runs beside it.  The serial
layer is tested against the oracle elsewhere (test_gpu_layer.py, test_gpu_graph_capture.py).

Shapes as in test_gpu_graph_capture.py: N=4, 12 -> 24 channels, 28 x 28, 2 x 2 units, kernel 9, float32.  One process, no graph
capture, at most two streams and two threads beside the main one; each test is one pass, and a thread that has not come back after
JOIN_SECONDS fails its test, which then makes no further GPU call."""
import copy
import functools
import importlib
import threading

import pytest
import torch

import dau_conv
import layers as fixtures
from dau_conv import _capi

pytestmark = pytest.mark.gpu
dc = importlib.import_module("dau_conv.dau_conv")            # (the package attribute of that name is the op function)

N, S, F, H, W = 4, 12, 24, 28, 28
STEPS, JOIN_SECONDS = 3, 120


@pytest.fixture(autouse=True)
def _fresh_plan_cache():
    """Every test starts and ends without cached plans, pending records and shared workspaces."""
    def clear():
        torch.cuda.synchronize()
        dc._PINNED.clear()
        dc._PLANS.clear()
        _capi._SHARED_WS.clear()
    clear()
    yield
    clear()


make_layer = functools.partial(fixtures.make_layer, S=S, F=F, mu=2.5, bias_initializer=None)       # (the layer's own zero bias)
rand_x = functools.partial(fixtures.rand_x, shape=(N, S, H, W))
rand_dy = functools.partial(fixtures.rand_dy, shape=(N, F, H, W))


def fwd_bwd(layer, x, dy):
    """One forward + backward from clean gradients -> [y, dx, the parameters' gradients]; nothing waits."""
    x = x.detach().requires_grad_(True)
    layer.zero_grad(set_to_none=True)
    y = layer(x)
    y.backward(dy)
    return [y.detach(), x.grad] + [p.grad for p in layer.parameters() if p.requires_grad]


def assert_equal(got, want, what):
    assert len(got) == len(want) >= 5
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), \
            "%s: tensor %d differs from the serial run (max |diff| %.3e)" % (what, i, float((g.float() - w.float()).abs().max()))


def shared_workspaces():
    return {key[1]: (ws.data_ptr(), ws.numel()) for key, ws in _capi._SHARED_WS.items()}


def _pair(**kw):
    """layers A and B of one shape and different seeds, their serial twins, two streams, inputs for STEPS steps; both layers warmed
    up on their own streams (a plan's first call, and the streams' workspaces)"""
    a, b = make_layer(seed=1, **kw), make_layer(seed=2, **kw)
    twins = copy.deepcopy(a), copy.deepcopy(b)
    xs = [[rand_x(100 + 10 * l + i) for i in range(STEPS)] for l in range(2)]
    dys = [[rand_dy(200 + 10 * l + i) for i in range(STEPS)] for l in range(2)]
    streams = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for layer, s in zip((a, b), streams):
        with torch.cuda.stream(s):
            fwd_bwd(layer, xs[0][0], dys[0][0])
    torch.cuda.synchronize()
    assert len(dc._PLANS) == 1, "layers of one shape were meant to share a plan"
    return (a, b), twins, streams, xs, dys


def _serial(twins, xs, dys):
    want = [[fwd_bwd(twin, xs[l][i], dys[l][i]) for i in range(STEPS)] for l, twin in enumerate(twins)]
    torch.cuda.synchronize()
    return want


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------------
def test_two_layers_of_one_shape_on_two_streams():
    layers, twins, streams, xs, dys = _pair()
    got = [[None] * STEPS, [None] * STEPS]
    for i in range(STEPS):                                   # A on stream 1, B on stream 2, alternately, and nothing waits
        for l in range(2):
            with torch.cuda.stream(streams[l]):
                got[l][i] = fwd_bwd(layers[l], xs[l][i], dys[l][i])
    torch.cuda.synchronize()
    assert len(dc._PLANS) == 1
    ws = shared_workspaces()                                 # (before the serial run, which uses the default stream's)
    want = _serial(twins, xs, dys)
    for l in range(2):
        for i in range(STEPS):
            assert_equal(got[l][i], want[l][i], "layer %s step %d" % ("AB"[l], i))
    assert sorted(ws) == sorted(s.cuda_stream for s in streams), "one shared workspace per stream: %r" % (ws,)
    (p0, n0), (p1, n1) = ws.values()
    assert p0 + n0 <= p1 or p1 + n1 <= p0, "the two streams' workspaces overlap: %r" % (ws,)
    dau_conv.check_pending_offsets()


# ---- 8 -----------------------------------------------------------------------------------------------------------------------------------
def test_one_streams_workspace_grows_while_the_other_works():
    layers, twins, streams, xs, dys = _pair()
    big = make_layer(seed=3, S=48, F=48)
    bx, bdy = rand_x(300, shape=(N, 48, 56, 56)), rand_dy(301, shape=(N, 48, 56, 56))
    torch.cuda.synchronize()
    before = shared_workspaces()
    got = [[None] * STEPS, [None] * STEPS]
    for i in range(STEPS):
        for l in range(2):
            with torch.cuda.stream(streams[l]):
                got[l][i] = fwd_bwd(layers[l], xs[l][i], dys[l][i])
        if i == 0:
            with torch.cuda.stream(streams[0]):              # between B's steps: stream 1's workspace is replaced by a larger one
                fwd_bwd(big, bx, bdy)
    torch.cuda.synchronize()
    after = shared_workspaces()
    s1, s2 = (s.cuda_stream for s in streams)
    assert after[s1][1] > before[s1][1], "the larger layer was meant to grow stream 1's workspace"
    assert after[s2] == before[s2], "stream 2's workspace changed: %r -> %r" % (before[s2], after[s2])
    want = _serial(twins, xs, dys)
    for l in range(2):
        for i in range(STEPS):
            assert_equal(got[l][i], want[l][i], "layer %s step %d" % ("AB"[l], i))
    dau_conv.check_pending_offsets()


# ---- 9 -----------------------------------------------------------------------------------------------------------------------------------
def test_a_bad_offset_on_one_stream_is_reported_once():
    """check_offsets="async" raises for a bad offset at the first call of the plan that is made after the bad call has COMPLETED,
    or in check_pending_offsets().  So that the test does not depend on when that is, layer A's call with the NaN is the last one
    enqueued, a forward call alone, while B's steps are still in flight on the other stream: no call of the plan follows it, and
    check_pending_offsets() is where the NaN must surface -- once."""
    layers, twins, streams, xs, dys = _pair(check_offsets="async")
    a, b = layers
    with torch.no_grad():
        a.mu1[0, 3, 1, 5] = float("nan")
    torch.cuda.synchronize()
    got = [None] * STEPS
    with torch.cuda.stream(streams[1]):
        for i in range(STEPS):
            got[i] = fwd_bwd(b, xs[1][i], dys[1][i])
    with torch.cuda.stream(streams[0]), torch.no_grad():
        ya = a(xs[0][0])
    with pytest.raises(_capi.FailedPreconditionError) as e:
        dau_conv.check_pending_offsets()
    assert "NaN" in str(e.value)
    dau_conv.check_pending_offsets()                         # reported once
    assert torch.isfinite(ya).all()                          # (a NaN offset reads as offset 0)
    want = _serial(twins, xs, dys)
    for i in range(STEPS):
        assert_equal(got[i], want[1][i], "layer B step %d" % i)
    dau_conv.check_pending_offsets()


# ---- 10 ----------------------------------------------------------------------------------------------------------------------------------
def test_two_threads_train_layers_that_share_a_plan():
    steps = 5
    layers = [make_layer(seed=1), make_layer(seed=2)]
    twins = copy.deepcopy(layers)
    target = rand_dy(77)
    xs = [[rand_x(400 + 10 * l + i) for i in range(steps)] for l in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()

    def train(layer, inputs, before_step=lambda: None):
        opt = torch.optim.SGD(layer.parameters(), lr=1e-2)
        for x in inputs:
            before_step()
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.mse_loss(layer(x.detach().requires_grad_(True)), target)
            loss.backward()
            opt.step()

    barrier = threading.Barrier(2)
    failures = [None, None]

    def work(l):
        try:
            with torch.cuda.stream(streams[l]):
                train(layers[l], xs[l], lambda: barrier.wait(JOIN_SECONDS))
                streams[l].synchronize()
        except BaseException as e:                            # noqa: B902 (kept for the main thread, which raises it)
            failures[l] = e
            barrier.abort()

    threads = [threading.Thread(target=work, args=(l,), daemon=True) for l in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(JOIN_SECONDS)
    if any(th.is_alive() for th in threads):
        pytest.fail("a thread has not come back after %d s; no further GPU call is made" % JOIN_SECONDS, pytrace=False)
    for e in failures:
        if e is not None and not isinstance(e, threading.BrokenBarrierError):
            raise e
    assert failures == [None, None], failures
    torch.cuda.synchronize()
    assert len(dc._PLANS) == 1, "the two threads' layers were meant to share a plan"
    for twin, inputs in zip(twins, xs):
        train(twin, inputs)
    torch.cuda.synchronize()
    for l in range(2):
        for (name, p), q in zip(layers[l].named_parameters(), twins[l].parameters()):
            assert torch.equal(p, q), "thread %d: parameter %s after %d steps differs from the twin trained serially" % (l, name, steps)
    dau_conv.check_pending_offsets()
