"""GPU: the opt-in line members of the two-limb gather-dot (DAU_FLAG_SPLIT_DOT_LINE, with DAU_FLAG_SINGLE_DIM_KERNEL).  A call whose
units all lie on the row of their pixel (mu2 == 0) runs its parameter gradients as the two-limb f16 GEMM of k_split_dot.hip with a
horizontal radius of 4 (namespace d4) or, for offsets within (4, 8], of 8 (d8) and no vertical halo -- instead of the exact fp32
gather-dot of bucket 4 / 8.  Bar: the fp32 one against the oracle with single_dim_kernel=True (util.assert_parity defaults: 1e-4
relative + 1e-6 of the max-norm) -- the member claims fp32 accuracy, so it gets no bar of its own; margins are recorded with
util.record_margins.  dau_conv_dot_line_status proves which member a call took.  Replaces the same reference code as the exact
gather-dot (dau_conv_backward_core.hpp), for the layers of the reference's test_DAUConv1d."""
import numpy as np
import pytest
import torch

import abi_arena
from oracle import dau_oracle as orc
from util import assert_parity, make_inputs, record_margins

pytestmark = pytest.mark.gpu

BAR = "1e-4 rel + 1e-6 max-norm (fp32 bar; two-limb line gather-dot)"
PARAMS = ("dw", "dmu1", "dmu2", "dsigma")
K = {4: 9, 8: 17}                 # max_kernel_size whose clip is the member's radius
M = {4: 3.99, 8: 7.99}
BITS = {4: 1 << 8, 8: 3 << 8}


def _flags(capi, on=True, forced=True, extra=0):
    return (capi.FLAG_USE_INTERPOLATION | capi.FLAG_SINGLE_DIM_KERNEL | (capi.FLAG_DENSE_SPLIT_F16 if forced else 0) |
            (capi.FLAG_SPLIT_DOT_LINE if on else 0) | extra)


def _plan(shape, radius, on=True, forced=True, extra=0, **kw):
    from dau_conv import _capi as capi
    N, S, F, G, H, W = shape
    plan = capi.Plan(N, S, F, G, H, W, max_kernel_size=K[radius], sigma_hint=kw.pop("sigma_hint", 0.5),
                     flags=_flags(capi, on, forced, extra), **kw)
    if not (extra & capi.FLAG_NO_DENSE_SPLIT):
        assert plan.info["gather_dense_split"] & (3 << 8) == (BITS[radius] if on else 0), bin(plan.info["gather_dense_split"])
    return plan


def _inputs(seed, shape, radius, **kw):
    """make_inputs with the units on the line; the two ends of the member's reach are used"""
    x, dy, w, mu1, mu2 = make_inputs(seed, *shape, K[radius], M[radius], **kw)
    mu2[:] = 0
    mu1.flat[0] = M[radius]; mu1.flat[1] = -M[radius]
    assert np.abs(mu1).max() > radius - 4 and np.abs(mu1).max() <= radius
    return x, dy, w, mu1, mu2


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(plan, x, dy, w, mu1, mu2, dtype=torch.float32, nhwc=False, sigma=0.5, need=None):
    """backward -> (gradients as numpy fp32, dot_line_status)"""
    from dau_conv import _capi
    S, G, F = w.shape[1:]
    sg = torch.full((1, S, G, F), float(sigma), device="cuda")
    xd, dyd = _dev(x).to(dtype), _dev(dy).to(dtype)
    if nhwc:
        xd, dyd = (t.contiguous(memory_format=torch.channels_last) for t in (xd, dyd))
    g = plan.backward(xd, dyd, _dev(w), _dev(mu1), _dev(mu2), sg, need_mask=_capi.NEED_ALL if need is None else need)
    plan.check_status()
    st = plan.dot_line_status()
    torch.cuda.synchronize()
    out = {k: (v.float().cpu().numpy() if v is not None else None) for k, v in zip(("dx",) + PARAMS, g)}
    return out, st


_ORACLE = {}


def _oracle(key, x, dy, w, mu1, mu2, sigma=0.5, **kw):
    """computed once per key, shared by the tests that need it, never written"""
    if key not in _ORACLE:
        want = orc.backward(x, dy, w, mu1, mu2, sigma, need=PARAMS, single_dim_kernel=True, **kw)
        for a in want.values():
            if a is not None:
                a.setflags(write=False)
        _ORACLE[key] = want
    return _ORACLE[key]


def _check(got, want, name, keys=PARAMS):
    m = record_margins(name, {k: got[k] for k in keys}, {k: want[k] for k in keys}, BAR)
    print(name, "margins", {k: "%.2e" % v for k, v in m.items()})
    for key in keys:
        assert_parity(got[key], want[key], name + "/" + key)


def _same(a, b, keys=("dx",) + PARAMS):
    for key in keys:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


SHAPES = [(3, 20, 36, G, 13, 17) for G in range(1, 7)] + [   # ragged octet, channel blocks, unit blocks, regions
    (2, 16, 32, 4, 28, 28),       # H a multiple of four: a thin last item
    (9, 7, 5, 2, 9, 6),           # two octets, one of them with one image; W below every region width; tiny channels
    (3, 16, 16, 2, 1, 40),        # a sequence, the layer's own use: one live row
    (2, 8, 8, 4, 27, 61),         # odd width, several column strips, W + 1 no multiple of a region width
    (1, 33, 130, 3, 12, 33),      # the last input and output blocks almost empty
]
_id = lambda s: "N%d_S%d_F%d_G%d_%dx%d" % tuple(s)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
@pytest.mark.parametrize("radius", [4, 8])
def test_line_dot_against_oracle(shape, radius):
    x, dy, w, mu1, mu2 = _inputs(143 + radius, shape, radius)
    if radius == 8:
        assert np.abs(mu1).max() > 4
    got, st = _run(_plan(shape, radius), x, dy, w, mu1, mu2)
    assert st == (0, radius), st
    _check(got, _oracle(("parity", shape, radius), x, dy, w, mu1, mu2), "linedot/r%d/%s" % (radius, _id(shape)))
    assert not got["dmu2"].any()


@pytest.mark.parametrize("radius", [4, 8])
def test_integer_offsets_and_the_exact_radius(radius):
    """Fraction 0: the corner at +1 carries factor 0 -- for an offset of exactly +R it reads the window's last column."""
    shape = (2, 20, 40, 3, 12, 30)
    x, dy, w, mu1, mu2 = _inputs(161, shape, radius)
    rs = np.random.RandomState(162)
    mu1[:] = rs.randint(-radius, radius + 1, mu1.shape).astype(np.float32)
    mu1.flat[0] = radius; mu1.flat[1] = -radius
    got, st = _run(_plan(shape, radius), x, dy, w, mu1, mu2)
    assert st == (0, radius), st
    _check(got, _oracle(("integer", radius), x, dy, w, mu1, mu2), "linedot/integer/r%d" % radius)
    assert not got["dmu2"].any()


@pytest.mark.parametrize("radius", [4, 8])
def test_without_dsigma_and_edge_rule(radius):
    """kinds = 3 (no dsigma requested), unit_testing edge rule, one ignored unit, sigma 0.8"""
    from dau_conv import _capi
    shape = (2, 12, 20, 4, 32, 32)
    x, dy, w, mu1, mu2 = _inputs(105, shape, radius, ignore=1)
    plan = _plan(shape, radius, extra=_capi.FLAG_UNIT_TESTING, number_units_ignore=1, sigma_hint=0.8)
    got, st = _run(plan, x, dy, w, mu1, mu2, sigma=0.8, need=_capi.NEED_DW | _capi.NEED_DMU1 | _capi.NEED_DMU2)
    assert st == (0, radius), st
    want = _oracle(("kinds3", radius), x, dy, w, mu1, mu2, sigma=0.8, ignore=1, unit_testing=True)
    _check(got, want, "linedot/kinds3/r%d" % radius, keys=("dw", "dmu1", "dmu2"))
    assert not got["dmu2"].any() and got["dsigma"] is None


@pytest.mark.parametrize("radius", [4, 8])
def test_agrees_with_the_exact_kernel(radius):
    from dau_conv import _capi
    shape = (4, 32, 48, 4, 24, 24)
    x, dy, w, mu1, mu2 = _inputs(113, shape, radius)
    got, st = _run(_plan(shape, radius), x, dy, w, mu1, mu2)
    assert st == (0, radius), st
    exact, st = _run(_plan(shape, radius, on=False, forced=False, extra=_capi.FLAG_NO_DENSE_SPLIT), x, dy, w, mu1, mu2)
    assert st == (0, 0), st
    for key in PARAMS:
        assert_parity(got[key], exact[key], "linedot-vs-exact/r%d/%s" % (radius, key))


@pytest.mark.parametrize("radius", [4, 8])
def test_scale_invariance(radius):
    """power-of-two scaling of the inputs scales dw bit-exactly (the scales are exact)"""
    shape = (2, 16, 16, 4, 16, 16)
    x, dy, w, mu1, mu2 = _inputs(117, shape, radius)
    plan = _plan(shape, radius)
    a, st = _run(plan, x, dy, w, mu1, mu2)
    b, st_b = _run(plan, x * np.float32(2.0 ** -12), dy * np.float32(2.0 ** 7), w, mu1, mu2)
    assert st == (0, radius) and st_b == (0, radius)
    np.testing.assert_array_equal(b["dw"], a["dw"] * np.float32(2.0 ** -5))


@pytest.mark.parametrize("radius", [4, 8])
def test_inf_beside_finite_channels(radius):
    shape = (2, 16, 32, 4, 16, 16)
    N, S, F, G, H, W = shape
    x, dy, w, mu1, mu2 = _inputs(111, shape, radius)
    want = _oracle(("inf", radius), x, dy, w, mu1, mu2)
    plan = _plan(shape, radius)
    dyi = dy.copy(); dyi[1, 5, 3, 3] = np.inf
    got, st = _run(plan, x, dyi, w, mu1, mu2)
    assert st == (0, radius), st
    keep = [f for f in range(F) if f != 5]
    for key in PARAMS:
        assert_parity(got[key][..., keep], want[key][..., keep], "linedot/inf-dy/r%d/%s" % (radius, key))
    # an Inf in x, in the image's last row but one: the row below it is no term of any sum
    xi = x.copy(); xi[1, 5, H - 2, 3] = np.inf
    got, st = _run(plan, xi, dy, w, mu1, mu2)
    assert st == (0, radius), st
    keep = [s for s in range(S) if s != 5]
    for key in PARAMS:
        assert np.isfinite(got[key][:, keep]).all(), key
        assert_parity(got[key][:, keep], want[key][:, keep], "linedot/inf-x/r%d/%s" % (radius, key))


@pytest.mark.parametrize("radius", [4, 8])
@pytest.mark.parametrize("what", ["mu2", "nan_weight"])
def test_a_call_off_the_line_is_the_plan_without_the_flag(radius, what):
    """One mu2 = 0.25; or one NaN weight together with DAU_FLAG_DENSE_SPLIT_LINE (dau_conv_backward has the weights: a NaN / Inf
    weight counts as a unit off the line for the parameter-gradient pass as it does for the gather-sum passes)."""
    from dau_conv import _capi
    shape = (2, 20, 40, 3, 14, 30)
    x, dy, w, mu1, mu2 = _inputs(171, shape, radius)
    extra = 0
    if what == "mu2":
        mu2[0, 3, 1, 7] = 0.25
    else:
        w[0, 5, 2, 11] = np.nan
        extra = _capi.FLAG_DENSE_SPLIT_LINE
    on, off = _plan(shape, radius, extra=extra), _plan(shape, radius, on=False, extra=extra)
    got, st = _run(on, x, dy, w, mu1, mu2)
    ref, rst = _run(off, x, dy, w, mu1, mu2)
    assert st == (1, 0), st
    assert rst == (0, 0)                                      # (a plan without a line member does not count)
    if extra:
        assert on.line_status() == (1, 0) and off.line_status() == (1, 0)
    _same(got, ref)
    assert np.isnan(got["dsigma"]).any() == (what == "nan_weight")
    # ... and the next on-line call takes the member again
    x, dy, w, mu1, mu2 = _inputs(171, shape, radius)
    _, st = _run(on, x, dy, w, mu1, mu2)
    assert st == (0, radius), st


@pytest.mark.parametrize("radius", [4, 8])
def test_with_the_line_gather_sum_the_statuses_stay_apart(radius):
    """DAU_FLAG_DENSE_SPLIT_LINE beside the new flag: both passes take their line member, each reports its own; dx is the bits of
    the plan without the new flag."""
    from dau_conv import _capi
    shape = (2, 20, 40, 3, 14, 30)
    x, dy, w, mu1, mu2 = _inputs(173, shape, radius)
    both = _plan(shape, radius, extra=_capi.FLAG_DENSE_SPLIT_LINE)
    got, st = _run(both, x, dy, w, mu1, mu2)
    assert st == (0, radius) and both.line_status() == (0, radius)
    ref, _ = _run(_plan(shape, radius, on=False, extra=_capi.FLAG_DENSE_SPLIT_LINE), x, dy, w, mu1, mu2)
    _same(got, ref, ("dx",))
    alone, _ = _run(_plan(shape, radius), x, dy, w, mu1, mu2)
    _same(got, alone, PARAMS)


IO = (2, 20, 40, 3, 14, 30)


@pytest.mark.parametrize("radius", [4, 8])
@pytest.mark.parametrize("io", ["f16", "bf16"])
def test_16_bit_io_is_the_float32_plan_on_the_widened_tensors(io, radius):
    from dau_conv import _capi
    dt, flag = (torch.float16, _capi.FLAG_IO_F16) if io == "f16" else (torch.bfloat16, _capi.FLAG_IO_BF16)
    x, dy, w, mu1, mu2 = _inputs(181, IO, radius)
    xw, dyw = (torch.from_numpy(a).to(dt).float().numpy() for a in (x, dy))
    got, st = _run(_plan(IO, radius, extra=flag), xw, dyw, w, mu1, mu2, dt)
    ref, _ = _run(_plan(IO, radius), xw, dyw, w, mu1, mu2)
    assert st == (0, radius), st
    _same(got, ref, PARAMS)


@pytest.mark.parametrize("radius", [4, 8])
@pytest.mark.parametrize("io", ["f32", "bf16"])
def test_nhwc_is_the_nchw_call_on_the_permuted_tensors(io, radius):
    from dau_conv import _capi
    dt, flag = dict(f32=(torch.float32, 0), bf16=(torch.bfloat16, _capi.FLAG_IO_BF16))[io]
    x, dy, w, mu1, mu2 = _inputs(183, IO, radius)
    got, st = _run(_plan(IO, radius, extra=flag | _capi.FLAG_IO_NHWC), x, dy, w, mu1, mu2, dt, nhwc=True)
    ref, _ = _run(_plan(IO, radius, extra=flag), x, dy, w, mu1, mu2, dt)
    assert st == (0, radius), st
    _same(got, ref, PARAMS)


@pytest.mark.parametrize("radius", [4, 8])
def test_input_relu(radius):
    """DAU_FLAG_INPUT_RELU, bit for bit: the plan without it on the clamped x."""
    from dau_conv import _capi
    x, dy, w, mu1, mu2 = _inputs(187, IO, radius)
    x = (x - 0.5).astype(np.float32)
    got, st = _run(_plan(IO, radius, extra=_capi.FLAG_INPUT_RELU), x, dy, w, mu1, mu2)
    ref, _ = _run(_plan(IO, radius), np.maximum(x, 0).astype(np.float32), dy, w, mu1, mu2)
    assert st == (0, radius), st
    _same(got, ref, PARAMS)


@pytest.mark.parametrize("radius", [4, 8])
def test_data_parallel_path(radius):
    """backward_param_sums + finalize_param_grads give the bits of backward"""
    x, dy, w, mu1, mu2 = _inputs(189, IO, radius)
    plan = _plan(IO, radius)
    ref, st = _run(plan, x, dy, w, mu1, mu2)
    assert st == (0, radius), st
    S, G, F = w.shape[1:]
    sg = torch.full((1, S, G, F), 0.5, device="cuda")
    sums = plan.backward_param_sums(_dev(x), _dev(dy), _dev(mu1), _dev(mu2), sg)
    assert plan.dot_line_status() == (0, radius)
    got = plan.finalize_param_grads(sums, _dev(w))
    for key, v in zip(PARAMS, got):
        assert np.array_equal(v.cpu().numpy(), ref[key]), key


@pytest.mark.parametrize("io,nhwc", [("f32", False), ("bf16", True)])
@pytest.mark.parametrize("radius", [4, 8])
def test_memory_contract(radius, io, nhwc):
    """Through the arena of tests/abi_arena.py: canaries clean, a workspace of exactly dau_conv_workspace_bytes, poisoned scratch,
    activation bases one element off."""
    from dau_conv import _capi
    shape = (2, 20, 40, 3, 13, 27)
    x, dy, w, mu1, mu2 = _inputs(191, shape, radius)
    S, G, F = w.shape[1:]
    # (the arena stores the activations' bytes as they come: an NHWC plan gets [N][H][W][C] arrays)
    lay = (lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1))) if nhwc else (lambda a: a)
    inputs = dict(x=lay(x), dy=lay(dy), w=w, mu1=mu1, mu2=mu2, sigma=np.full((1, S, G, F), 0.5, np.float32))
    plan = _plan(shape, radius, extra=(_capi.FLAG_IO_BF16 if io == "bf16" else 0) | (_capi.FLAG_IO_NHWC if nhwc else 0))
    rep = abi_arena.backward(_capi, plan, inputs, io=io, skew=1, fill=0xFF)
    assert rep.rc == _capi.DAU_OK and rep.status_rc == _capi.DAU_OK
    rep.assert_clean("linedot/r%d/%s" % (radius, io))
    for name, v in rep.values.items():
        assert np.isfinite(v).all(), name
    xs, dys = (abi_arena.widen(abi_arena.to_storage(a, io), io) for a in (x, dy))
    ref, st = _run(plan, xs, dys, w, mu1, mu2, torch.bfloat16 if io == "bf16" else torch.float32, nhwc=nhwc)
    assert st == (0, radius), st
    for key in PARAMS:
        assert np.array_equal(rep.values[key], ref[key]), key


@pytest.mark.parametrize("radius", [4, 8])
def test_at_baseline_depth(radius):
    """real reduction depth, a DEFAULT plan with the flag; the oracle on a slice of eight output channels"""
    shape = (8, 256, 256, 4, 56, 56)
    x, dy, w, mu1, mu2 = _inputs(2025, shape, radius)
    plan = _plan(shape, radius, forced=False)
    got, st = _run(plan, x, dy, w, mu1, mu2, need=30)
    assert st == (0, radius), st
    fs = slice(0, 8)
    want = _oracle(("depth", radius), x, dy[:, fs], w[..., fs], mu1[..., fs], mu2[..., fs])
    _check({k: got[k][..., fs] for k in PARAMS}, want, "linedot/depth/r%d" % radius)


def test_layer():
    """DAUConv1d(dense_line=True, dense_line_grads=True): the plan-level member runs; against the layer without the new keyword
    inside the bar; torch.compile(fullgraph=True) gives eager's bits."""
    import importlib
    import dau_conv
    dc = importlib.import_module("dau_conv.dau_conv")
    dc._PLANS.clear()
    torch.manual_seed(5)

    def make(flag):
        return dau_conv.DAUConv1d(filters=16, dau_units=(2, 1), max_kernel_size=9, in_channels=8, dense_line=True, dense_line_grads=flag,
                                  dense_split=True, mu1_initializer=dau_conv.random_uniform_initializer(-3.9, 3.9)).cuda()
    on, off = make(True), make(False)
    off.load_state_dict(on.state_dict())
    x = torch.rand(2, 8, 5, 24, device="cuda")
    dy = torch.randn(2, 16, 5, 24, device="cuda")

    def step(layer, fn=None):
        layer.zero_grad()
        xi = x.clone().requires_grad_(True)
        y = (layer if fn is None else fn)(xi)
        y.backward(dy)
        return [y.detach(), xi.grad] + [p.grad.clone() for p in layer.parameters() if p.grad is not None]
    got = step(on)
    plans = [p for p in dc._PLANS.values() if p.info["gather_dense_split"] & (1 << 8)]
    assert len(plans) == 1
    assert plans[0].dot_line_status() == (0, 4) and plans[0].line_status() == (0, 4)
    ref = step(off)
    assert len(got) == len(ref) >= 5
    for i, (a, b) in enumerate(zip(got, ref)):
        assert_parity(a.cpu().numpy(), b.cpu().numpy(), "layer/%d" % i)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])       # y and dx: the same members either way
    compiled = torch.compile(on, fullgraph=True, backend="aot_eager")
    again = step(on, compiled)
    assert plans[0].dot_line_status() == (0, 4)
    for i, (a, b) in enumerate(zip(again, got)):
        assert torch.equal(a, b), i
    dau_conv.check_pending_offsets()
