"""GPU: the opt-in line members of the two-limb gather-sum (DAU_FLAG_DENSE_SPLIT_LINE, with DAU_FLAG_SINGLE_DIM_KERNEL).  A call whose
units all lie on the row of their pixel (mu2 == 0) runs its y and dx passes as the two-limb f16 GEMM of k_dense_split.hip over ONE
row of taps -- 1 x 9 for offsets within +-4 (namespace l4), 1 x 17 within (4, 8] (l8) -- instead of the 9 x 9 kernel or the exact
gather.  Bar: the fp32 one against the oracle with single_dim_kernel=True (util.assert_parity defaults: 1e-4 relative + 1e-6 of the
max-norm) -- the form claims fp32 accuracy, so it gets no bar of its own; margins are recorded with util.record_margins.
dau_conv_gather_line_status proves which member a call took.  Replaces the same reference code as the exact gather
(dau_conv_forward_core.hpp:804-1605), for the layers of the reference's test_DAUConv1d."""
import numpy as np
import pytest
import torch

import abi_arena
from oracle import dau_oracle as orc
from util import assert_parity, make_inputs, record_margins, tuning_capi

pytestmark = pytest.mark.gpu

BAR = "1e-4 rel + 1e-6 max-norm (fp32 bar; two-limb line member)"
KEYS = ("y", "dx", "dw", "dmu1", "dmu2", "dsigma")
GRADS = KEYS[2:]
K = {4: 9, 8: 17}                 # max_kernel_size whose clip is the member's radius
M = {4: 3.99, 8: 7.99}


def _flags(capi, line=True, forced=True, extra=0):
    return (capi.FLAG_USE_INTERPOLATION | capi.FLAG_SINGLE_DIM_KERNEL | (capi.FLAG_DENSE_SPLIT_F16 if forced else 0) |
            (capi.FLAG_DENSE_SPLIT_LINE if line else 0) | extra)


def _plan(shape, radius, line=True, forced=True, extra=0, capi=None, **kw):
    if capi is None:
        from dau_conv import _capi as capi
    N, S, F, G, H, W = (shape[q] for q in ("N", "S", "F", "G", "H", "W"))
    plan = capi.Plan(N, S, F, G, H, W, max_kernel_size=K[radius], sigma_hint=0.5, flags=_flags(capi, line, forced, extra), **kw)
    if forced:
        assert plan.info["gather_dense_split"] == 0b11100 | ((0b01000000 if radius == 4 else 0b11000000) if line else 0)
    return plan


def _inputs(seed, shape, radius):
    """make_inputs with the units on the line; the two ends of the member's row of taps are used"""
    N, S, F, G, H, W = (shape[q] for q in ("N", "S", "F", "G", "H", "W"))
    x, dy, w, mu1, mu2 = make_inputs(seed, N, S, F, G, H, W, K[radius], M[radius])
    mu2[:] = 0
    mu1.flat[0] = M[radius]; mu1.flat[1] = -M[radius]
    assert np.abs(mu1).max() > radius - 4 and np.abs(mu1).max() <= radius
    return x, dy, w, mu1, mu2


def _run(plan, x, dy, w, mu1, mu2, dtype=torch.float32, nhwc=False):
    """forward + backward -> (tensors as numpy fp32, y and dx also raw; line status after the forward call, after the backward call)"""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    S, G, F = w.shape[1:]
    sg = torch.full((1, S, G, F), 0.5, device="cuda")
    xd, dyd = dev(x).to(dtype), dev(dy).to(dtype)
    if nhwc:
        xd, dyd = (t.contiguous(memory_format=torch.channels_last) for t in (xd, dyd))
    wd, m1, m2 = dev(w), dev(mu1), dev(mu2)
    y = plan.forward(xd, wd, m1, m2, sg)
    plan.check_status()
    st_f = plan.line_status()
    g = plan.backward(xd, dyd, wd, m1, m2, sg)
    plan.check_status()
    st_b = plan.line_status()
    torch.cuda.synchronize()
    out = dict(y=y.float().cpu().numpy(), dx=g[0].float().cpu().numpy(), dw=g[1].cpu().numpy(), dmu1=g[2].cpu().numpy(),
               dmu2=g[3].cpu().numpy(), dsigma=g[4].cpu().numpy())
    out["raw"] = dict(y=y.cpu(), dx=g[0].cpu())
    return out, st_f, st_b


_ORACLE = {}


def _oracle(key, x, dy, w, mu1, mu2):
    """computed once per key, shared by the tests that need it, never written"""
    if key not in _ORACLE:
        want = orc.backward(x, dy, w, mu1, mu2, 0.5, single_dim_kernel=True)
        want["y"] = orc.forward(x, w, mu1, mu2, 0.5, single_dim_kernel=True)
        for a in want.values():
            a.setflags(write=False)
        _ORACLE[key] = want
    return _ORACLE[key]


def _check(got, want, name):
    m = record_margins(name, {k: got[k] for k in KEYS}, want, BAR)
    print(name, "margins", {k: "%.2e" % v for k, v in m.items()})
    for key in KEYS:
        assert_parity(got[key], want[key], name + "/" + key)


def _same(a, b, keys=KEYS):
    for key in keys:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


# the tile-geometry shapes of test_gpu_dense_split.py::test_split_gather_against_oracle, and a sequence
SHAPES = [
    dict(N=2, S=16, F=128, G=4, H=56, W=56),      # column blocks of four and of three tiles, whole chunks and channel blocks
    dict(N=3, S=20, F=40, G=3, H=30, W=45),       # ragged everything: channels, rows, columns, odd batch; blocks of 3 + 3
    dict(N=2, S=7, F=5, G=2, H=9, W=6),           # tiny: one block of one tile
    dict(N=2, S=33, F=130, G=6, H=28, W=28),      # two channel blocks, the second almost empty
    dict(N=1, S=16, F=16, G=2, H=20, W=130),      # seventeen tiles
    dict(N=2, S=32, F=64, G=1, H=17, W=64),       # two blocks of four
    dict(N=4, S=24, F=32, G=5, H=14, W=14),       # one block of two
    dict(N=2, S=8, F=8, G=4, H=27, W=27),         # odd width: the staging kernel's scalar loads
    dict(N=3, S=16, F=16, G=2, H=1, W=40),        # a sequence: one live row in an eight-row block
]
_id = lambda s: "S%d_F%d_G%d_%dx%d" % tuple(s[q] for q in "SFGHW")


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
@pytest.mark.parametrize("radius", [4, 8])
def test_line_member_against_oracle(shape, radius):
    x, dy, w, mu1, mu2 = _inputs(43 + radius, shape, radius)
    if radius == 8:
        assert np.abs(mu1).max() > 4
    got, st_f, st_b = _run(_plan(shape, radius), x, dy, w, mu1, mu2)
    _check(got, _oracle(("parity", _id(shape), radius), x, dy, w, mu1, mu2), "line/r%d/%s" % (radius, _id(shape)))
    assert st_f == (0, radius) and st_b == (0, radius), (st_f, st_b)
    assert not got["dmu2"].any()


@pytest.mark.parametrize("radius", [4, 8])
def test_integer_offsets_and_the_exact_radius(radius):
    """Fraction 0: the tap at +1 carries weight 0 -- for an offset of exactly +R it lies outside the row of taps."""
    shape = dict(N=2, S=20, F=40, G=3, H=12, W=30)
    x, dy, w, mu1, mu2 = _inputs(61, shape, radius)
    rs = np.random.RandomState(62)
    mu1[:] = rs.randint(-radius, radius + 1, mu1.shape).astype(np.float32)
    mu1.flat[0] = radius; mu1.flat[1] = -radius; mu1.flat[2] = radius - 0.5
    got, st_f, st_b = _run(_plan(shape, radius), x, dy, w, mu1, mu2)
    assert st_f == (0, radius) and st_b == (0, radius), (st_f, st_b)
    _check(got, _oracle(("integer", radius), x, dy, w, mu1, mu2), "line/integer/r%d" % radius)


@pytest.mark.parametrize("shape", [dict(N=2, S=16, F=130, G=4, H=28, W=28), dict(N=2, S=8, F=8, G=4, H=9, W=27)], ids=_id)
@pytest.mark.parametrize("radius", [4, 8])
def test_block_of_four_rows(shape, radius, monkeypatch):
    """split_gather_kernel<NSUB, RG = 1> of the line forms, forced by the tuning build: the oracle's values, and the bits of the
    eight-row form (the same sums in the same order)."""
    capi = tuning_capi()
    x, dy, w, mu1, mu2 = _inputs(143 + radius, shape, radius)
    monkeypatch.setenv("DAU_SPLIT_TALL", "0")
    monkeypatch.setenv("DAU_SPLIT_ROWS4", "2")
    got, st_f, st_b = _run(_plan(shape, radius, capi=capi), x, dy, w, mu1, mu2)
    assert st_f == (0, radius) and st_b == (0, radius)
    _check(got, _oracle(("rows4", _id(shape), radius), x, dy, w, mu1, mu2), "line/rows4/r%d/%s" % (radius, _id(shape)))
    monkeypatch.setenv("DAU_SPLIT_ROWS4", "0")
    ref, _, _ = _run(_plan(shape, radius, capi=capi), x, dy, w, mu1, mu2)
    _same(got, ref, ("y", "dx"))


@pytest.mark.parametrize("shape", [dict(N=2, S=16, F=16, G=4, H=28, W=28), dict(N=2, S=24, F=8, G=3, H=11, W=17)], ids=_id)
@pytest.mark.parametrize("radius", [4, 8])
def test_tall_tiles(shape, radius, monkeypatch):
    """split_gather_kernel<NSUB, 2, TT = true> of the line forms (7 and 5 tiles of four columns), forced by the tuning build."""
    capi = tuning_capi()
    x, dy, w, mu1, mu2 = _inputs(151 + radius, shape, radius)
    monkeypatch.setenv("DAU_SPLIT_TALL", "2")
    monkeypatch.setenv("DAU_SPLIT_ROWS4", "2")
    got, st_f, st_b = _run(_plan(shape, radius, capi=capi), x, dy, w, mu1, mu2)
    assert st_f == (0, radius) and st_b == (0, radius)
    _check(got, _oracle(("tall", _id(shape), radius), x, dy, w, mu1, mu2), "line/tall/r%d/%s" % (radius, _id(shape)))
    monkeypatch.setenv("DAU_SPLIT_TALL", "0")
    monkeypatch.setenv("DAU_SPLIT_ROWS4", "0")
    ref, _, _ = _run(_plan(shape, radius, capi=capi), x, dy, w, mu1, mu2)
    _same(got, ref, ("y", "dx"))


@pytest.mark.parametrize("radius", [4, 8])
def test_depth_256_channels(radius):
    """S = F = 256: sixteen chunks of accumulation behind every output, through the members a caller gets by DEFAULT (not forced).
    This is where a chain through one accumulator goes wrong (k_dense_split.hip, header)."""
    shape = dict(N=1, S=256, F=256, G=4, H=8, W=16)
    x, dy, w, mu1, mu2 = _inputs(31, shape, radius)
    plan = _plan(shape, radius, forced=False)
    assert plan.info["gather_dense_split"] >> 6 == (1 if radius == 4 else 3), bin(plan.info["gather_dense_split"])
    got, st_f, st_b = _run(plan, x, dy, w, mu1, mu2)
    assert st_f == (0, radius) and st_b == (0, radius)
    _check(got, _oracle(("depth", radius), x, dy, w, mu1, mu2), "line/depth/256x256_8x16/r%d" % radius)


@pytest.mark.parametrize("radius", [4, 8])
@pytest.mark.parametrize("what", ["mu2", "nan_weight"])
def test_a_call_off_the_line_is_the_plan_without_the_flag(radius, what):
    shape = dict(N=2, S=20, F=40, G=3, H=14, W=30)
    x, dy, w, mu1, mu2 = _inputs(71, shape, radius)
    if what == "mu2":
        mu2[0, 3, 1, 7] = 0.25
    else:
        w[0, 5, 2, 11] = np.nan
    on, off = _plan(shape, radius), _plan(shape, radius, line=False)
    got, st_f, st_b = _run(on, x, dy, w, mu1, mu2)
    ref, rf, rb = _run(off, x, dy, w, mu1, mu2)
    assert st_f == (1, 0) and st_b == (1, 0), (st_f, st_b)
    assert rf == (0, 0) and rb == (0, 0)                      # (a plan without a line member does not count)
    _same(got, ref)
    assert np.isnan(got["y"]).any() == (what == "nan_weight")
    # ... and the next call decides for itself
    x, dy, w, mu1, mu2 = _inputs(71, shape, radius)
    _, st_f, st_b = _run(on, x, dy, w, mu1, mu2)
    assert st_f == (0, radius) and st_b == (0, radius)


@pytest.mark.parametrize("radius", [4, 8])
def test_parameter_gradients_are_the_flag_off_plan_s(radius):
    shape = dict(N=2, S=20, F=40, G=3, H=14, W=30)
    x, dy, w, mu1, mu2 = _inputs(73, shape, radius)
    got, st_f, st_b = _run(_plan(shape, radius), x, dy, w, mu1, mu2)
    ref, _, _ = _run(_plan(shape, radius, line=False), x, dy, w, mu1, mu2)
    assert st_f == (0, radius) and st_b == (0, radius)
    _same(got, ref, GRADS)
    assert not got["dmu2"].any()


IO = dict(N=2, S=20, F=40, G=3, H=14, W=30)


@pytest.mark.parametrize("radius", [4, 8])
@pytest.mark.parametrize("io", ["f16", "bf16"])
def test_16_bit_io_rounds_once(io, radius):
    """A float16 / bfloat16 line call = the float32 line plan on the widened tensors, rounded once."""
    from dau_conv import _capi
    dt, flag = (torch.float16, _capi.FLAG_IO_F16) if io == "f16" else (torch.bfloat16, _capi.FLAG_IO_BF16)
    x, dy, w, mu1, mu2 = _inputs(81, IO, radius)
    xw, dyw = (torch.from_numpy(a).to(dt).float().numpy() for a in (x, dy))
    got, st_f, st_b = _run(_plan(IO, radius, extra=flag), xw, dyw, w, mu1, mu2, dt)
    ref, _, _ = _run(_plan(IO, radius), xw, dyw, w, mu1, mu2)
    assert st_f == (0, radius) and st_b == (0, radius)
    assert got["raw"]["y"].dtype == dt
    for key in ("y", "dx"):
        assert torch.equal(got["raw"][key].view(torch.int16), ref["raw"][key].to(dt).view(torch.int16)), key
    _same(got, ref, GRADS)


@pytest.mark.parametrize("radius", [4, 8])
@pytest.mark.parametrize("io", ["f32", "f16", "bf16"])
def test_nhwc_is_the_nchw_call_on_the_permuted_tensors(io, radius):
    from dau_conv import _capi
    dt, flag = dict(f32=(torch.float32, 0), f16=(torch.float16, _capi.FLAG_IO_F16), bf16=(torch.bfloat16, _capi.FLAG_IO_BF16))[io]
    x, dy, w, mu1, mu2 = _inputs(83, IO, radius)
    got, st_f, st_b = _run(_plan(IO, radius, extra=flag | _capi.FLAG_IO_NHWC), x, dy, w, mu1, mu2, dt, nhwc=True)
    ref, _, _ = _run(_plan(IO, radius, extra=flag), x, dy, w, mu1, mu2, dt)
    assert st_f == (0, radius) and st_b == (0, radius)
    for key in ("y", "dx"):
        assert got["raw"][key].is_contiguous(memory_format=torch.channels_last)
        a, b = got["raw"][key].contiguous(), ref["raw"][key]
        assert torch.equal(a.view(torch.int32 if io == "f32" else torch.int16), b.view(torch.int32 if io == "f32" else torch.int16)), key
    _same(got, ref, GRADS)


@pytest.mark.parametrize("radius", [4, 8])
def test_fused_epilogue_and_residual(radius):
    """float32, bit for bit: relu((y + bias) + r) of the unfused line plan; epilogue_backward then backward = the unfused chain."""
    from dau_conv import _capi
    x, dy, w, mu1, mu2 = _inputs(85, IO, radius)
    dev = lambda a: torch.from_numpy(a).cuda()
    S, G, F = w.shape[1:]
    sg = torch.full((1, S, G, F), 0.5, device="cuda")
    xd, dyd, wd, m1, m2 = dev(x), dev(dy), dev(w), dev(mu1), dev(mu2)
    rs = np.random.RandomState(86)
    bias = dev(rs.randn(F).astype(np.float32))
    res = dev(rs.randn(IO["N"], F, IO["H"], IO["W"]).astype(np.float32))
    plan = _plan(IO, radius)
    assert plan.epilogue_supported(_capi.EPILOGUE_BIAS | _capi.EPILOGUE_RELU)
    y = plan.forward(xd, wd, m1, m2, sg)
    assert plan.line_status() == (0, radius)
    ye = plan.forward(xd, wd, m1, m2, sg, bias=bias, relu=True)
    assert plan.line_status() == (0, radius)
    assert torch.equal(ye, torch.relu(y + bias.reshape(1, -1, 1, 1)))
    yr = plan.forward(xd, wd, m1, m2, sg, bias=bias, relu=True, residual=res)
    assert plan.line_status() == (0, radius)
    want = torch.relu((y + bias.reshape(1, -1, 1, 1)) + res)
    assert torch.equal(yr, want)
    dz, dbias = plan.epilogue_backward(dyd, yr, relu=True, need_dbias=True)
    got = plan.backward(xd, dz, wd, m1, m2, sg)
    assert plan.line_status() == (0, radius)
    dz_ref = torch.where(want <= 0, torch.zeros_like(dyd), dyd)
    ref = plan.backward(xd, dz_ref, wd, m1, m2, sg)
    assert torch.equal(dz, dz_ref)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    assert_parity(dbias.cpu().numpy(), dz_ref.sum((0, 2, 3)).cpu().numpy(), "dbias")


@pytest.mark.parametrize("radius", [4, 8])
def test_input_relu(radius):
    """DAU_FLAG_INPUT_RELU, float32, bit for bit: the line plan on the clamped x, dx masked by x."""
    from dau_conv import _capi
    x, dy, w, mu1, mu2 = _inputs(87, IO, radius)
    x = (x - 0.5).astype(np.float32)
    got, st_f, st_b = _run(_plan(IO, radius, extra=_capi.FLAG_INPUT_RELU), x, dy, w, mu1, mu2)
    ref, _, _ = _run(_plan(IO, radius), np.maximum(x, 0).astype(np.float32), dy, w, mu1, mu2)
    assert st_f == (0, radius) and st_b == (0, radius)
    ref["dx"] = np.where(x <= 0, np.float32(0), ref["dx"])
    _same(got, ref)


@pytest.mark.parametrize("radius", [4, 8])
def test_images_are_independent(radius, monkeypatch):
    """Image 1 of a batch of three -- one batch-mate scaled by 2^20, one holding an Inf -- gives the bits it gives alone; a pass cut
    into batch slabs gives the bits of the whole-batch pass (the library cuts even slabs of at least two images, so that part runs
    on four images: two slabs of two)."""
    shape = dict(N=3, S=16, F=16, G=2, H=16, W=24)
    x, dy, w, mu1, mu2 = _inputs(89, shape, radius)
    whole, st_f, st_b = _run(_plan(shape, radius), x, dy, w, mu1, mu2)
    assert st_f == (0, radius) and st_b == (0, radius)
    xb, dyb = x.copy(), dy.copy()
    xb[0] *= np.float32(2.0 ** 20); dyb[0] *= np.float32(2.0 ** 20)
    xb[2, 3, 5, 7] = np.inf; dyb[2, 1, 2, 3] = np.inf
    mates, _, _ = _run(_plan(shape, radius), xb, dyb, w, mu1, mu2)
    alone, _, _ = _run(_plan(dict(shape, N=1), radius), x[1:2], dy[1:2], w, mu1, mu2)
    for key in ("y", "dx"):
        assert np.array_equal(mates[key][1], whole[key][1]) and np.array_equal(alone[key][0], whole[key][1]), key
    shape = dict(shape, N=4)
    x, dy, w, mu1, mu2 = _inputs(90, shape, radius)
    x[:2] *= np.float32(2.0 ** -20); dy[:2] *= np.float32(2.0 ** -20)     # the first slab far below the second
    whole, _, _ = _run(_plan(shape, radius), x, dy, w, mu1, mu2)
    monkeypatch.setenv("DAU_WORKSPACE_BUDGET_GB", "0.0000005")
    slabbed = _plan(shape, radius)
    monkeypatch.delenv("DAU_WORKSPACE_BUDGET_GB")
    assert slabbed.info["batch_slab_gather"] == 2, slabbed.info
    got, st_f, st_b = _run(slabbed, x, dy, w, mu1, mu2)
    assert st_f == (0, radius) and st_b == (0, radius)
    _same(got, whole, ("y", "dx"))


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("io", ["f32", "bf16"])
@pytest.mark.parametrize("radius", [4, 8])
def test_memory_contract(radius, io, skew):
    """Through the arena of tests/abi_arena.py: canaries clean, a workspace of exactly dau_conv_workspace_bytes."""
    from dau_conv import _capi
    shape = dict(N=2, S=20, F=40, G=3, H=13, W=27)
    x, dy, w, mu1, mu2 = _inputs(91, shape, radius)
    S, G, F = w.shape[1:]
    inputs = dict(x=x, dy=dy, w=w, mu1=mu1, mu2=mu2, sigma=np.full((1, S, G, F), 0.5, np.float32))
    plan = _plan(shape, radius, extra=_capi.FLAG_IO_BF16 if io == "bf16" else 0)

    for call in (abi_arena.forward, abi_arena.backward):
        rep = call(_capi, plan, inputs, io=io, skew=skew, fill=0xFF)
        assert rep.rc == _capi.DAU_OK and rep.status_rc == _capi.DAU_OK
        rep.assert_clean("line/r%d/%s/skew%d" % (radius, io, skew))
        for name, v in rep.values.items():
            assert np.isfinite(v).all(), name
    # the values are the plan's own through the package's workspace
    xs, dys = (abi_arena.widen(abi_arena.to_storage(a, io), io) for a in (x, dy))
    ref, st_f, st_b = _run(plan, xs, dys, w, mu1, mu2, torch.bfloat16 if io == "bf16" else torch.float32)
    assert st_f == (0, radius) and st_b == (0, radius)
    rep = abi_arena.backward(_capi, plan, inputs, io=io, skew=skew, fill=0x7B)
    for key in ("dx",) + GRADS:
        assert np.array_equal(rep.values[key], ref[key]), key


def test_layer():
    """DAUConv1d(dense_line=True) against the same layer without the keyword, eager and under torch.compile(fullgraph=True).
    dense_split=True on both: at 8 -> 16 channels on 5 x 24 pixels no two-limb member pays by the cost model, so a default plan of
    this size holds none (tests/test_line_plan.py has the default plans of the sizes where they pay)."""
    import importlib
    import dau_conv
    dc = importlib.import_module("dau_conv.dau_conv")
    dc._PLANS.clear()
    torch.manual_seed(5)

    def make(flag):
        return dau_conv.DAUConv1d(filters=16, dau_units=(2, 1), max_kernel_size=9, in_channels=8, dense_line=flag, dense_split=True,
                                  mu1_initializer=dau_conv.random_uniform_initializer(-3.9, 3.9)).cuda()
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
    plans = [p for p in dc._PLANS.values() if p.info["gather_dense_split"] & (1 << 6)]
    assert len(plans) == 1
    assert plans[0].line_status() == (0, 4)                # (asked before another plan's call overwrites the shared workspace)
    ref = step(off)
    assert len(got) == len(ref) >= 5
    for i, (a, b) in enumerate(zip(got, ref)):
        assert_parity(a.cpu().numpy(), b.cpu().numpy(), "layer/%d" % i)
    compiled = torch.compile(on, fullgraph=True, backend="aot_eager")      # (as tests/test_gpu_compile.py: torch's own ops stay eager's)
    again = step(on, compiled)
    assert plans[0].line_status() == (0, 4)
    for i, (a, b) in enumerate(zip(again, got)):
        assert torch.equal(a, b), i
    dau_conv.check_pending_offsets()
    dc._PLANS.clear()
