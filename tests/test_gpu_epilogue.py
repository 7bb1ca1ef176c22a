"""GPU: the fused epilogue at the plan level.  dau_conv_forward_epilogue stores y = act(sum + bias[f]) -- one fp32 add and a clamp on
the very value dau_conv_forward stores, before the store's one rounding -- so for float32 the bar is identity with
relu(forward(x) + bias), for the 16-bit formats identity with the rounded float32 fused result, and for NHWC identity with the NCHW
call.  dau_conv_epilogue_backward: dz is aten::threshold_backward bit for bit; dbias is a hierarchical fp32 sum in which no value
passes through more than 256 additions, hence |dbias[f] - exact| <= 256 * 2^-24 * sum |dz[:, f]| = 2^-16 * sum |dz[:, f]|.
The rows are member_rows.FUSED_ROWS; each proves through Plan.info / outlier_status that its member runs."""
import ctypes

import numpy as np
import pytest
import torch

import abi_arena as aa
import member_rows as mr
from member_rows import I, IO, OUTLIERS, act as _act, inputs as _inputs, io_of as _io_of, nhwc as _nhwc, params as _params, plan as _plan
from util import assert_parity, bits as _bits

pytestmark = pytest.mark.gpu

BIAS, RELU = 1, 2
EPILOGUES = (BIAS, BIAS | RELU, RELU)
ROWS = mr.FUSED_ROWS

_SHARED = {}        # name -> (x fp32 on the device, unfused fp32 y, bias): computed once, never written


def _shared(name):
    if name not in _SHARED:
        x = torch.from_numpy(_inputs(name)[0]).cuda()
        plan = _plan(name, "f32")
        y = plan.forward(x, *_params(name))
        plan.check_status()
        # randn(F) at the size of y: about half of the outputs end up negative, so ReLU cuts them
        F = y.shape[1]
        bias = (torch.from_numpy(np.random.RandomState(7).randn(F).astype(np.float32)).cuda() * y.std()).contiguous()
        _SHARED[name] = (x, y, bias)
    return _SHARED[name]


def _fused(plan, name, x, epilogue):
    """the fused forward on a plan of its own with `plan`'s flags: a plan's first call has no offset-bucket hint and runs the kernels
    of its static bucket, as the call that made the shared unfused y did -- a later call of a kernel-65 plan would run the set of the
    bucket its offsets need, one window pass instead of four, whose sums come in another order"""
    _, _, bias = _shared(name)
    plan = _plan(name, _io_of(plan), plan.io_layout == "NHWC")
    y = plan.forward(x, *_params(name), bias=bias if epilogue & BIAS else None, relu=bool(epilogue & RELU))
    plan.check_status()
    if mr.ROWS[name][0] & OUTLIERS:
        assert plan.outlier_status() == (1, True), "the radius-3 + ring member did not run"
    return y


def _unfused(y, bias, epilogue):
    out = y + bias.view(1, -1, 1, 1) if epilogue & BIAS else y
    return torch.relu(out) if epilogue & RELU else out


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", list(ROWS))
def test_fp32_fused_is_the_unfused_result(name, nhwc):
    """identity, not a tolerance: both forms perform the same single fp32 add (a contracted FMA in any member fails this)"""
    x, y, bias = _shared(name)
    plan = _plan(name, "f32", nhwc)
    xin = _act(x, torch.float32, plan)
    for e in EPILOGUES:
        got = _fused(plan, name, xin, e)
        assert got.dtype == torch.float32 and got.is_contiguous(memory_format=torch.channels_last if nhwc else torch.contiguous_format)
        want = _unfused(y, bias, e)
        if e & RELU:
            cut = float((want == 0).float().mean())
            assert 0.2 < cut < 0.8, "ReLU cuts %.2f of the outputs: the bias is not at the size of y" % cut
        assert torch.equal(got.contiguous(), want), "epilogue %d: %d of %d values differ" % (e, int((got != want).sum()), want.numel())


@pytest.mark.parametrize("io", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(ROWS))
def test_16bit_fused_is_the_rounded_fp32_fused_result_in_both_layouts(name, io):
    """one rounding: the 16-bit plan stores the rounding of what the fp32 plan computes from the widened input (the invariant
    test_gpu_f16.py holds for the unfused store), and the NHWC plan stores the bits of the NCHW plan"""
    x, _, _ = _shared(name)
    dtype = IO[io][1]
    p16, p16n, p32 = _plan(name, io), _plan(name, io, True), _plan(name, "f32")
    x16 = x.to(dtype)
    windows = p16.info["gather_windows"]
    for e in EPILOGUES:
        got = _fused(p16, name, x16, e)
        got_nhwc = _fused(p16n, name, _act(x16, dtype, p16n), e)
        assert got.dtype == dtype and got_nhwc.dtype == dtype and got_nhwc.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(_bits(got_nhwc), _bits(got)), "epilogue %d: NHWC differs from NCHW" % e
        ref = _fused(p32, name, x16.float(), e)
        if windows == 1:
            assert torch.equal(_bits(got), _bits(ref.to(dtype))), "epilogue %d: %d values differ" % (
                e, int((_bits(got) != _bits(ref.to(dtype))).sum()))
        elif io == "f16":
            # every window pass re-reads the stored value, adds and rounds again: test_gpu_f16.py's bar for windowed plans
            assert_parity(got.float().cpu().numpy(), ref.cpu().numpy(), "y", rel=2e-3, floor=1e-3)
        else:
            # bfloat16: test_gpu_bf16.py's bar for the same kernel-65, four-window plan (the fused store adds no rounding to it)
            assert_parity(got.float().cpu().numpy(), ref.cpu().numpy(), "y", rel=2e-2, floor=4e-3)


def test_nhwc_fp32_fused_is_the_nchw_fused():
    for name in ("split_17x13_m3", "outliers_28x28", "k65_gather_windows"):
        x, _, _ = _shared(name)
        a, b = _plan(name, "f32"), _plan(name, "f32", True)
        for e in EPILOGUES:
            assert torch.equal(_bits(_fused(b, name, _act(x, torch.float32, b), e)), _bits(_fused(a, name, x, e))), (name, e)


# ---- epilogue_backward ------------------------------------------------------------------------------------------------------------
GRAD_SHAPES = {
    "f5_17x13": (2, 5, 17, 13),          # nothing divides: element access in both layouts
    "f40_28x28": (2, 40, 28, 28),        # 16-byte access in both layouts
    "f20_37x100": (3, 20, 37, 100),      # several images per workgroup (NCHW), a part-filled pixel block (NHWC)
}


def _grad_plan(shape, io, nhwc):
    from dau_conv import _capi
    N, F, H, W = shape
    return _capi.Plan(N, 2, F, 1, H, W, flags=I | IO[io][0] | (_capi.FLAG_IO_NHWC if nhwc else 0))


def _grad_inputs(shape, dtype, plan, seed=3):
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(shape, generator=g).cuda()
    y = torch.relu(torch.randn(shape, generator=g)).cuda()
    return _act(dy, dtype, plan), _act(y, dtype, plan)


def _check_dbias(dbias, dz, tag):
    exact = dz.double().sum(dim=(0, 2, 3))
    bound = 2.0 ** -16 * dz.double().abs().sum(dim=(0, 2, 3))
    err = (dbias.double() - exact).abs()
    print("%s: max |dbias - exact| / bound = %.3g" % (tag, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), "%s: |dbias - exact| %s exceeds 2^-16 * sum|dz| %s" % (tag, err.tolist(), bound.tolist())


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("io", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", list(GRAD_SHAPES))
def test_epilogue_backward(shape, io, nhwc):
    plan = _grad_plan(GRAD_SHAPES[shape], io, nhwc)
    dtype = IO[io][1]
    dy, y = _grad_inputs(GRAD_SHAPES[shape], dtype, plan)
    want = torch.ops.aten.threshold_backward(dy, y, 0)
    dz, dbias = plan.epilogue_backward(dy, y, relu=True)
    assert dz.dtype == dtype and dz.stride() == dy.stride() and dbias.dtype == torch.float32
    assert torch.equal(_bits(dz), _bits(want)), "dz"
    _check_dbias(dbias, dz, "%s %s %s" % (shape, io, "nhwc" if nhwc else "nchw"))
    dz2, dbias2 = plan.epilogue_backward(dy, y, relu=True)
    assert torch.equal(dbias2.view(torch.int32), dbias.view(torch.int32)) and torch.equal(_bits(dz2), _bits(dz)), "two calls differ"
    # dz only; dz written over dy
    dz3, none = plan.epilogue_backward(dy, y, relu=True, need_dbias=False)
    assert none is None and torch.equal(_bits(dz3), _bits(want))
    alias = dy.clone(memory_format=torch.preserve_format)
    dz4, dbias4 = plan.epilogue_backward(alias, y, relu=True, dz=alias)
    assert dz4 is alias and torch.equal(_bits(alias), _bits(want)) and torch.equal(dbias4.view(torch.int32), dbias.view(torch.int32))
    # without ReLU dz IS dy: nothing is written, the sum runs over dy
    before = dy.clone(memory_format=torch.preserve_format)
    nodz, dbias5 = plan.epilogue_backward(dy, relu=False)
    assert nodz is None and torch.equal(_bits(dy), _bits(before))
    _check_dbias(dbias5, dy, "%s %s no relu" % (shape, io))
    assert plan.epilogue_backward(dy, relu=False, need_dbias=False) == (None, None)


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw_plane_chunks", "nhwc_two_levels"])
def test_epilogue_backward_long_planes_and_two_reduction_levels(nhwc):
    """planes of more than 16384 elements are cut into chunks (NCHW); 255 channels leave one pixel row per workgroup in the
    element-wise NHWC form, 4112 partial sums per channel: more than one level of 4096 reduces"""
    shape = (4, 255, 256, 257)
    plan = _grad_plan(shape, "f16", nhwc)
    g = torch.Generator(device="cuda").manual_seed(5)
    fmt = torch.channels_last if nhwc else torch.contiguous_format
    dy = torch.randn(shape, generator=g, device="cuda", dtype=torch.float16).contiguous(memory_format=fmt)
    y = torch.relu(torch.randn(shape, generator=g, device="cuda", dtype=torch.float16)).contiguous(memory_format=fmt)
    dz, dbias = plan.epilogue_backward(dy, y, relu=True)
    assert torch.equal(_bits(dz), _bits(torch.ops.aten.threshold_backward(dy, y, 0)))
    _check_dbias(dbias, dz, "long planes nhwc=%s" % nhwc)
    assert torch.equal(plan.epilogue_backward(dy, y, relu=True)[1].view(torch.int32), dbias.view(torch.int32))


@pytest.mark.parametrize("io", ["f32", "f16"])
def test_epilogue_backward_with_values_that_are_not_finite(io):
    shape = GRAD_SHAPES["f40_28x28"]
    plan = _grad_plan(shape, io, False)
    dy, y = _grad_inputs(shape, IO[io][1], plan)
    y[0, 3, 4, 5] = float("nan")          # a NaN y passes dy through
    y[1, 7, 0, 0] = -0.0                  # -0 <= 0: cut
    dy[1, 7, 0, 0] = 2.5
    dz, dbias = plan.epilogue_backward(dy, y, relu=True)
    assert torch.equal(_bits(dz), _bits(torch.ops.aten.threshold_backward(dy, y, 0)))
    assert dz[0, 3, 4, 5] == dy[0, 3, 4, 5] and dz[1, 7, 0, 0] == 0 and torch.isfinite(dbias).all()
    y2 = torch.ones_like(y)
    dy[0, 11, 2, 2] = float("inf")
    _, dbias = plan.epilogue_backward(dy, y2, relu=True)
    finite = torch.isfinite(dbias)
    assert not finite[11] and int(finite.sum()) == shape[1] - 1, "an Inf in dy reaches other channels' dbias"


# ---- memory: outputs and workspace as slices of poisoned allocations, aligned and one element off -----------------------------------
@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("io", ["f32", "f16"])
def test_memory_contract_of_the_fused_forward(io, nhwc, skew):
    from dau_conv import _capi
    name = "split_tall_28x28"
    plan = _plan(name, io, nhwc)
    x, dy, w, mu1, mu2 = _inputs(name)
    S, G, F = w.shape[1:]
    inputs = dict(w=w, mu1=mu1, mu2=mu2, sigma=np.full((1, S, G, F), 0.5, np.float32), x=_nhwc(x) if nhwc else x, dy=_nhwc(dy) if nhwc else dy)
    bias = _shared(name)[2]
    a = aa.Arena(_capi, plan, inputs, io, _capi.PASS_FORWARD, skew, 0x7B)
    rc = _capi.lib.dau_conv_forward_epilogue(plan._h, a.stream, a.ptr("x"), a.ptr("w"), a.ptr("mu1"), a.ptr("mu2"), a.ptr("sigma"),
                                             ctypes.c_void_p(bias.data_ptr()), BIAS | RELU, a.ptr("y"), a.ptr("workspace"), a.ws_bytes)
    rep = a.finish(rc, ("y",))
    assert rep.rc == _capi.DAU_OK and rep.status_rc == _capi.DAU_OK, _capi.lib.dau_conv_last_error()
    rep.assert_clean("fused forward %s nhwc=%s skew %d" % (io, nhwc, skew))
    assert np.isfinite(rep.values["y"]).all()
    # the same bits as the Plan call on tensors of its own
    xin = _act(torch.from_numpy(aa.widen(aa.to_storage(x, io), io)).cuda(), IO[io][1], plan)
    want = _fused(plan, name, xin, BIAS | RELU)
    got = torch.from_numpy(rep.values["y"]).cuda()
    if nhwc:
        got = got.reshape(x.shape[0], x.shape[2], x.shape[3], F).permute(0, 3, 1, 2)
    assert torch.equal(got.contiguous(), want.float().contiguous())


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("io", ["f32", "f16"])
def test_memory_contract_of_epilogue_backward(io, nhwc, skew):
    """the arena's x slot holds y, its y slot receives dz, its dw slot dbias (F floats: the rest of the slot keeps its poison)"""
    from dau_conv import _capi
    shape = GRAD_SHAPES["f40_28x28"]
    N, F, H, W = shape
    plan = _grad_plan(shape, io, nhwc)
    rs = np.random.RandomState(11)
    dy, y = rs.randn(*shape).astype(np.float32), np.maximum(rs.randn(*shape), 0).astype(np.float32)
    par = np.zeros((1, 2, 1, F), np.float32)
    inputs = dict(x=_nhwc(y) if nhwc else y, dy=_nhwc(dy) if nhwc else dy, w=par, mu1=par, mu2=par, sigma=par + 0.5)
    fill = 0x7B
    a = aa.Arena(_capi, plan, inputs, io, _capi.PASS_EPILOGUE_BACKWARD, skew, fill)
    assert a.ws_bytes == plan.workspace_bytes(_capi.PASS_EPILOGUE_BACKWARD) > 0
    rc = _capi.lib.dau_conv_epilogue_backward(plan._h, a.stream, a.ptr("dy"), a.ptr("x"), BIAS | RELU, a.ptr("y"), a.ptr("dw"),
                                              a.ptr("workspace"), a.ws_bytes)
    rep = a.finish(rc, ("y", "dw"), check_status=False)
    assert rep.rc == _capi.DAU_OK, _capi.lib.dau_conv_last_error()
    rep.assert_clean("epilogue_backward %s nhwc=%s skew %d" % (io, nhwc, skew))
    dw = rep.outputs["dw"].reshape(-1)
    assert (dw[F:].view(np.uint8) == fill).all(), "dbias was written beyond its F floats"
    dyv, yv = aa.widen(aa.to_storage(inputs["dy"], io), io), aa.widen(aa.to_storage(inputs["x"], io), io)
    dz = np.where(yv <= 0, np.float32(0), dyv)
    assert np.array_equal(rep.values["y"].reshape(dz.shape), dz)
    axes = (0, 1, 2) if nhwc else (0, 2, 3)
    exact, bound = dz.astype(np.float64).sum(axis=axes), 2.0 ** -16 * np.abs(dz.astype(np.float64)).sum(axis=axes)
    assert (np.abs(dw[:F].astype(np.float64) - exact) <= bound).all()
    # a workspace declared one byte short is refused before anything is written
    b = aa.Arena(_capi, plan, inputs, io, _capi.PASS_EPILOGUE_BACKWARD, skew, fill)
    rc = _capi.lib.dau_conv_epilogue_backward(plan._h, b.stream, b.ptr("dy"), b.ptr("x"), BIAS | RELU, b.ptr("y"), b.ptr("dw"),
                                              b.ptr("workspace"), b.ws_bytes - 1)
    short = b.finish(rc, (), check_status=False)
    assert short.rc == _capi.DAU_INVALID_ARGUMENT
    short.assert_clean("short workspace")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_plans_without_a_fused_epilogue_refuse_it():
    from dau_conv import _capi
    dev = lambda *s: torch.rand(*s, device="cuda")
    for plan, dtype in ((_capi.Plan(2, 4, 8, 2, 16, 16, algo=_capi.ALGO_DIRECT), torch.float32),
                        (_capi.Plan(2, 32, 32, 4, 16, 16, flags=I | _capi.FLAG_IO_BF16 | _capi.FLAG_DENSE_BF16), torch.bfloat16)):
        S, G, F = plan.S, plan.G, plan.F
        with pytest.raises(_capi.InvalidArgumentError):
            plan.epilogue_supported(BIAS | RELU)
        x, w = dev(plan.N, S, plan.H, plan.W).to(dtype), dev(1, S, G, F)
        mu, sigma = torch.zeros(1, S, G, F, device="cuda"), torch.full((1, S, G, F), 0.5, device="cuda")
        with pytest.raises(_capi.InvalidArgumentError):
            plan.forward(x, w, mu, mu.clone(), sigma, bias=torch.zeros(F, device="cuda"))
        with pytest.raises(_capi.InvalidArgumentError):
            plan.forward(x, w, mu, mu.clone(), sigma, relu=True)
        plan.forward(x, w, mu, mu.clone(), sigma)                # the plain call still runs
        plan.check_status()


@pytest.mark.parametrize("name", ["split_17x13_m3", "exact_stacked_28x28"])
def test_no_epilogue_through_the_new_entry_is_forward(name):
    from dau_conv import _capi
    x, y, _ = _shared(name)
    plan = _plan(name, "f32")
    w, mu1, mu2, sigma = _params(name)
    out = torch.full_like(y, float("nan"))
    ws = torch.empty(plan.workspace_bytes(_capi.PASS_FORWARD), dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = _capi.lib.dau_conv_forward_epilogue(plan._h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), p(x), p(w), p(mu1), p(mu2),
                                             p(sigma), None, 0, p(out), p(ws), ws.numel())
    assert rc == _capi.DAU_OK, _capi.lib.dau_conv_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), y.view(torch.int32))
