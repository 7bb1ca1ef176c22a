"""GPU: the residual add of the fused epilogue at the plan level.  dau_conv_forward_residual stores
y = act((sum + bias[f]) + r[n,f,h,w]) -- two fp32 adds in that order and a clamp on the very value dau_conv_forward stores, before the
store's one rounding -- so for float32 the bar is identity with relu((forward(x) + bias) + r), for the 16-bit formats identity with
the rounded float32 fused result on the widened x and r, and for NHWC identity with the NCHW call.  The rows are
member_rows.FUSED_ROWS; each proves through Plan.info / outlier_status that its member runs, and each fused call runs on a fresh plan
so that it takes the bucket set the unfused call took."""
import ctypes

import numpy as np
import pytest
import torch

import member_rows as mr
from member_rows import I, IO, OUTLIERS, SLAB_ROWS, act as _act, inputs as _inputs, io_of as _io_of, nhwc_view as _nhwc_view, params as _params, \
    plan as _plan
from util import assert_parity, bits as _bits

pytestmark = pytest.mark.gpu

BIAS, RELU = 1, 2
EPILOGUES = (0, BIAS, BIAS | RELU, RELU)     # each WITH a residual: 0 is the plain fused add
ROWS = mr.FUSED_ROWS                         # the parametrised tests run these, the slab test its four-image row as well

_SHARED = {}        # name -> (x fp32 on the device, unfused fp32 y, bias, residual fp32): computed once, never written


def _shared(name):
    if name not in _SHARED:
        x = torch.from_numpy(_inputs(name)[0]).cuda()
        plan = _plan(name, "f32")
        y = plan.forward(x, *_params(name))
        plan.check_status()
        # bias and residual: randn at the size of y, all three terms symmetric about zero, so ReLU cuts about half of the outputs
        F = y.shape[1]
        bias = (torch.from_numpy(np.random.RandomState(7).randn(F).astype(np.float32)).cuda() * y.std()).contiguous()
        r = torch.from_numpy(np.random.RandomState(8).randn(*y.shape).astype(np.float32)).cuda() * y.std()
        _SHARED[name] = (x, y, bias, r)
    return _SHARED[name]


def _fused(plan, name, x, epilogue, r, extra_plan=None):
    """the fused forward with the residual `r` (a tensor in the plan's dtype and layout, or None) on a plan of its own with `plan`'s
    flags: a plan's first call has no offset-bucket hint and runs the kernels of its static bucket, as the call that made the shared
    unfused y did"""
    bias = _shared(name)[2]
    plan = extra_plan if extra_plan is not None else _plan(name, _io_of(plan), plan.io_layout == "NHWC")
    y = plan.forward(x, *_params(name), bias=bias if epilogue & BIAS else None, relu=bool(epilogue & RELU), residual=r)
    plan.check_status()
    if mr.ROWS[name][0] & OUTLIERS:
        assert plan.outlier_status() == (1, True), "the radius-3 + ring member did not run"
    return y


def _unfused(y, bias, r, epilogue):
    out = y + bias.view(1, -1, 1, 1) if epilogue & BIAS else y
    out = out + r
    return torch.relu(out) if epilogue & RELU else out


def _assert_cut(want, what):
    cut = float((want == 0).float().mean())
    assert 0.2 < cut < 0.8, "ReLU cuts %.2f of the outputs: %s is not at the size of y" % (cut, what)


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", list(ROWS))
def test_fp32_fused_is_the_unfused_result(name, nhwc):
    """identity, not a tolerance: both forms perform the same two fp32 adds in the same order (a contracted FMA, or the adds the
    other way round, fails this)"""
    x, y, bias, r = _shared(name)
    plan = _plan(name, "f32", nhwc)
    xin, rin = _act(x, torch.float32, plan), _act(r, torch.float32, plan)
    for e in EPILOGUES:
        got = _fused(plan, name, xin, e, rin)
        assert got.dtype == torch.float32 and got.is_contiguous(memory_format=torch.channels_last if nhwc else torch.contiguous_format)
        want = _unfused(y, bias, r, e)
        if e & RELU:
            _assert_cut(want, "bias or residual")
        assert torch.equal(got.contiguous(), want), "epilogue %d: %d of %d values differ" % (e, int((got != want).sum()), want.numel())


@pytest.mark.parametrize("io", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(ROWS))
def test_16bit_fused_is_the_rounded_fp32_fused_result_in_both_layouts(name, io):
    """one rounding: the 16-bit plan stores the rounding of what the fp32 plan computes from the widened x and the widened r, and
    the NHWC plan stores the bits of the NCHW plan"""
    x, _, _, r = _shared(name)
    dtype = IO[io][1]
    p16, p16n, p32 = _plan(name, io), _plan(name, io, True), _plan(name, "f32")
    x16, r16 = x.to(dtype), r.to(dtype)
    windows = p16.info["gather_windows"]
    for e in EPILOGUES:
        got = _fused(p16, name, x16, e, r16)
        got_nhwc = _fused(p16n, name, _act(x16, dtype, p16n), e, _act(r16, dtype, p16n))
        assert got.dtype == dtype and got_nhwc.dtype == dtype and got_nhwc.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(_bits(got_nhwc), _bits(got)), "epilogue %d: NHWC differs from NCHW" % e
        ref = _fused(p32, name, x16.float(), e, r16.float())
        if e & RELU:
            _assert_cut(ref, "bias or residual")
        if windows == 1:
            assert torch.equal(_bits(got), _bits(ref.to(dtype))), "epilogue %d: %d values differ" % (
                e, int((_bits(got) != _bits(ref.to(dtype))).sum()))
        elif io == "f16":
            # every window pass re-reads the stored value, adds and rounds again: test_gpu_f16.py's bar for windowed plans
            assert_parity(got.float().cpu().numpy(), ref.cpu().numpy(), "y", rel=2e-3, floor=1e-3)
        else:
            # bfloat16: test_gpu_bf16.py's bar for the same kernel-65, four-window plan (the fused store adds no rounding to it)
            assert_parity(got.float().cpu().numpy(), ref.cpu().numpy(), "y", rel=2e-2, floor=4e-3)


@pytest.mark.parametrize("name", list(ROWS))
def test_nhwc_fp32_fused_is_the_nchw_fused(name):
    x, _, _, r = _shared(name)
    a, b = _plan(name, "f32"), _plan(name, "f32", True)
    for e in (0, BIAS | RELU):
        got = _fused(b, name, _act(x, torch.float32, b), e, _act(r, torch.float32, b))
        assert torch.equal(_bits(got), _bits(_fused(a, name, x, e, r))), (name, e)


# ---- the raw entry point: buffers at addresses of the test's choosing --------------------------------------------------------------
def _raw(plan, name, x, bias, r, epilogue, y):
    """dau_conv_forward_residual itself on the given device pointers (tensors; r may be None); y is written in place"""
    from dau_conv import _capi
    w, mu1, mu2, sigma = _params(name)
    ws = torch.empty(plan.workspace_bytes(_capi.PASS_FORWARD), dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = _capi.lib.dau_conv_forward_residual(plan._h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), p(x), p(w), p(mu1), p(mu2),
                                             p(sigma), p(bias), p(r), epilogue, p(y), p(ws), ws.numel())
    assert rc == _capi.DAU_OK, _capi.lib.dau_conv_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("io", ["f32", "f16", "bf16"])
def test_residual_and_output_bases_one_element_off(io):
    """F = 40, NHWC: groups of four channels move as 16- or 8-byte accesses where the base allows it.  The residual's base and y's are
    two allocations: an unaligned residual beside an aligned y must be loaded by elements, and the reverse must still load vectors and
    store elements -- the bits of the call on two aligned tensors either way, and the residual's buffer keeps every byte."""
    name = "split_tall_28x28"
    x, _, bias, r = _shared(name)
    dtype = IO[io][1]
    plan = _plan(name, io, True)
    xin, rin = _act(x.to(dtype), dtype, plan), _act(r.to(dtype), dtype, plan)
    want = _fused(plan, name, xin, BIAS | RELU, rin)
    shape, n, pad = tuple(want.shape), want.numel(), 8
    flat_r = rin.permute(0, 2, 3, 1).reshape(-1)
    width = 16 if io == "f32" else 8
    for r_off, y_off in ((1, 0), (0, 1), (1, 1)):
        rbuf = torch.full((n + 2 * pad,), 3.0, dtype=dtype, device="cuda")
        rbuf[r_off:r_off + n] = flat_r
        ybuf = torch.full((n + 2 * pad,), -7.0, dtype=dtype, device="cuda")
        rv, yv = _nhwc_view(rbuf, shape, r_off), _nhwc_view(ybuf, shape, y_off)
        assert rbuf.data_ptr() % width == 0 and ybuf.data_ptr() % width == 0
        assert (rv.data_ptr() % width != 0) == bool(r_off) and (yv.data_ptr() % width != 0) == bool(y_off)
        assert rv.is_contiguous(memory_format=torch.channels_last)
        before = rbuf.clone()
        _raw(_plan(name, io, True), name, xin, bias, rv, BIAS | RELU, yv)
        assert torch.equal(_bits(yv), _bits(want)), "residual offset %d, y offset %d: %d values differ" % (
            r_off, y_off, int((_bits(yv) != _bits(want)).sum()))
        assert torch.equal(_bits(rbuf), _bits(before)), "the residual's buffer was written"
        assert bool((ybuf[:y_off] == -7).all()) and bool((ybuf[y_off + n:] == -7).all()), "y was written outside its view"
    # the Plan call takes the unaligned view as well (channels_last strides at another storage offset)
    rbuf = torch.zeros(n + 2 * pad, dtype=dtype, device="cuda")
    rbuf[1:1 + n] = flat_r
    got = _fused(plan, name, xin, BIAS | RELU, _nhwc_view(rbuf, shape, 1))
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("name", list(SLAB_ROWS))
def test_batch_slabs_index_the_residual_by_the_global_image(name, monkeypatch):
    """under a workspace budget the pass runs in slabs of images: every slab reads the residual of the images it writes"""
    name = SLAB_ROWS[name]
    x, _, _, r = _shared(name)
    N = x.shape[0]
    for io in ("f32", "f16", "bf16"):
        dtype = IO[io][1]
        for nhwc in (False, True):
            whole = _plan(name, io, nhwc)
            assert whole.info["batch_slab_gather"] == N
            xin, rin = _act(x.to(dtype), dtype, whole), _act(r.to(dtype), dtype, whole)
            want = _fused(whole, name, xin, BIAS | RELU, rin)
            monkeypatch.setenv("DAU_WORKSPACE_BUDGET_GB", "0.0005")
            slabbed = _plan(name, io, nhwc)
            monkeypatch.delenv("DAU_WORKSPACE_BUDGET_GB")
            assert slabbed.info["batch_slab_gather"] < N, slabbed.info
            got = _fused(slabbed, name, xin, BIAS | RELU, rin, extra_plan=slabbed)
            assert torch.equal(_bits(got), _bits(want)), (name, io, nhwc)
            # the images differ, so a slab that read the first images' residual would show
            assert not torch.equal(_bits(want[:2]), _bits(want[2:]))


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", ["split_tall_28x28", "outliers_28x28", "exact_stacked_28x28", "k65_gather_windows"])
def test_a_nan_and_an_inf_in_the_residual_reach_their_own_elements_only(name, nhwc):
    x, _, _, r = _shared(name)
    plan = _plan(name, "f32", nhwc)
    xin = _act(x, torch.float32, plan)
    N, F, H, W = r.shape
    at_nan, at_inf = (0, F - 1, H - 1, W - 1), (N - 1, 1, 2, 3)
    bad = r.clone()
    bad[at_nan] = float("nan")
    bad[at_inf] = float("inf")
    for e in (BIAS, BIAS | RELU):
        clean = _fused(plan, name, xin, e, _act(r, torch.float32, plan)).contiguous()
        got = _fused(plan, name, xin, e, _act(bad, torch.float32, plan)).contiguous()
        assert bool(torch.isnan(got[at_nan])), "ReLU %d: the NaN is lost" % (e & RELU)
        assert float(got[at_inf]) == float("inf")
        same = _bits(got) == _bits(clean)
        assert int((~same).sum()) == 2 and not bool(same[at_nan]) and not bool(same[at_inf]), \
            "%d elements differ from the call with a finite residual" % int((~same).sum())
        assert bool(torch.isfinite(clean).all())


@pytest.mark.parametrize("name", ["split_17x13_m3", "exact_stacked_28x28"])
def test_no_residual_through_the_new_entry_is_the_epilogue_call(name):
    x, y, bias, _ = _shared(name)
    for e in (0, BIAS, BIAS | RELU, RELU):
        plan = _plan(name, "f32")
        want = plan.forward(x, *_params(name), bias=bias if e & BIAS else None, relu=bool(e & RELU))
        out = torch.full_like(y, float("nan"))
        _raw(_plan(name, "f32"), name, x, bias if e & BIAS else None, None, e, out)
        assert torch.equal(_bits(out), _bits(want)), e
        if e == 0:
            assert torch.equal(_bits(out), _bits(y))


# ---- refusals on real tensors ---------------------------------------------------------------------------------------------------------
def test_a_residual_unlike_y_is_refused_before_any_launch():
    from dau_conv import _capi
    name = "split_17x13_m3"
    x, y, bias, r = _shared(name)
    plan = _plan(name, "f32")
    args = (x,) + _params(name)
    with pytest.raises(_capi.InvalidArgumentError, match="residual has shape"):
        plan.forward(*args, residual=r[:, :, :-1].contiguous())
    with pytest.raises(_capi.InvalidArgumentError, match="residual must be a contiguous float32"):
        plan.forward(*args, residual=r.half())
    with pytest.raises(_capi.InvalidArgumentError, match="residual must be a contiguous float32"):
        plan.forward(*args, residual=r.contiguous(memory_format=torch.channels_last))
    with pytest.raises(_capi.InvalidArgumentError, match="residual must be a channels_last"):
        _plan(name, "f32", True).forward(_act(x, torch.float32, _plan(name, "f32", True)), *_params(name), residual=r)
    assert torch.equal(plan.forward(*args, residual=r), y + r)       # and the well-formed one runs: a plain fused add
    dev = lambda *s: torch.rand(*s, device="cuda")
    for p2, dtype, why in ((_capi.Plan(2, 4, 8, 2, 16, 16, algo=_capi.ALGO_DIRECT), torch.float32, "direct kernels"),
                           (_capi.Plan(2, 32, 32, 4, 16, 16, flags=I | _capi.FLAG_IO_BF16 | _capi.FLAG_DENSE_BF16), torch.bfloat16,
                            "DAU_FLAG_DENSE_BF16")):
        S, G, F = p2.S, p2.G, p2.F
        x2, w2 = dev(p2.N, S, p2.H, p2.W).to(dtype), dev(1, S, G, F)
        mu, sigma = torch.zeros(1, S, G, F, device="cuda"), torch.full((1, S, G, F), 0.5, device="cuda")
        res = torch.zeros(p2.N, F, p2.H, p2.W, device="cuda", dtype=dtype)
        with pytest.raises(_capi.InvalidArgumentError, match=why):
            p2.forward(x2, w2, mu, mu.clone(), sigma, residual=res)
        # ... and the C entry itself refuses, with a message of its own
        ws = torch.empty(p2.workspace_bytes(_capi.PASS_FORWARD), dtype=torch.uint8, device="cuda")
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        out = torch.empty_like(res)
        rc = _capi.lib.dau_conv_forward_residual(p2._h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), p(x2), p(w2), p(mu), p(mu),
                                                 p(sigma), None, p(res), 0, p(out), p(ws), ws.numel())
        assert rc == _capi.DAU_INVALID_ARGUMENT and why.encode() in _capi.lib.dau_conv_last_error()
