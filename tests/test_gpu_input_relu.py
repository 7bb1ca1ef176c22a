"""GPU: the fused input ReLU (DAU_FLAG_INPUT_RELU) at the plan level.  ReLU rounds nothing, so every bar is identity: a flagged plan
fed the raw x returns the bits the SAME plan without the flag returns on x' = where(x <= 0, 0, x) -- y and the four parameter
gradients -- and its dx is where(x <= 0, 0, dx of that reference), for float32, float16 and bfloat16, NCHW and NHWC.  x is randn
(sign-symmetric); every test asserts that between 0.2 and 0.8 of it is <= 0, so a clamp that does nothing cannot pass.  The rows are
member_rows.FUSED_ROWS, the smallest shapes that reach every member; each proves through Plan.info / outlier_status that its member
runs, and every call runs on a fresh plan, forward first and backward second, so that the flagged calls take the bucket sets the
reference calls took (test_gpu_residual.py explains why)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import member_rows as mr
from member_rows import IO, OUTLIERS, SLAB_ROWS, lay as _lay, nhwc_view as _nhwc_view
from util import assert_parity, assert_same_bits, bits as _bits

pytestmark = pytest.mark.gpu

INPUT_RELU = 1 << 14
GRADS = ("dw", "dmu1", "dmu2", "dsigma")
ROWS = mr.FUSED_ROWS                         # the parametrised tests run these, the slab test the rows of four images
_inputs = functools.partial(mr.inputs, x="randn")      # sign-symmetric: the ReLU cuts about half
_params = functools.partial(mr.params, x="randn")
_assert_same_bits = functools.partial(assert_same_bits, keys=("y", "dx") + GRADS)


def _plan(name, io, nhwc=False, fused=False):
    plan = mr.plan(name, io, nhwc, INPUT_RELU if fused else 0)
    assert plan.input_relu == fused
    return plan


def _clamp(x):
    return torch.where(x <= 0, torch.zeros_like(x), x)          # the issue's reference: a NaN stays, -0 becomes +0


def _assert_share(x):
    share = float((x.float() <= 0).float().mean())
    assert 0.2 < share < 0.8, "%.2f of x is <= 0: the clamp would not show" % share


def _run(plan, name, x, dy, **fwd):
    """forward, then backward, each followed by the status check (the order every call of this file keeps) -> dict of tensors"""
    p = _params(name)
    y = plan.forward(_lay(x, plan), *p, **fwd)
    plan.check_status()
    if mr.ROWS[name][0] & OUTLIERS:
        assert plan.outlier_status() == (1, True), "the radius-3 + ring member did not run (forward)"
    dx, dw, dmu1, dmu2, dsigma = plan.backward(_lay(x, plan), _lay(dy, plan), *p)
    plan.check_status()
    if mr.ROWS[name][0] & OUTLIERS:
        assert plan.outlier_status() == (1, True), "the radius-3 + ring member did not run (dx)"
    return dict(y=y, dx=dx, dw=dw, dmu1=dmu1, dmu2=dmu2, dsigma=dsigma)


_X = {}             # name -> (x, dy) fp32 on the device: made once, never written
_REF = {}           # (name, io) -> the unflagged NCHW plan's tensors on the clamped x, dx masked: computed once, never written


def _xdy(name):
    if name not in _X:
        x, dy = _inputs(name)[:2]
        _X[name] = (torch.from_numpy(x).cuda(), torch.from_numpy(dy).cuda())
    return _X[name]


def _reference(name, io, x=None):
    """the same plan without the flag, fed where(x <= 0, 0, x); its dx followed by where(x <= 0, 0, dx)"""
    key = (name, io)
    if x is None and key in _REF:
        return _REF[key]
    dtype = IO[io][1]
    x0, dy = _xdy(name)
    xr = (x0 if x is None else x).to(dtype)
    out = _run(_plan(name, io), name, _clamp(xr), dy.to(dtype))
    out["dx"] = torch.where(xr <= 0, torch.zeros_like(out["dx"]), out["dx"])
    if x is None:
        _REF[key] = out
    return out


# ---- 1. float32, 16-bit, layouts, slabs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", list(ROWS))
def test_the_flagged_plan_on_raw_x_is_the_plan_on_clamped_x(name, nhwc):
    """y, dx (masked) and all four parameter gradients, bit for bit, in all three formats; the NHWC call against the NCHW reference,
    so it also equals the NCHW call's bits"""
    x, dy = _xdy(name)
    _assert_share(x)
    for io in ("f32", "f16", "bf16"):
        dtype = IO[io][1]
        want = _reference(name, io)
        plan = _plan(name, io, nhwc, fused=True)
        got = _run(plan, name, x.to(dtype), dy.to(dtype))
        fmt = torch.channels_last if nhwc else torch.contiguous_format
        assert got["y"].dtype == dtype and got["dx"].dtype == dtype
        assert got["y"].is_contiguous(memory_format=fmt) and got["dx"].is_contiguous(memory_format=fmt)
        _assert_same_bits(got, want, "%s/%s/%s" % (name, io, "nhwc" if nhwc else "nchw"))
        # the mask is there and is the input's: dx vanishes exactly where x <= 0 (the sums themselves are not zero there)
        cut = (x.to(dtype) <= 0)
        assert bool((got["dx"].contiguous()[cut] == 0).all())
        assert float((got["dx"].contiguous()[~cut] != 0).float().mean()) > 0.9


def test_param_sums_take_the_clamp():
    """dau_conv_backward_param_sums: the raw sums of the flagged plan on x are those of the plain plan on the clamped x"""
    for name in ("exact_stacked_28x28", "default_128"):
        x, dy = _xdy(name)
        _assert_share(x)
        _, mu1, mu2, sigma = _params(name)
        want = _plan(name, "f32").backward_param_sums(_clamp(x), dy, mu1, mu2, sigma)
        got = _plan(name, "f32", fused=True).backward_param_sums(x, dy, mu1, mu2, sigma)
        assert torch.equal(_bits(got), _bits(want)), name


@pytest.mark.parametrize("name", list(SLAB_ROWS))
def test_batch_slabs_index_the_gate_by_the_global_image(name, monkeypatch):
    """under a workspace budget the passes run in slabs of images: every slab masks by the x of the images it writes"""
    name = SLAB_ROWS[name]
    x, dy = _xdy(name)
    _assert_share(x)
    N = x.shape[0]
    for io in ("f32", "f16", "bf16"):
        dtype = IO[io][1]
        for nhwc in (False, True):
            whole = _plan(name, io, nhwc, fused=True)
            assert whole.info["batch_slab_gather"] == N
            want = _run(whole, name, x.to(dtype), dy.to(dtype))
            monkeypatch.setenv("DAU_WORKSPACE_BUDGET_GB", "0.0005")
            slabbed = _plan(name, io, nhwc, fused=True)
            monkeypatch.delenv("DAU_WORKSPACE_BUDGET_GB")
            assert slabbed.info["batch_slab_gather"] < N, slabbed.info
            got = _run(slabbed, name, x.to(dtype), dy.to(dtype))
            _assert_same_bits(got, want, "%s/%s/slabs" % (name, io), keys=("y", "dx"))
            _assert_same_bits(got, _reference(name, io), "%s/%s/slabs against the reference" % (name, io), keys=("y", "dx"))
            # the images differ, so a slab that read the first images' x would show
            assert not torch.equal(_bits(want["dx"][:2]), _bits(want["dx"][2:]))


# ---- 2. special values, unaligned bases ----------------------------------------------------------------------------------------------
def _same_values(got, want, what):
    g, w = got.float().contiguous().cpu().numpy(), want.float().contiguous().cpu().numpy()
    assert np.array_equal(np.isnan(g), np.isnan(w)), "%s: NaNs in other places" % what
    np.testing.assert_array_equal(g, w, err_msg=what)          # (NaNs in the same places count as equal)


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", list(ROWS))
def test_special_values_and_an_all_negative_image(name, nhwc):
    x0, dy = _xdy(name)
    N, S, H, W = x0.shape
    x = x0.clone()
    c1, c2 = 1 % S, 2 % S                                       # (S = 2: the rows' smallest channel count)
    x[0, 0, 1, 2] = float("nan")
    x[0, S - 1, H - 1, W - 1] = float("inf")
    x[0, c1, 3, 0] = float("-inf")
    x[0, c2, 0, 1] = -0.0
    x[0, c2, 0, 2] = 0.0
    dead = N - 1                                                # one image entirely <= 0 (zeros and -0 among the negatives)
    x[dead] = -x0[dead].abs()
    x[dead, 0, 0, :3] = torch.tensor([0.0, -0.0, float("-inf")], device="cuda")
    _assert_share(x)
    want = _reference(name, "f32", x)
    got = _run(_plan(name, "f32", nhwc, fused=True), name, x, dy)
    for k in ("y", "dx") + GRADS:
        _same_values(got[k], want[k], "%s/%s" % (name, k))
    assert bool(torch.isnan(got["y"]).any()), "the NaN of x is lost"
    # -0, 0 and -Inf cut their dx (a NaN x passes it through: the reference's where(x <= 0, 0, dx) above says so)
    dxc = got["dx"].contiguous()
    assert float(dxc[0, c2, 0, 1]) == 0 and float(dxc[0, c2, 0, 2]) == 0 and float(dxc[0, c1, 3, 0]) == 0
    # the all-negative image: y is the layer's output for a zero image (no bias: zeros), dx vanishes
    assert bool((got["y"].contiguous()[dead] == 0).all()) and bool((dxc[dead] == 0).all())
    # images are independent: the other images' bits are those of the batch in which that image is an ordinary one
    x2 = x.clone()
    x2[dead] = x0[dead]
    other = _run(_plan(name, "f32", nhwc, fused=True), name, x2, dy)
    for k in ("y", "dx"):
        assert torch.equal(_bits(got[k])[:dead], _bits(other[k])[:dead]), "%s: %s of the other images moved" % (name, k)


def _raw_backward(plan, name, x, dy, dx):
    """dau_conv_backward itself on the given device pointers; dx is written in place -> the four parameter gradients"""
    from dau_conv import _capi
    w, mu1, mu2, sigma = _params(name)
    ws = torch.empty(plan.workspace_bytes(_capi.PASS_BACKWARD), dtype=torch.uint8, device="cuda")
    grads = [torch.empty_like(w) for _ in range(4)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = _capi.lib.dau_conv_backward(plan._h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), p(x), p(dy), p(w), p(mu1), p(mu2),
                                     p(sigma), p(dx), p(grads[0]), p(grads[1]), p(grads[2]), p(grads[3]), p(ws), ws.numel(),
                                     _capi.NEED_ALL)
    assert rc == _capi.DAU_OK, _capi.lib.dau_conv_last_error()
    torch.cuda.synchronize()
    return dict(zip(GRADS, grads))


@pytest.mark.parametrize("io", ["f32", "f16", "bf16"])
def test_x_and_dx_bases_one_element_off(io):
    """S = 16, NHWC: groups of four channels of the gate move as 16- or 8-byte loads where x's OWN base allows it, dx's groups as
    vector stores where dx's does: an unaligned x beside an aligned dx, the reverse, and both -- the bits of the aligned call, x keeps
    every byte and nothing is written outside dx"""
    name = "split_tall_28x28"
    x, dy = _xdy(name)
    _assert_share(x)
    dtype = IO[io][1]
    probe = _plan(name, io, True, fused=True)
    xin, dyin = _lay(x.to(dtype), probe), _lay(dy.to(dtype), probe)
    shape, n, pad = tuple(x.shape), x.numel(), 8
    width = 16 if io == "f32" else 8
    flat_x = xin.permute(0, 2, 3, 1).reshape(-1)
    aligned = torch.empty_like(xin)
    want = _raw_backward(_plan(name, io, True, fused=True), name, xin, dyin, aligned)
    want["dx"] = aligned
    # (a first backward call of a fresh plan: compare with the same of the reference plan)
    ref_dx = torch.empty_like(xin)
    ref = _raw_backward(_plan(name, io, True), name, _lay(_clamp(x.to(dtype)), probe), dyin, ref_dx)
    ref["dx"] = torch.where(xin <= 0, torch.zeros_like(ref_dx), ref_dx)
    _assert_same_bits(want, ref, "aligned/" + io, keys=("dx",) + GRADS)
    for x_off, dx_off in ((1, 0), (0, 1), (1, 1)):
        xbuf = torch.full((n + 2 * pad,), 3.0, dtype=dtype, device="cuda")
        xbuf[x_off:x_off + n] = flat_x
        dxbuf = torch.full((n + 2 * pad,), -7.0, dtype=dtype, device="cuda")
        xv, dxv = _nhwc_view(xbuf, shape, x_off), _nhwc_view(dxbuf, shape, dx_off)
        assert xbuf.data_ptr() % width == 0 and dxbuf.data_ptr() % width == 0
        assert (xv.data_ptr() % width != 0) == bool(x_off) and (dxv.data_ptr() % width != 0) == bool(dx_off)
        before = xbuf.clone()
        got = _raw_backward(_plan(name, io, True, fused=True), name, xv, dyin, dxv)
        got["dx"] = dxv
        _assert_same_bits(got, want, "x offset %d, dx offset %d" % (x_off, dx_off), keys=("dx",) + GRADS)
        assert torch.equal(_bits(xbuf), _bits(before)), "x was written"
        assert bool((dxbuf[:dx_off] == -7).all()) and bool((dxbuf[dx_off + n:] == -7).all()), "dx was written outside its view"


# ---- 3. with the fused output epilogue -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", list(ROWS))
def test_with_bias_relu_and_residual_in_the_same_call(name, nhwc):
    """input ReLU in front, bias + residual + ReLU behind: float32 is relu((y_ref + bias) + r) of the reference y, bit for bit; the
    16-bit formats are the unflagged plan's fused call on the clamped tensor, bit for bit"""
    x, dy = _xdy(name)
    _assert_share(x)
    y32 = _reference(name, "f32")["y"]
    F = y32.shape[1]
    bias = (torch.from_numpy(np.random.RandomState(7).randn(F).astype(np.float32)).cuda() * y32.std()).contiguous()
    r = torch.from_numpy(np.random.RandomState(8).randn(*y32.shape).astype(np.float32)).cuda() * y32.std()
    for io in ("f32", "f16", "bf16"):
        dtype = IO[io][1]
        plan = _plan(name, io, nhwc, fused=True)
        xin, rin = x.to(dtype), r.to(dtype)
        got = plan.forward(_lay(xin, plan), *_params(name), bias=bias, relu=True, residual=_lay(rin, plan))
        plan.check_status()
        if io == "f32":
            want = torch.relu((y32 + bias.view(1, -1, 1, 1)) + r)
            cut = float((want == 0).float().mean())
            assert 0.2 < cut < 0.8, cut
        else:
            ref = _plan(name, io)
            want = ref.forward(_clamp(xin), *_params(name), bias=bias, relu=True, residual=rin)
            ref.check_status()
        assert torch.equal(_bits(got), _bits(want)), "%s/%s: %d values differ" % (name, io, int((_bits(got) != _bits(want)).sum()))


# ---- 4. against the CPU oracle: a bug shared by both sides of the identities would pass them -----------------------------------------
@pytest.mark.parametrize("name", ["exact_stacked_28x28", "default_128"])
def test_against_the_oracle_on_the_clamped_input(name):
    from oracle import dau_oracle as orc
    xn, dyn, w, mu1, mu2 = _inputs(name)
    x, dy = _xdy(name)
    _assert_share(x)
    got = _run(_plan(name, "f32", fused=True), name, x, dy)
    xc = np.where(xn <= 0, np.float32(0), xn)
    want = orc.backward(xc, dyn, w, mu1, mu2, 0.5)
    want["y"] = orc.forward(xc, w, mu1, mu2, 0.5)
    want["dx"] = np.where(xn <= 0, np.float32(0), want["dx"])
    for k in ("y", "dx") + GRADS:                              # the members' own bars: util.assert_parity's defaults
        assert_parity(got[k].cpu().numpy(), want[k], "%s/oracle/%s" % (name, k))
