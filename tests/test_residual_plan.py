"""CPU: the additive part of the C ABI for the residual add of the fused epilogue (dau_conv_forward_residual) and the refusals that
need no device.  The residual is an argument, not an epilogue bit.  No compute is launched here."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dau_conv.h")
LIB = os.path.join(ROOT, "dau-convnet_amd", "dau_conv", "libdau_conv_hip.so")
I = 1 << 0          # DAU_FLAG_USE_INTERPOLATION


def test_the_entry_is_declared_and_exported_and_the_abi_version_stays():
    src = open(HEADER).read()
    decl = re.search(r"DAU_API\s+int\s+dau_conv_forward_residual\s*\(([^;]*)\)\s*;", src)
    assert decl, "include/dau_conv.h does not declare dau_conv_forward_residual"
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["plan", "stream", "x", "w", "mu1", "mu2", "sigma", "bias", "residual", "epilogue", "y",
                                                        "workspace", "workspace_bytes"]
    assert re.search(r"#define\s+DAU_CONV_ABI_VERSION\s+4\b", src)
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "dau_conv_forward_residual"), "missing export dau_conv_forward_residual"
    assert lib.dau_conv_abi_version() == 4
    from dau_conv import _capi
    assert len(_capi.lib.dau_conv_forward_residual.argtypes) == 13


def test_the_residual_is_no_epilogue_bit():
    from dau_conv import _capi
    tiled = _capi.Plan(2, 8, 16, 2, 16, 16)
    with pytest.raises(_capi.InvalidArgumentError, match="unknown epilogue bits"):
        tiled.epilogue_supported(4)
    assert tiled._residual_supported() is True
    # the C entry refuses the bit as well, residual or not, before it looks at any pointer
    for residual in (None, ctypes.c_void_p(256)):
        rc = _capi.lib.dau_conv_forward_residual(tiled._h, None, None, None, None, None, None, None, residual, 4, None, None, 0)
        assert rc == _capi.DAU_INVALID_ARGUMENT and b"unknown epilogue bits" in _capi.lib.dau_conv_last_error()


def _tensors(plan, dtype=torch.float32):
    S, G, F = plan.S, plan.G, plan.F
    x = torch.zeros(plan.N, S, plan.H, plan.W, dtype=dtype)
    par = torch.zeros(1, S, G, F)
    return x, par, par, par, par + 0.5


def test_a_residual_unlike_y_is_refused_before_any_launch():
    """(no device here: a tensor that is not on the GPU is refused whatever else it is, so these calls cannot launch; the same
    refusals on device tensors, where a well-formed residual runs, are in test_gpu_residual.py)"""
    from dau_conv import _capi
    plan = _capi.Plan(2, 8, 16, 2, 16, 16)
    args = _tensors(plan)
    shape = (plan.N, plan.F, plan.H, plan.W)
    with pytest.raises(_capi.InvalidArgumentError, match="residual has shape"):
        plan.forward(*args, residual=torch.zeros(plan.N, plan.F, plan.H, plan.W - 1))          # a wrong shape
    with pytest.raises(_capi.InvalidArgumentError, match="residual must be a contiguous float32"):
        plan.forward(*args, residual=torch.zeros(shape, dtype=torch.float16))                  # a wrong dtype
    with pytest.raises(_capi.InvalidArgumentError, match="residual must be a contiguous float32"):
        plan.forward(*args, residual=torch.zeros(shape).contiguous(memory_format=torch.channels_last))   # a wrong layout
    nhwc = _capi.Plan(2, 8, 16, 2, 16, 16, flags=I | _capi.FLAG_IO_NHWC | _capi.FLAG_IO_F16)
    with pytest.raises(_capi.InvalidArgumentError, match="residual must be a channels_last float16"):
        nhwc.forward(*_tensors(nhwc, torch.float16), residual=torch.zeros(shape, dtype=torch.float16))


def test_plans_without_a_fused_epilogue_refuse_a_residual_and_name_the_reason():
    from dau_conv import _capi
    direct = _capi.Plan(2, 8, 16, 2, 16, 16, algo=_capi.ALGO_DIRECT)
    dense = _capi.Plan(2, 32, 32, 4, 16, 16, flags=I | _capi.FLAG_IO_BF16 | _capi.FLAG_DENSE_BF16)
    for plan, dtype, why in ((direct, torch.float32, "direct kernels"), (dense, torch.bfloat16, "DAU_FLAG_DENSE_BF16")):
        res = torch.zeros(plan.N, plan.F, plan.H, plan.W, dtype=dtype)
        with pytest.raises(_capi.InvalidArgumentError, match=why):
            plan._residual_supported()
        with pytest.raises(_capi.InvalidArgumentError, match=why):
            plan.forward(*_tensors(plan, dtype), residual=res)
        # the C entry itself: refused with its own message whatever the epilogue bits (the pointer is never followed)
        for e in (0, _capi.EPILOGUE_BIAS | _capi.EPILOGUE_RELU):
            rc = _capi.lib.dau_conv_forward_residual(plan._h, None, None, None, None, None, None, None, ctypes.c_void_p(256), e, None, None, 0)
            msg = _capi.lib.dau_conv_last_error()
            assert rc == _capi.DAU_INVALID_ARGUMENT and why.encode() in msg and b"residual" in msg, msg


def test_layer_and_op_take_the_new_argument():
    import dau_conv
    from dau_conv import _capi
    assert inspect.signature(_capi.Plan.forward).parameters["residual"].default is None
    assert inspect.signature(dau_conv.dau_conv).parameters["residual"].default is None
    for cls in (dau_conv.DAUConv2d, dau_conv.DAUConv1d):
        assert inspect.signature(cls.forward).parameters["residual"].default is None
        assert cls.call is cls.forward
    for fn in (dau_conv.dau_conv2d, dau_conv.dau_conv1d):              # the functional wrappers do not change
        assert "residual" not in inspect.signature(fn).parameters
