"""CPU: the fused input ReLU (DAU_FLAG_INPUT_RELU) at plan level -- the flag's value, that a plan with it IS the plan without it
(dau_conv_plan_info and all three workspace sizes, for every activation format and layout), the three refusals and their messages,
Plan.input_relu, the layer's argument handling and the plan-cache key, and the NULL x of a dx-only backward call.  Plan creation
needs no device; nothing is launched here.  (GPU: tests/test_gpu_input_relu.py, tests/test_gpu_input_relu_layer.py.)"""
import ctypes
import re

import pytest

from layers import _leave_the_plan_cache_as_it_was  # noqa: F401 (the autouse fixture)
from test_capi_symbols import HEADER


# S, F, G, H, W, kernel: the north-star layer, a small exact plan, a four-window plan, a forced-split odd shape
SHAPES = ((256, 256, 4, 56, 56, 9), (8, 16, 6, 28, 28, 9), (2, 20, 9, 37, 100, 65), (7, 5, 2, 17, 13, 9))


def _flags():
    from dau_conv import _capi
    return _capi, _capi.FLAG_USE_INTERPOLATION, _capi.FLAG_INPUT_RELU


def test_flag_value_in_the_header_and_the_binding():
    _capi, _, IR = _flags()
    assert IR == 1 << 14
    m = re.search(r"DAU_FLAG_INPUT_RELU\s*=\s*1\s*<<\s*(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == 14
    assert re.search(r"#define DAU_CONV_ABI_VERSION 4\b", open(HEADER).read())      # the ABI version stays
    assert _capi.lib.dau_conv_abi_version() == 4


def test_the_flagged_plan_is_the_unflagged_plan():
    """info field by field and the forward / backward / epilogue-backward workspaces, f32 / f16 / bf16, NCHW / NHWC, and with the
    flags it combines with"""
    _capi, I, IR = _flags()
    combos = [0, _capi.FLAG_DENSE_SPLIT_F16, _capi.FLAG_NO_DENSE_SPLIT, _capi.FLAG_DENSE_SPLIT_F16 | _capi.FLAG_DENSE_SPLIT_OUTLIERS,
              _capi.FLAG_STATIC_BUCKET]
    for S, F, G, H, W, k in SHAPES:
        for io in (0, _capi.FLAG_IO_F16, _capi.FLAG_IO_BF16):
            for layout in (0, _capi.FLAG_IO_NHWC):
                for extra in combos:
                    base = I | io | layout | extra
                    on = _capi.Plan(4, S, F, G, H, W, max_kernel_size=k, sigma_hint=0.5, flags=base | IR)
                    off = _capi.Plan(4, S, F, G, H, W, max_kernel_size=k, sigma_hint=0.5, flags=base)
                    assert on.info == off.info, (S, F, G, H, W, k, hex(base))
                    for which in (_capi.PASS_FORWARD, _capi.PASS_BACKWARD, _capi.PASS_EPILOGUE_BACKWARD):
                        assert on.workspace_bytes(which) == off.workspace_bytes(which), (S, F, G, H, W, k, hex(base), which)
                    assert on.input_relu is True and off.input_relu is False
                    assert on.io_layout == off.io_layout and on.io_dtype == off.io_dtype


def test_a_slabbed_plan_stays_the_same_plan(monkeypatch):
    _capi, I, IR = _flags()
    monkeypatch.setenv("DAU_WORKSPACE_BUDGET_GB", "0.0005")
    on = _capi.Plan(4, 16, 40, 4, 28, 28, sigma_hint=0.5, flags=I | _capi.FLAG_DENSE_SPLIT_F16 | IR)
    off = _capi.Plan(4, 16, 40, 4, 28, 28, sigma_hint=0.5, flags=I | _capi.FLAG_DENSE_SPLIT_F16)
    assert on.info == off.info and on.info["batch_slab_gather"] < 4


def test_the_three_refusals_name_the_flag():
    _capi, I, IR = _flags()
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_INPUT_RELU excludes DAU_FLAG_DENSE_BF16"):
        _capi.Plan(2, 32, 32, 4, 16, 16, flags=I | _capi.FLAG_IO_BF16 | _capi.FLAG_DENSE_BF16 | IR)
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_INPUT_RELU needs the tiled kernels"):
        _capi.Plan(2, 4, 8, 2, 16, 16, flags=I | IR, algo=_capi.ALGO_DIRECT)
    # a shape that falls back to the direct kernels: more than 16 units per channel pair under a kernel larger than 17
    direct = dict(max_kernel_size=33, sigma_hint=0.5)
    fallback = _capi.Plan(2, 4, 8, 20, 16, 16, flags=I, **direct)
    assert _capi.ALGO_DIRECT in (fallback.info["algo_forward"], fallback.info["algo_backward"])
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_INPUT_RELU needs the tiled kernels"):
        _capi.Plan(2, 4, 8, 20, 16, 16, flags=I | IR, **direct)
    # the same descs without the flag are taken
    _capi.Plan(2, 32, 32, 4, 16, 16, flags=I | _capi.FLAG_IO_BF16 | _capi.FLAG_DENSE_BF16)
    _capi.Plan(2, 4, 8, 2, 16, 16, flags=I, algo=_capi.ALGO_DIRECT)


def test_dx_alone_with_a_null_x_is_refused():
    """the dx pass of a flagged plan reads x: DAU_NEED_DX alone does not make it optional.  (All pointers but x are non-null fakes;
    the call returns before it touches any.)"""
    _capi, I, IR = _flags()
    plan = _capi.Plan(2, 8, 16, 2, 16, 16, sigma_hint=0.5, flags=I | IR)
    fake = ctypes.c_void_p(4096)
    need = plan.workspace_bytes(_capi.PASS_BACKWARD)
    rc = _capi.lib.dau_conv_backward(plan._h, None, None, fake, fake, fake, fake, fake, fake, None, None, None, None, fake, need,
                                     _capi.NEED_DX)
    assert rc == _capi.DAU_INVALID_ARGUMENT
    assert b"DAU_FLAG_INPUT_RELU" in _capi.lib.dau_conv_last_error()


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_layer_argument_handling():
    import torch
    import torch.nn as nn
    import dau_conv
    mk = lambda **kw: dau_conv.DAUConv2d(filters=8, dau_units=(2, 1), max_kernel_size=9, in_channels=4, **kw)
    assert mk()._input_relu is False and mk().input_activation is None
    for act in ("relu", torch.relu, nn.functional.relu, nn.ReLU(), nn.ReLU(inplace=True)):
        layer = mk(input_activation=act)
        assert layer._input_relu is True, act
    other = mk(input_activation=torch.tanh)
    assert other._input_relu is False and other.input_activation is torch.tanh
    with pytest.raises(ValueError, match="input_activation"):
        mk(input_activation="gelu")
    with pytest.raises(ValueError, match="input_activation"):
        mk(input_activation=3)
    one_d = dau_conv.DAUConv1d(filters=8, dau_units=(2, 1), max_kernel_size=9, in_channels=4, input_activation="relu")
    assert one_d._input_relu is True and one_d.dau_unit_single_dim


def test_functional_forms_take_input_activation_fn():
    import inspect
    import dau_conv
    import importlib
    impl = importlib.import_module("dau_conv.dau_conv")
    for fn in (dau_conv.dau_conv2d, dau_conv.dau_conv1d):
        assert inspect.signature(fn).parameters["input_activation_fn"].default is None
    assert inspect.signature(impl.dau_conv).parameters["input_activation"].default is None


class _FakeInput(object):
    """what _get_plan reads of an input tensor (plan creation needs no device)"""
    def __init__(self, shape, dtype):
        import torch
        self.shape, self.dtype, self.device = torch.Size(shape), dtype, torch.device("cuda", 0)


def test_the_flag_is_part_of_the_plan_key_and_refusals_fall_back():
    import torch
    from dau_conv import _capi
    import importlib
    impl = importlib.import_module("dau_conv.dau_conv")
    sigma = torch.full((1, 8, 2, 16), 0.5)
    w = torch.zeros(1, 8, 2, 16)
    st = impl._settings(sigma, num_output=16, kernel_size=9, sigma_hint=0.5)
    x = _FakeInput((2, 8, 16, 16), torch.float32)
    plain = impl._get_plan(x, w, st)
    fused = impl._get_plan(x, w, dict(st, input_relu=True))
    assert plain is not fused and fused.input_relu and not plain.input_relu
    assert impl._get_plan(x, w, dict(st, input_relu=True)) is fused and impl._get_plan(x, w, st) is plain      # both cached
    assert fused.info == plain.info
    # dense_bf16: the flag is excluded -- the unflagged plan comes back, and the caller applies torch.relu
    xb = _FakeInput((2, 32, 16, 16), torch.bfloat16)
    wb = torch.zeros(1, 32, 4, 32)
    stb = impl._settings(torch.full((1,), 0.5), num_output=32, kernel_size=9, sigma_hint=0.5, dense_bf16=True)
    got = impl._get_plan(xb, wb, dict(stb, input_relu=True))
    assert not got.input_relu and got.info["gather_dense_bf16"]
    # the direct kernels: refused once, remembered
    std = impl._settings(sigma, num_output=16, kernel_size=9, sigma_hint=0.5, algo=_capi.ALGO_DIRECT)
    n = len(impl._REFUSED)
    got = impl._get_plan(x, w, dict(std, input_relu=True))
    assert not got.input_relu and got.info["algo_forward"] == _capi.ALGO_DIRECT
    assert len(impl._REFUSED) == n + 1
    assert impl._get_plan(x, w, dict(std, input_relu=True)) is got and len(impl._REFUSED) == n + 1


def test_dau_conv_refuses_other_input_activations():
    import torch
    from dau_conv import _capi
    import importlib
    impl = importlib.import_module("dau_conv.dau_conv")
    t = torch.zeros(1, 2, 2, 4)
    with pytest.raises(_capi.InvalidArgumentError, match="input_activation must be None or \"relu\""):
        impl.dau_conv(torch.zeros(1, 2, 8, 8), t, t, t, t, input_activation="tanh", num_output=4)
