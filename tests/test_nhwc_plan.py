"""CPU: channels_last activations (DAU_FLAG_IO_NHWC) at plan creation, which needs no device.  An NHWC plan must be the NCHW plan
of the same desc in everything but the addresses of x, y, dy, dx: the same members, buckets, windows, tilings and batch slabs, so
every dau_conv_plan_info field and both workspace sizes are equal -- alone and together with either 16-bit storage format.  Also
the rule by which the layer tells a channels_last input from a contiguous one (CPU tensors, no plan call)."""
import os
import re

import pytest

from test_f16_plan import DESCS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dau_conv.h")

I = 1 << 0          # DAU_FLAG_USE_INTERPOLATION


def test_flag_value_in_python_and_header():
    from dau_conv import _capi
    assert _capi.FLAG_IO_NHWC == 1 << 13
    m = re.search(r"DAU_FLAG_IO_NHWC\s*=\s*1\s*<<\s*(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == 13
    assert _capi.lib.dau_conv_abi_version() == 4          # additive: the ABI version stays


def test_plan_io_layout():
    import torch
    from dau_conv import _capi
    assert _capi.Plan(2, 4, 8, 2, 16, 16, flags=I | _capi.FLAG_IO_NHWC).io_layout == "NHWC"
    assert _capi.Plan(2, 4, 8, 2, 16, 16, flags=I).io_layout == "NCHW"
    p = _capi.Plan(2, 4, 8, 2, 16, 16, flags=I | _capi.FLAG_IO_NHWC | _capi.FLAG_IO_F16)
    assert p.io_layout == "NHWC" and p.io_dtype == torch.float16


@pytest.mark.parametrize("extra", ["FLAG_DENSE_BF16", "FLAG_DENSE_WGRAD_NEVER", "FLAG_DENSE_WGRAD_ALWAYS"])
def test_rejected_combinations(extra):
    from dau_conv import _capi
    # (the qualifiers together with the flag they qualify, so that no other rule refuses the plan first)
    flags = I | _capi.FLAG_IO_NHWC | _capi.FLAG_IO_BF16 | _capi.FLAG_DENSE_BF16 | getattr(_capi, extra)
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_IO_NHWC excludes"):
        _capi.Plan(2, 8, 8, 4, 16, 16, flags=flags)


def test_needs_the_tiled_kernels():
    from dau_conv import _capi
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_IO_NHWC needs the tiled kernels"):
        _capi.Plan(2, 4, 8, 2, 16, 16, flags=I | _capi.FLAG_IO_NHWC, algo=_capi.ALGO_DIRECT)
    # a shape the tiled kernels refuse, where an fp32 plan falls back to the direct kernels (tests/test_f16_plan.py)
    fp32 = _capi.Plan(2, 2, 2, 18, 16, 16, max_kernel_size=65, flags=I)
    assert _capi.ALGO_DIRECT in (fp32.info["algo_forward"], fp32.info["algo_backward"])
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_IO_NHWC needs the tiled kernels"):
        _capi.Plan(2, 2, 2, 18, 16, 16, max_kernel_size=65, flags=I | _capi.FLAG_IO_NHWC)


@pytest.mark.parametrize("storage", [None, "FLAG_IO_F16", "FLAG_IO_BF16"], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("desc", DESCS, ids=lambda d: "%dx%d->%d_G%d_%dx%d_k%d%s" % (d[1], d[4], d[2], d[3], d[5], d[4], d[6], "".join("_" + f[5:] for f in d[7])))
def test_nhwc_plan_equals_the_nchw_plan(desc, storage):
    from dau_conv import _capi
    N, S, F, G, H, W, k, extra = desc
    flags = I | (getattr(_capi, storage) if storage else 0)
    for f in extra:
        flags |= getattr(_capi, f)
    nchw = _capi.Plan(N, S, F, G, H, W, max_kernel_size=k, sigma_hint=0.5, flags=flags)
    nhwc = _capi.Plan(N, S, F, G, H, W, max_kernel_size=k, sigma_hint=0.5, flags=flags | _capi.FLAG_IO_NHWC)
    assert nhwc.info == nchw.info
    assert nchw.info["algo_forward"] == _capi.ALGO_TILED and nchw.info["algo_backward"] == _capi.ALGO_TILED
    for which in (_capi.PASS_FORWARD, _capi.PASS_BACKWARD):
        assert nhwc.workspace_bytes(which) == nchw.workspace_bytes(which)


def test_outlier_plan_keeps_its_ring_member():
    from dau_conv import _capi
    flags = I | _capi.FLAG_DENSE_SPLIT_F16 | _capi.FLAG_DENSE_SPLIT_OUTLIERS
    nchw = _capi.Plan(2, 16, 40, 4, 28, 28, flags=flags)
    nhwc = _capi.Plan(2, 16, 40, 4, 28, 28, flags=flags | _capi.FLAG_IO_NHWC)
    assert nhwc.info == nchw.info and nhwc.info["gather_dense_split"] & (1 << 5)
    for which in (_capi.PASS_FORWARD, _capi.PASS_BACKWARD):
        assert nhwc.workspace_bytes(which) == nchw.workspace_bytes(which)


def test_channels_last_detection():
    """x.dim() == 4 and not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last); strides that fit both
    layouts (C = 1, H = W = 1) count as contiguous and take the NCHW path"""
    import torch
    import dau_conv
    cl = lambda *shape: torch.zeros(*shape).to(memory_format=torch.channels_last)
    assert not dau_conv.is_channels_last(torch.zeros(2, 6, 17, 13))
    assert dau_conv.is_channels_last(cl(2, 6, 17, 13))
    assert dau_conv.is_channels_last(torch.zeros(2, 17, 13, 6).permute(0, 3, 1, 2))
    assert not dau_conv.is_channels_last(cl(2, 1, 17, 13))                   # C = 1
    assert not dau_conv.is_channels_last(cl(2, 6, 1, 1))                     # H = W = 1
    assert not dau_conv.is_channels_last(torch.zeros(6, 17, 13))             # rank 3
    assert not dau_conv.is_channels_last(cl(2, 6, 17, 13)[:, :, ::2])        # neither layout: the layer makes it contiguous
    assert not dau_conv.is_channels_last(torch.zeros(2, 6, 13, 17).transpose(2, 3))


def test_layer_settings_carry_channels_last():
    import dau_conv
    for value in (None, True, False):
        layer = dau_conv.DAUConv2d(filters=8, dau_units=(2, 2), max_kernel_size=9, in_channels=6, channels_last=value)
        assert layer.channels_last is value and layer._dau_convolution_op.channels_last is value
    assert dau_conv.DAUConv2d(filters=8, dau_units=(2, 2), max_kernel_size=9, in_channels=6).channels_last is None
