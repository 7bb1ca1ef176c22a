"""CPU: the additive part of the C ABI for the fused epilogue (bias and ReLU in the gather-sum store, their backward pass).  New
symbols and constants, the ABI version and the struct sizes where they were, the forward / backward workspaces at their sizes, and the
refusals that need no device.  No compute is launched here."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dau_conv.h")
LIB = os.path.join(ROOT, "dau-convnet_amd", "dau_conv", "libdau_conv_hip.so")
I = 1 << 0          # DAU_FLAG_USE_INTERPOLATION


def test_new_symbols_are_exported_and_the_abi_version_stays():
    lib = ctypes.CDLL(LIB)
    for name in ("dau_conv_epilogue_supported", "dau_conv_forward_epilogue", "dau_conv_epilogue_backward"):
        assert hasattr(lib, name), "missing export %s" % name
    assert lib.dau_conv_abi_version() == 4


def test_header_defines_the_new_constants():
    src = open(HEADER).read()
    assert re.search(r"\bDAU_EPILOGUE_BIAS\s*=\s*1\b", src) and re.search(r"\bDAU_EPILOGUE_RELU\s*=\s*2\b", src)
    assert re.search(r"\bDAU_PASS_EPILOGUE_BACKWARD\s*=\s*3\b", src)
    assert re.search(r"#define\s+DAU_CONV_ABI_VERSION\s+4\b", src)
    from dau_conv import _capi
    assert (_capi.EPILOGUE_BIAS, _capi.EPILOGUE_RELU, _capi.PASS_EPILOGUE_BACKWARD) == (1, 2, 3)


def test_struct_sizes_are_unchanged():
    from dau_conv import _capi
    assert ctypes.sizeof(_capi._Desc) == 52 and ctypes.sizeof(_capi._Info) == 76
    # the library checks struct_size against its own sizeof(dau_conv_desc): a plan is created, so the C side agrees
    assert _capi.Plan(2, 3, 4, 2, 8, 9).info["offset_bucket"] == 4


# (N, S, F, G, H, W), kwargs, DAU_PASS_FORWARD bytes, DAU_PASS_BACKWARD bytes -- as reported before the epilogue existed
WORKSPACES = [
    ((2, 7, 5, 2, 17, 13), dict(flags=I | 1 << 9), 850176, 1878784),
    ((2, 128, 128, 4, 16, 16), dict(), 9445632, 34040832),
    ((2, 2, 20, 9, 37, 100), dict(max_kernel_size=65), 1100544, 27899904),
    ((128, 256, 256, 4, 56, 56), dict(), 727720192, 4956108288),
    ((2, 16, 40, 4, 28, 28), dict(flags=I | 1 << 9 | 1 << 12 | 1 << 11 | 1 << 13), 2068736, 10738688),
]


@pytest.mark.parametrize("shape, kw, fwd, bwd", WORKSPACES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_forward_and_backward_workspaces_keep_their_size(shape, kw, fwd, bwd):
    from dau_conv import _capi
    p = _capi.Plan(*shape, sigma_hint=0.5, **kw)
    assert p.workspace_bytes(_capi.PASS_FORWARD) == fwd and p.workspace_bytes(_capi.PASS_BACKWARD) == bwd
    # the partial sums of the bias gradient: a float per output channel and 16384 activations or so, twice over at most
    small = p.workspace_bytes(_capi.PASS_EPILOGUE_BACKWARD)
    elements = shape[0] * shape[2] * shape[4] * shape[5]
    assert 0 < small <= 2 * (4 * shape[2] * (elements // shape[2] // 4096 + 2) + 512), small
    with pytest.raises(_capi.InvalidArgumentError):
        p.workspace_bytes(4)


def test_refusals_name_their_reason():
    from dau_conv import _capi
    both = _capi.EPILOGUE_BIAS | _capi.EPILOGUE_RELU
    tiled = _capi.Plan(2, 8, 16, 2, 16, 16)
    for e in (0, _capi.EPILOGUE_BIAS, _capi.EPILOGUE_RELU, both):
        assert tiled.epilogue_supported(e) is True
    with pytest.raises(_capi.InvalidArgumentError, match="unknown epilogue bits"):
        tiled.epilogue_supported(4)
    direct = _capi.Plan(2, 8, 16, 2, 16, 16, algo=_capi.ALGO_DIRECT)
    with pytest.raises(_capi.InvalidArgumentError, match="direct kernels"):
        direct.epilogue_supported(both)
    dense = _capi.Plan(2, 32, 32, 4, 16, 16, flags=I | _capi.FLAG_IO_BF16 | _capi.FLAG_DENSE_BF16)
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_DENSE_BF16"):
        dense.epilogue_supported(_capi.EPILOGUE_BIAS)


def test_layer_and_op_take_the_new_arguments():
    import inspect
    import dau_conv
    from dau_conv import dau_conv as op_module      # noqa: F401  (the package attribute of that name is the op function)
    assert "fused_epilogue" in inspect.signature(dau_conv.DAUConv2d.__init__).parameters
    assert inspect.signature(dau_conv.DAUConv2d.__init__).parameters["fused_epilogue"].default is False
    sig = inspect.signature(dau_conv.dau_conv)
    assert sig.parameters["bias"].default is None and sig.parameters["activation"].default is None
    for fn in (dau_conv.dau_conv2d, dau_conv.dau_conv1d):
        assert inspect.signature(fn).parameters["fused_epilogue"].default is False
    layer = dau_conv.DAUConv2d(filters=4, dau_units=(2, 1), max_kernel_size=9, in_channels=3, fused_epilogue=True)
    assert layer.fused_epilogue is True and dau_conv.DAUConv1d(4, (2, 1), 9, fused_epilogue=True).fused_epilogue is True
