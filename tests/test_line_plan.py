"""CPU: the opt-in line members of the two-limb gather-sum (DAU_FLAG_DENSE_SPLIT_LINE; k_dense_split.hip compiled with one row of
taps, namespaces l4 and l8) at plan level -- which plans hold them (dau_conv_plan_info.gather_dense_split bits 6 and 7), which flag
combinations are refused, the status query's declaration and export, how the layer keyword and the ops' integer reach the flag -- and
in the built gfx950 code: the l4 / l8 gather and densify kernels (named line_*_kernel) ship and use no scratch.  Plan creation needs no device; nothing
is launched here.  (GPU: tests/test_gpu_dense_line.py.)"""
import ctypes
import re

import pytest

from test_built_code import _kernel_name, release  # noqa: F401  (release: the fixture)
from test_capi_symbols import HEADER, LIB, declared_symbols

LINE4, LINE8 = 1 << 6, 1 << 7


def _plan(flags, S, F, G, H, W, N=2, k=9, **kw):
    from dau_conv import _capi
    return _capi.Plan(N, S, F, G, H, W, max_kernel_size=k, sigma_hint=0.5, flags=_capi.FLAG_USE_INTERPOLATION | flags, **kw)


def _single(extra=0):
    from dau_conv import _capi
    return _capi.FLAG_SINGLE_DIM_KERNEL | extra


def _line(extra=0):
    from dau_conv import _capi
    return _capi.FLAG_SINGLE_DIM_KERNEL | _capi.FLAG_DENSE_SPLIT_LINE | extra


def test_flag_value_and_query_are_declared_and_exported():
    from dau_conv import _capi
    src = open(HEADER).read()
    assert re.search(r"DAU_FLAG_DENSE_SPLIT_LINE\s*=\s*1\s*<<\s*15\b", src) and _capi.FLAG_DENSE_SPLIT_LINE == 1 << 15
    assert re.search(r"#define\s+DAU_CONV_ABI_VERSION\s+4\b", src)
    assert "dau_conv_gather_line_status" in declared_symbols()
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "dau_conv_gather_line_status")
    assert lib.dau_conv_abi_version() == 4
    # the query validates its arguments like dau_conv_check_status
    lib.dau_conv_gather_line_status.argtypes = [ctypes.c_void_p] * 5
    assert lib.dau_conv_gather_line_status(None, None, None, None, None) == _capi.DAU_INVALID_ARGUMENT


def test_invalid_flag_combinations():
    from dau_conv import _capi
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_DENSE_SPLIT_LINE needs DAU_FLAG_SINGLE_DIM_KERNEL"):
        _plan(_capi.FLAG_DENSE_SPLIT_LINE, 8, 8, 2, 8, 8)
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_DENSE_SPLIT_LINE excludes"):
        _plan(_line(_capi.FLAG_NO_DENSE_SPLIT), 8, 8, 2, 8, 8)
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_DENSE_SPLIT_LINE excludes"):
        _plan(_line(_capi.FLAG_IO_BF16 | _capi.FLAG_DENSE_BF16), 8, 8, 2, 8, 8)
    # fine together with ...
    for extra in (_capi.FLAG_DENSE_SPLIT_F16, _capi.FLAG_DENSE_SPLIT_OUTLIERS, _capi.FLAG_IO_F16, _capi.FLAG_IO_BF16, _capi.FLAG_IO_NHWC,
                  _capi.FLAG_INPUT_RELU, _capi.FLAG_UNIT_TESTING, _capi.FLAG_FORBID_POSITIVE_DIM1,
                  _capi.FLAG_DENSE_SPLIT_F16 | _capi.FLAG_IO_F16 | _capi.FLAG_IO_NHWC | _capi.FLAG_INPUT_RELU):
        _plan(_line(extra), 8, 8, 2, 8, 8)


@pytest.mark.parametrize("case", [
    # (S, F, G, H, W), k, forcing flag, bit 6, bit 7: today's split_pays formula evaluated with 9 and 17 taps, per padded pixel
    #   dense = Fp Sp taps 3 / 16 / 0.55 + 430 Sp against 1.1 x exact = 1.1 x 4 G F S (H W / Hp Wp) / (0.60, or 0.45 below 32 pixels)
    ((256, 256, 1, 56, 56), 9, False, True, False),
    ((256, 256, 1, 56, 56), 17, False, True, False),     # 17 taps: 7.47 >= 1.1 x 6.67 units per pixel and channel pair
    ((256, 256, 2, 56, 56), 17, False, True, True),
    ((7, 5, 4, 16, 16), 17, False, False, False),
    ((7, 5, 4, 16, 16), 17, True, True, True),
])
def test_held_members(case):
    from dau_conv import _capi
    shape, k, forced, want6, want7 = case
    extra = _capi.FLAG_DENSE_SPLIT_F16 if forced else 0
    on = _plan(_line(extra), *shape, k=k).info["gather_dense_split"]
    off = _plan(_single(extra), *shape, k=k).info["gather_dense_split"]
    assert bool(on & LINE4) == want6 and bool(on & LINE8) == want7, (case, bin(on))
    assert on & 0b111100 == off and not off & (LINE4 | LINE8), (case, bin(on), bin(off))      # bits 2..5 as without the flag


def test_radius_8_needs_a_kernel_that_reaches_it():
    from dau_conv import _capi
    for k, want in ((9, LINE4), (11, LINE4 | LINE8), (17, LINE4 | LINE8), (33, LINE4 | LINE8)):
        got = _plan(_line(_capi.FLAG_DENSE_SPLIT_F16), 16, 16, 2, 16, 16, k=k).info["gather_dense_split"]
        assert got & (LINE4 | LINE8) == want, (k, bin(got))
    # 16-bit activations and NHWC: the same members
    for io in (_capi.FLAG_IO_F16, _capi.FLAG_IO_BF16, _capi.FLAG_IO_NHWC):
        assert _plan(_line(io), 256, 256, 2, 56, 56, k=17).info["gather_dense_split"] & (LINE4 | LINE8) == LINE4 | LINE8
    # a prefilter support without a two-limb staging kernel (sigma 1.2: 13 taps): no line member
    assert _capi.Plan(2, 16, 16, 2, 16, 16, max_kernel_size=9, sigma_hint=1.2,
                      flags=_capi.FLAG_USE_INTERPOLATION | _line(_capi.FLAG_DENSE_SPLIT_F16)).info["gather_dense_split"] == 0


def test_the_flag_leaves_the_rest_of_the_plan_alone():
    from dau_conv import _capi
    for shape, k, extra in (((256, 256, 1, 56, 56), 9, 0), ((256, 256, 2, 56, 56), 17, 0), ((256, 256, 4, 56, 56), 9, 0),
                            ((20, 40, 3, 27, 27), 17, _capi.FLAG_DENSE_SPLIT_F16), ((7, 5, 4, 16, 16), 17, 0)):
        on, off = _plan(_line(extra), *shape, N=4, k=k), _plan(_single(extra), *shape, N=4, k=k)
        a, b = dict(on.info), dict(off.info)
        a["gather_dense_split"] &= ~(LINE4 | LINE8)
        assert a == b, (shape, a, b)
        for which in (_capi.PASS_FORWARD, _capi.PASS_BACKWARD, _capi.PASS_EPILOGUE_BACKWARD):
            assert on.workspace_bytes(which) >= off.workspace_bytes(which), (shape, which)
        assert on.epilogue_supported(_capi.EPILOGUE_BIAS | _capi.EPILOGUE_RELU) == off.epilogue_supported(_capi.EPILOGUE_BIAS | _capi.EPILOGUE_RELU)


def test_the_flag_is_inert_without_per_call_selection():
    from dau_conv import _capi
    for shape, k in (((256, 256, 2, 56, 56), 17), ((256, 256, 1, 56, 56), 9)):
        on, off = (_plan(f(_capi.FLAG_STATIC_BUCKET), *shape, k=k) for f in (_line, _single))
        assert on.info == off.info and not on.info["gather_dense_split"] & (LINE4 | LINE8)
        assert on.workspace_bytes(_capi.PASS_FORWARD) == off.workspace_bytes(_capi.PASS_FORWARD)
    on, off = (_capi.Plan(2, 8, 8, 4, 16, 16, flags=_capi.FLAG_USE_INTERPOLATION | f(), algo=_capi.ALGO_DIRECT).info for f in (_line, _single))
    assert on == off and on["gather_dense_split"] == 0


def test_layer_keyword_reaches_the_flag():
    import importlib
    import torch
    from dau_conv import _capi
    dc = importlib.import_module("dau_conv.dau_conv")
    dc._PLANS.clear()
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    x, w = torch.zeros(2, 128, 16, 16, device=dev), torch.zeros(1, 128, 2, 128, device=dev)
    st = lambda **kw: dc._settings(torch.full((1,), 0.5), num_output=128, kernel_size=17, single_dim_kernel=True, **kw)
    assert st()["dense_line"] is False and st(dense_line=1)["dense_line"] is True
    off, on = dc._get_plan(x, w, st()), dc._get_plan(x, w, st(dense_line=True))
    assert off is not on and len(dc._PLANS) == 2
    assert on.info["gather_dense_split"] == off.info["gather_dense_split"] | LINE4 | LINE8
    assert dc._get_plan(x, w, st(dense_line=True)) is on
    forced = dc._get_plan(x, w, st(dense_line=True, dense_split=True))
    assert forced.info["gather_dense_split"] == 0b11100 | LINE4 | LINE8
    dc._PLANS.clear()
    with pytest.raises(ValueError, match="single-dimension"):
        dc._settings(torch.full((1,), 0.5), dense_line=True)
    with pytest.raises(ValueError, match="dense_split=False"):
        st(dense_line=True, dense_split=False)
    with pytest.raises(ValueError, match="dense_bf16"):
        st(dense_line=True, dense_bf16=True)
    layer = dc.DAUConv1d(filters=8, dau_units=(2, 1), max_kernel_size=9, in_channels=4, dense_line=True)
    assert layer.dense_line is True and layer._dau_convolution_op.dense_line is True and layer.dau_unit_single_dim is True
    layer = dc.DAUConv2d(filters=8, dau_units=(2, 1), max_kernel_size=9, in_channels=4, dau_unit_single_dim=True, dense_line=True)
    assert layer.dense_line is True and layer._dau_convolution_op.dense_line is True
    assert dc.DAUConv1d(filters=8, dau_units=(2, 1), max_kernel_size=9, in_channels=4).dense_line is False
    with pytest.raises(ValueError, match="single-dimension"):
        dc.DAUConv2d(filters=8, dau_units=(2, 2), max_kernel_size=9, in_channels=4, dense_line=True)
    with pytest.raises(ValueError, match="dense_split=False"):
        dc.DAUConv1d(filters=8, dau_units=(2, 1), max_kernel_size=9, in_channels=4, dense_line=True, dense_split=False)


def test_dense_split_encoding_round_trips_through_the_ops():
    """The ops' trailing arguments are fixed: dense_line travels inside the integer dense_split (2, 3), and the shape functions do
    not depend on it."""
    import importlib
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from dau_conv import _capi, _ops
    dc = importlib.import_module("dau_conv.dau_conv")
    want = {(None, False): -1, (False, False): 0, (True, False): 1, (None, True): 2, (True, True): 3}
    sigma = torch.full((1,), 0.5)
    w = torch.zeros(1, 4, 2, 8)
    for (split, line), code in want.items():
        st = dc._settings(sigma, num_output=8, kernel_size=9, single_dim_kernel=True, dense_split=split, dense_line=line)
        enc = _ops.encode_settings(st)
        assert len(enc) == 13 and enc[9] == code, (split, line, enc)
        back = _ops._run_settings(w, sigma, False, *enc)
        assert back["dense_split"] is split and back["dense_line"] is line
        for key in st:
            if key != "sigma_hint":
                assert back[key] == st[key], key
    with pytest.raises(_capi.InvalidArgumentError, match="dense_split must be -1, 0, 1, 2 or 3"):
        _ops._run_settings(w, sigma, False, 0, 9, False, 1.0, True, False, True, 0, False, 4, False, -1, "async")
    with FakeTensorMode():
        x, wf = torch.empty(2, 4, 5, 24), torch.empty(1, 4, 2, 8)
        shapes = set()
        for code in (-1, 2, 3):
            y = torch.ops.dau_conv.conv(x, wf, wf, wf, torch.empty(1), None, None, False, False, 0, 9, False, 1.0, True, False, True, 0,
                                        False, code, False, -1, "async")
            shapes.add((tuple(y.shape), y.dtype, tuple(y.stride())))
        assert shapes == {((2, 8, 5, 24), torch.float32, (8 * 5 * 24, 5 * 24, 24, 1))}


# ---- the built code -------------------------------------------------------------------------------------------------------

def _line_kernels(funcs, which):
    return {sym: ins for sym, ins in funcs.items() if re.search(r"3dau2l[48]\d+%s" % which, sym)}


@pytest.mark.parametrize("ns", ["l4", "l8"])
def test_line_kernels_ship_and_use_no_scratch(release, ns):
    for which in ("line_gather_kernel", "line_densify_kernel", "line_stage_walk_kernel", "line_stage_kernel"):
        found = {s: i for s, i in _line_kernels(release, which).items() if "3dau2%s" % ns in s}
        assert found, (ns, which)
        for sym, ins in found.items():
            assert any(mn == "s_endpgm" for mn, _ in ins)
            if which in ("line_gather_kernel", "line_densify_kernel"):
                assert not [mn for mn, _ in ins if mn.startswith("scratch_")], _kernel_name(sym)


def test_release_library_reads_no_split_knob():
    assert b"DAU_SPLIT_" not in open(LIB, "rb").read()
