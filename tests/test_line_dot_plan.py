"""CPU: the opt-in line members of the two-limb gather-dot (DAU_FLAG_SPLIT_DOT_LINE; k_split_dot.hip compiled with a horizontal radius
of 4 / 8 and no vertical halo, namespaces d4 and d8) at plan level -- which plans hold them (dau_conv_plan_info.gather_dense_split
bits 8 and 9), which flag combinations are refused, the status query's declaration and export, how the layer keyword and the ops'
integer reach the flag -- and in the built gfx950 code: the d4 / d8 kernels (named line_dot_kernel, line_e1_dot_kernel, ld_*_kernel)
ship, use no scratch and fit the LDS.  Plan creation needs no device; nothing is launched here.  (GPU: tests/test_gpu_line_dot.py.)"""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

from test_built_code import LLVM, PKG, _code_objects, _kernel_name, release  # noqa: F401  (release: the fixture)
from test_capi_symbols import HEADER, LIB, declared_symbols

DOT4, DOT8 = 1 << 8, 1 << 9


def _plan(flags, S, F, G, H, W, N=2, k=9, **kw):
    from dau_conv import _capi
    return _capi.Plan(N, S, F, G, H, W, max_kernel_size=k, sigma_hint=0.5, flags=_capi.FLAG_USE_INTERPOLATION | flags, **kw)


def _single(extra=0):
    from dau_conv import _capi
    return _capi.FLAG_SINGLE_DIM_KERNEL | extra


def _dot(extra=0):
    from dau_conv import _capi
    return _capi.FLAG_SINGLE_DIM_KERNEL | _capi.FLAG_SPLIT_DOT_LINE | extra


def test_flag_value_and_query_are_declared_and_exported():
    from dau_conv import _capi
    src = open(HEADER).read()
    assert re.search(r"DAU_FLAG_SPLIT_DOT_LINE\s*=\s*1\s*<<\s*16\b", src) and _capi.FLAG_SPLIT_DOT_LINE == 1 << 16
    assert re.search(r"#define\s+DAU_CONV_ABI_VERSION\s+4\b", src)
    assert "dau_conv_dot_line_status" in declared_symbols()
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "dau_conv_dot_line_status")
    assert lib.dau_conv_abi_version() == 4
    lib.dau_conv_dot_line_status.argtypes = [ctypes.c_void_p] * 5
    assert lib.dau_conv_dot_line_status(None, None, None, None, None) == _capi.DAU_INVALID_ARGUMENT


def test_invalid_flag_combinations():
    from dau_conv import _capi
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_SPLIT_DOT_LINE needs DAU_FLAG_SINGLE_DIM_KERNEL"):
        _plan(_capi.FLAG_SPLIT_DOT_LINE, 8, 8, 2, 8, 8)
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_SPLIT_DOT_LINE needs DAU_FLAG_USE_INTERPOLATION"):
        _capi.Plan(2, 8, 8, 2, 8, 8, max_kernel_size=9, sigma_hint=0.5, flags=_dot())
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_SPLIT_DOT_LINE excludes"):
        _plan(_dot(_capi.FLAG_NO_DENSE_SPLIT), 8, 8, 2, 8, 8)
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_SPLIT_DOT_LINE excludes"):
        _plan(_dot(_capi.FLAG_IO_BF16 | _capi.FLAG_DENSE_BF16), 8, 8, 2, 8, 8)
    # fine together with ...
    for extra in (_capi.FLAG_DENSE_SPLIT_F16, _capi.FLAG_DENSE_SPLIT_LINE, _capi.FLAG_DENSE_SPLIT_OUTLIERS, _capi.FLAG_IO_F16, _capi.FLAG_IO_BF16,
                  _capi.FLAG_IO_NHWC, _capi.FLAG_INPUT_RELU, _capi.FLAG_UNIT_TESTING, _capi.FLAG_FORBID_POSITIVE_DIM1,
                  _capi.FLAG_DENSE_SPLIT_F16 | _capi.FLAG_DENSE_SPLIT_LINE | _capi.FLAG_IO_F16 | _capi.FLAG_IO_NHWC | _capi.FLAG_INPUT_RELU):
        _plan(_dot(extra), 8, 8, 2, 8, 8)


def test_held_members():
    from dau_conv import _capi
    forced = _dot(_capi.FLAG_DENSE_SPLIT_F16)
    # radius 8 only where the plan's offsets reach it (max_kernel_size >= 11)
    for k, want in ((9, DOT4), (11, DOT4 | DOT8), (17, DOT4 | DOT8), (33, DOT4 | DOT8)):
        got = _plan(forced, 16, 16, 2, 16, 16, k=k).info["gather_dense_split"]
        assert got & (DOT4 | DOT8) == want, (k, bin(got))
    # default plans: the fill rule of the 2-D member (three or four units of every block of four)
    for G, held in ((1, False), (2, False), (3, True), (4, True), (5, False), (7, True), (8, True)):
        got = _plan(_dot(), 32, 32, G, 20, 20, k=17).info["gather_dense_split"]
        assert got & (DOT4 | DOT8) == (DOT4 | DOT8 if held else 0), (G, bin(got))
    assert _plan(_dot(), 7, 5, 1, 16, 16, k=17).info["gather_dense_split"] & (DOT4 | DOT8) == 0
    assert _plan(forced, 7, 5, 4, 16, 16, k=17).info["gather_dense_split"] & (DOT4 | DOT8) == DOT4 | DOT8
    # 16-bit activations and NHWC: the same members
    for io in (_capi.FLAG_IO_F16, _capi.FLAG_IO_BF16, _capi.FLAG_IO_NHWC):
        assert _plan(_dot(io), 64, 64, 4, 28, 28, k=17).info["gather_dense_split"] & (DOT4 | DOT8) == DOT4 | DOT8
    # the bits say nothing about the gather-sum's line members, and those nothing about these
    both = _plan(forced | _capi.FLAG_DENSE_SPLIT_LINE, 16, 16, 2, 16, 16, k=17).info["gather_dense_split"]
    assert both == 0b11100 | (3 << 6) | DOT4 | DOT8, bin(both)
    # a gather-dot cut into batch slabs keeps the exact kernels
    os.environ["DAU_WORKSPACE_BUDGET_GB"] = "0.0000005"
    try:
        slabbed = _plan(forced, 16, 16, 2, 16, 16, N=4, k=17).info
    finally:
        del os.environ["DAU_WORKSPACE_BUDGET_GB"]
    assert slabbed["batch_slab_dot"] == 2 and not slabbed["gather_dense_split"] & (DOT4 | DOT8), slabbed


def test_the_flag_leaves_the_rest_of_the_plan_alone():
    from dau_conv import _capi
    for shape, k, extra in (((256, 256, 1, 56, 56), 9, 0), ((256, 256, 3, 56, 56), 17, 0), ((256, 256, 4, 56, 56), 9, 0),
                            ((20, 40, 3, 27, 27), 17, _capi.FLAG_DENSE_SPLIT_F16), ((7, 5, 4, 16, 16), 17, 0),
                            ((64, 64, 4, 28, 28), 17, _capi.FLAG_DENSE_SPLIT_LINE)):
        on, off = _plan(_dot(extra), *shape, N=4, k=k), _plan(_single(extra), *shape, N=4, k=k)
        a, b = dict(on.info), dict(off.info)
        a["gather_dense_split"] &= ~(DOT4 | DOT8)
        assert a == b, (shape, a, b)
        for which in (_capi.PASS_FORWARD, _capi.PASS_BACKWARD, _capi.PASS_EPILOGUE_BACKWARD):
            assert on.workspace_bytes(which) >= off.workspace_bytes(which), (shape, which)
        assert on.workspace_bytes(_capi.PASS_FORWARD) == off.workspace_bytes(_capi.PASS_FORWARD)
        assert on.epilogue_supported(_capi.EPILOGUE_BIAS | _capi.EPILOGUE_RELU) == off.epilogue_supported(_capi.EPILOGUE_BIAS | _capi.EPILOGUE_RELU)


def test_the_flag_is_inert_without_per_call_selection():
    from dau_conv import _capi
    for shape, k in (((256, 256, 4, 56, 56), 17), ((64, 64, 3, 28, 28), 9)):
        on, off = (_plan(f(_capi.FLAG_STATIC_BUCKET), *shape, k=k) for f in (_dot, _single))
        assert on.info == off.info and not on.info["gather_dense_split"] & (DOT4 | DOT8)
        for which in (_capi.PASS_FORWARD, _capi.PASS_BACKWARD):
            assert on.workspace_bytes(which) == off.workspace_bytes(which)
    on, off = (_capi.Plan(2, 8, 8, 4, 16, 16, flags=_capi.FLAG_USE_INTERPOLATION | f(), algo=_capi.ALGO_DIRECT) for f in (_dot, _single))
    assert on.info == off.info and on.info["gather_dense_split"] == 0
    for which in (_capi.PASS_FORWARD, _capi.PASS_BACKWARD):
        assert on.workspace_bytes(which) == off.workspace_bytes(which)


def test_layer_keyword_reaches_the_flag():
    import importlib
    import torch
    dc = importlib.import_module("dau_conv.dau_conv")
    dc._PLANS.clear()
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    x, w = torch.zeros(2, 128, 16, 16, device=dev), torch.zeros(1, 128, 4, 128, device=dev)
    st = lambda **kw: dc._settings(torch.full((1,), 0.5), num_output=128, kernel_size=17, single_dim_kernel=True, **kw)
    assert st()["dense_line_grads"] is False and st(dense_line_grads=1)["dense_line_grads"] is True
    off, on = dc._get_plan(x, w, st()), dc._get_plan(x, w, st(dense_line_grads=True))
    assert off is not on and len(dc._PLANS) == 2
    assert on.info["gather_dense_split"] == off.info["gather_dense_split"] | DOT4 | DOT8
    assert dc._get_plan(x, w, st(dense_line_grads=True)) is on
    both = dc._get_plan(x, w, st(dense_line=True, dense_line_grads=True, dense_split=True))
    assert both.info["gather_dense_split"] == 0b11100 | (3 << 6) | DOT4 | DOT8
    dc._PLANS.clear()
    with pytest.raises(ValueError, match="dense_line_grads=True needs a single-dimension"):
        dc._settings(torch.full((1,), 0.5), dense_line_grads=True)
    with pytest.raises(ValueError, match="dense_line_grads=True excludes dense_split=False"):
        st(dense_line_grads=True, dense_split=False)
    with pytest.raises(ValueError, match="dense_line_grads=True excludes dense_bf16"):
        st(dense_line_grads=True, dense_bf16=True)
    layer = dc.DAUConv1d(filters=8, dau_units=(2, 1), max_kernel_size=9, in_channels=4, dense_line_grads=True)
    assert layer.dense_line_grads is True and layer._dau_convolution_op.dense_line_grads is True and layer.dense_line is False
    layer = dc.DAUConv2d(filters=8, dau_units=(2, 1), max_kernel_size=9, in_channels=4, dau_unit_single_dim=True, dense_line_grads=True)
    assert layer.dense_line_grads is True and layer._dau_convolution_op.dense_line_grads is True
    assert dc.DAUConv1d(filters=8, dau_units=(2, 1), max_kernel_size=9, in_channels=4).dense_line_grads is False
    with pytest.raises(ValueError, match="single-dimension"):
        dc.DAUConv2d(filters=8, dau_units=(2, 2), max_kernel_size=9, in_channels=4, dense_line_grads=True)
    with pytest.raises(ValueError, match="dense_split=False"):
        dc.DAUConv1d(filters=8, dau_units=(2, 1), max_kernel_size=9, in_channels=4, dense_line_grads=True, dense_split=False)
    with pytest.raises(ValueError, match="dense_bf16"):
        dc.DAUConv1d(filters=8, dau_units=(2, 1), max_kernel_size=9, in_channels=4, dense_line_grads=True, dense_bf16=True)


def test_algo_encoding_round_trips_through_the_ops():
    """The ops' trailing arguments are fixed: dense_line_grads travels inside the integer algo (+ 16), and the shape functions do
    not depend on it."""
    import importlib
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from dau_conv import _capi, _ops
    dc = importlib.import_module("dau_conv.dau_conv")
    sigma = torch.full((1,), 0.5)
    w = torch.zeros(1, 4, 2, 8)
    for algo in (_capi.ALGO_AUTO, _capi.ALGO_DIRECT, _capi.ALGO_TILED):
        for grads in (False, True):
            for line in (False, True):
                st = dc._settings(sigma, num_output=8, kernel_size=9, single_dim_kernel=True, algo=algo, dense_line=line, dense_line_grads=grads)
                enc = _ops.encode_settings(st)
                assert len(enc) == 13 and enc[7] == algo + (16 if grads else 0), (algo, grads, enc)
                back = _ops._run_settings(w, sigma, False, *enc)
                assert back["algo"] == algo and back["dense_line_grads"] is grads and back["dense_line"] is line
                assert set(back) == set(st)
                for key in st:
                    if key != "sigma_hint":
                        assert back[key] == st[key], key
    with FakeTensorMode():
        x, wf = torch.empty(2, 4, 5, 24), torch.empty(1, 4, 2, 8)
        shapes = set()
        for algo in (0, 16):
            y = torch.ops.dau_conv.conv(x, wf, wf, wf, torch.empty(1), None, None, False, False, 0, 9, False, 1.0, True, False, True, algo,
                                        False, 2, False, -1, "async")
            shapes.add((tuple(y.shape), y.dtype, tuple(y.stride())))
            g = torch.ops.dau_conv.conv_backward(y, x, wf, wf, wf, torch.empty(1), None, False, False, _capi.NEED_ALL, False, 0, 9, False, 1.0,
                                                 True, False, True, algo, False, 2, False, -1, "async")
            shapes.add(tuple(tuple(t.shape) for t in g))
        assert len(shapes) == 2, shapes


# ---- the built code -------------------------------------------------------------------------------------------------------

KERNELS = ("line_dot_kernel", "line_e1_dot_kernel", "ld_xk_walk_kernel", "ld_stage_e_kernel", "ld_stage_e1_kernel", "ld_stage_nhwc_e_kernel",
           "ld_stage_x_kernel", "ld_absmax_e_kernel", "ld_absmax_nhwc_e_kernel")


def _notes(so):
    """{kernel symbol: (private segment bytes, static LDS bytes)} from the code objects' metadata"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in _code_objects(so, d):
            txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
            for blk in txt.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s*(\S+)", blk)
                get = lambda k: int(re.search(r"\.%s:\s*(\d+)" % k, blk)[1])
                if name:
                    out[name.group(1)] = (get("private_segment_fixed_size"), get("group_segment_fixed_size"))
    return out


@pytest.fixture(scope="module")
def notes():
    so = os.path.join(PKG, "libdau_conv_hip.so")
    if not os.path.exists(so):
        pytest.skip("library not built")
    return _notes(so)


@pytest.mark.parametrize("ns", ["d4", "d8"])
def test_line_dot_kernels_ship_use_no_scratch_and_fit_the_lds(release, notes, ns):
    radius = int(ns[1])
    for which in KERNELS:
        found = {s: i for s, i in release.items() if "3dau2%s" % ns in s and which in s}
        assert found, (ns, which)
        for sym, ins in found.items():
            assert any(mn == "s_endpgm" for mn, _ in ins)
            if which in ("line_dot_kernel", "line_e1_dot_kernel"):
                assert not [mn for mn, _ in ins if mn.startswith("scratch_")], _kernel_name(sym)
                assert any(mn.startswith("v_mfma_f32_16x16x32") for mn, _ in ins), _kernel_name(sym)
                private, lds = notes[sym]
                assert private == 0, (_kernel_name(sym), private)
                # the ring is dynamic LDS: 2 RH = 8 slots x (RW + 2 R) positions x 256 B per limb
                rw = int(re.search(r"dot_kernel<(\d+)>", _kernel_name(sym))[1])
                limbs = 1 if "e1" in which else 2
                assert rw in (10, 12) and lds + 8 * (rw + 2 * radius) * 256 * limbs <= 160 * 1024, (_kernel_name(sym), lds)
    main = [s for s in release if "3dau2%s" % ns in s and "line_dot_kernel" in s]
    assert len(main) == 2, [_kernel_name(s) for s in main]
    # the 2-D member's names count the 2-D member's kernels alone
    assert not [s for s in release if "3dau2%s" % ns in s and ("split_gather_dot_kernel" in s or "sd_" in s)]


def test_release_library_reads_no_split_dot_knob():
    blob = open(LIB, "rb").read()
    assert b"DAU_SD_" not in blob and b"DAU_DOT_" not in blob and b"DAU_SPLIT_" not in blob
