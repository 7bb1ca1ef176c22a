"""CPU: the opt-in radius-3 + ring gather-sum member (DAU_FLAG_DENSE_SPLIT_OUTLIERS; k_dense_ring.hip) at plan level -- which plans
hold it (dau_conv_plan_info.gather_dense_split bit 5), which flag combinations are refused, the status query's declaration and
export -- and in the built gfx950 code: the list and pass kernels are there, spill nothing, and the release library reads no
tuning knob for them.  Plan creation needs no device; nothing is launched here.  (GPU: tests/test_gpu_dense_outliers.py.)"""
import ctypes
import re

import pytest

from test_built_code import _kernel_name, release  # noqa: F401  (release: the fixture)
from test_capi_symbols import HEADER, LIB, declared_symbols

RING = 1 << 5
NS = (256, 256, 4, 56, 56)      # S, F, G, H, W of the north-star layer


def _info(flags, S, F, G, H, W, N=2, **kw):
    from dau_conv import _capi
    return _capi.Plan(N, S, F, G, H, W, max_kernel_size=kw.pop("k", 9), sigma_hint=0.5, flags=_capi.FLAG_USE_INTERPOLATION | flags, **kw).info


def test_forced_plans_hold_the_ring_member():
    from dau_conv import _capi
    for shape in ((7, 5, 1, 16, 16), (20, 40, 3, 27, 27), (16, 130, 4, 28, 28), (33, 16, 6, 20, 100)):
        on = _info(_capi.FLAG_DENSE_SPLIT_F16 | _capi.FLAG_DENSE_SPLIT_OUTLIERS, *shape)["gather_dense_split"]
        off = _info(_capi.FLAG_DENSE_SPLIT_F16, *shape)["gather_dense_split"]
        assert on & RING, (shape, bin(on))
        assert off == 0b11100 and on == off | RING, (shape, bin(on), bin(off))       # bits 2..4 as without the flag


def test_default_plans_hold_it_where_they_hold_radius_3():
    from dau_conv import _capi
    assert _info(_capi.FLAG_DENSE_SPLIT_OUTLIERS, *NS)["gather_dense_split"] == 0b11100 | RING
    assert _info(0, *NS)["gather_dense_split"] == 0b11100
    # float16 / bfloat16 activations: the same members
    for io in (_capi.FLAG_IO_F16, _capi.FLAG_IO_BF16):
        assert _info(io | _capi.FLAG_DENSE_SPLIT_OUTLIERS, *NS)["gather_dense_split"] == 0b11100 | RING
        assert _info(io, *NS)["gather_dense_split"] == 0b11100
    # a larger kernel: the member serves the calls within +-4 of any plan
    assert _info(_capi.FLAG_DENSE_SPLIT_OUTLIERS, *NS, k=17)["gather_dense_split"] == 0b11100 | RING
    # plans whose radius-3 member does not pay (split_pays) have no ring member either; bits 2..4 never move
    for shape in ((256, 256, 2, 56, 56), (256, 256, 1, 56, 56), (7, 5, 4, 16, 16), (64, 64, 2, 56, 56)):
        off = _info(0, *shape)["gather_dense_split"]
        assert not off & (1 << 3) and _info(_capi.FLAG_DENSE_SPLIT_OUTLIERS, *shape)["gather_dense_split"] == off, shape
    assert _info(_capi.FLAG_DENSE_SPLIT_OUTLIERS, 96, 256, 4, 27, 27)["gather_dense_split"] == 0b01100 | RING


def test_the_flag_is_inert_without_per_call_selection():
    from dau_conv import _capi
    on, off = (_info(_capi.FLAG_STATIC_BUCKET | f, *NS) for f in (_capi.FLAG_DENSE_SPLIT_OUTLIERS, 0))
    assert on == off and on["gather_dense_split"] == 0
    on, off = (_capi.Plan(2, 8, 8, 4, 16, 16, flags=_capi.FLAG_USE_INTERPOLATION | f, algo=_capi.ALGO_DIRECT).info
               for f in (_capi.FLAG_DENSE_SPLIT_OUTLIERS, 0))
    assert on == off and on["gather_dense_split"] == 0


def test_the_flag_leaves_the_rest_of_the_plan_alone():
    """Everything dau_conv_plan_info reports but bit 5 is the flag-off plan's; the workspace grows by the list and the partial sums
    (gather-sum passes only), and only where the member is held."""
    from dau_conv import _capi
    I = _capi.FLAG_USE_INTERPOLATION
    for shape, extra in ((NS, 0), ((20, 40, 3, 27, 27), _capi.FLAG_DENSE_SPLIT_F16), ((7, 5, 4, 16, 16), 0)):
        S, F, G, H, W = shape
        on = _capi.Plan(4, S, F, G, H, W, sigma_hint=0.5, flags=I | extra | _capi.FLAG_DENSE_SPLIT_OUTLIERS)
        off = _capi.Plan(4, S, F, G, H, W, sigma_hint=0.5, flags=I | extra)
        a, b = dict(on.info), dict(off.info)
        held = bool(a["gather_dense_split"] & RING)
        a["gather_dense_split"] &= ~RING
        assert a == b, shape
        for which in (_capi.PASS_FORWARD, _capi.PASS_BACKWARD):
            grow = on.workspace_bytes(which) - off.workspace_bytes(which)
            assert (grow >= 0 if held else grow == 0), (shape, which, grow)
        if held:
            # forward: at least the fp32 partial sums of the slab fit behind the radius-3 form's workspace
            assert on.workspace_bytes(_capi.PASS_FORWARD) >= 4 * 4 * F * H * W


def test_invalid_flag_combinations():
    from dau_conv import _capi
    I = _capi.FLAG_USE_INTERPOLATION
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_DENSE_SPLIT_OUTLIERS excludes"):
        _capi.Plan(2, 8, 8, 2, 8, 8, flags=I | _capi.FLAG_DENSE_SPLIT_OUTLIERS | _capi.FLAG_NO_DENSE_SPLIT)
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_DENSE_SPLIT_OUTLIERS excludes"):
        _capi.Plan(2, 8, 8, 2, 8, 8, flags=I | _capi.FLAG_DENSE_SPLIT_OUTLIERS | _capi.FLAG_IO_BF16 | _capi.FLAG_DENSE_BF16)
    # fine together with the forcing flag and with 16-bit activations
    for extra in (_capi.FLAG_DENSE_SPLIT_F16, _capi.FLAG_IO_BF16, _capi.FLAG_IO_F16, _capi.FLAG_DENSE_SPLIT_F16 | _capi.FLAG_IO_F16):
        _capi.Plan(2, 8, 8, 2, 8, 8, flags=I | _capi.FLAG_DENSE_SPLIT_OUTLIERS | extra)


def test_flag_value_and_query_are_declared_and_exported():
    from dau_conv import _capi
    src = open(HEADER).read()
    assert re.search(r"DAU_FLAG_DENSE_SPLIT_OUTLIERS\s*=\s*1\s*<<\s*12\b", src) and _capi.FLAG_DENSE_SPLIT_OUTLIERS == 1 << 12
    assert re.search(r"#define\s+DAU_CONV_ABI_VERSION\s+4\b", src)
    assert "dau_conv_gather_outlier_status" in declared_symbols()
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "dau_conv_gather_outlier_status")
    # the query validates its arguments like dau_conv_check_status
    lib.dau_conv_gather_outlier_status.argtypes = [ctypes.c_void_p] * 5
    assert lib.dau_conv_gather_outlier_status(None, None, None, None, None) == _capi.DAU_INVALID_ARGUMENT


def test_layer_keyword_reaches_the_plan_key():
    import importlib
    import torch
    from dau_conv import _capi
    dc = importlib.import_module("dau_conv.dau_conv")
    dc._PLANS.clear()
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    x, w = torch.zeros(2, 128, 16, 16, device=dev), torch.zeros(1, 128, 4, 128, device=dev)
    st = lambda **kw: dc._settings(torch.full((1,), 0.5), num_output=128, kernel_size=9, **kw)
    off, on = dc._get_plan(x, w, st()), dc._get_plan(x, w, st(dense_outliers=True))
    assert off is not on and len(dc._PLANS) == 2
    assert on.info["gather_dense_split"] == off.info["gather_dense_split"] | RING == 0b11100 | RING
    assert dc._get_plan(x, w, st(dense_outliers=True)) is on
    # where the split members are switched off the keyword is inert (the library would refuse the combination)
    never = dc._get_plan(x, w, st(dense_outliers=True, dense_split=False))
    assert never.info["gather_dense_split"] == 0
    dc._PLANS.clear()
    for cls in (dc.DAUConv2d, dc.DAUConv1d):
        layer = cls(filters=8, dau_units=(2, 1), max_kernel_size=9, in_channels=4, dense_outliers=True)
        assert layer.dense_outliers is True and layer._dau_convolution_op.dense_outliers is True
    assert dc.DAUConv2d(filters=8, dau_units=(2, 2), max_kernel_size=9, in_channels=4).dense_outliers is False
    assert _capi.FLAG_DENSE_SPLIT_OUTLIERS == 4096


# ---- the built code -------------------------------------------------------------------------------------------------------

def _ring(funcs):
    return {sym: ins for sym, ins in funcs.items() if re.search(r"ring_(pass|pairs|scan)_kernel", sym)}


def test_ring_kernels_ship(release):
    names = sorted(re.sub(r"\(.*", "", _kernel_name(s)) for s in _ring(release))
    assert len(names) == 4, names
    for want in ("ring_pass_kernel", "ring_pairs_kernel<false>", "ring_pairs_kernel<true>", "ring_scan_kernel"):
        assert any(want in n for n in names), (want, names)


def test_ring_kernels_use_no_scratch(release):
    for sym, ins in _ring(release).items():
        assert not [mn for mn, _ in ins if mn.startswith("scratch_")], _kernel_name(sym)
        assert any(mn == "s_endpgm" for mn, _ in ins)
    # the pass reads its wave-uniform entry stream lane by lane and its pixels from LDS
    (ins,) = [i for s, i in _ring(release).items() if "ring_pass_kernel" in s]
    assert any(mn == "v_readlane_b32" for mn, _ in ins) and any(mn.startswith("ds_read") for mn, _ in ins)
    assert not [mn for mn, _ in ins if "atomic_add" in mn or "atomic_fadd" in mn]       # no atomics on results


def test_the_added_partial_epilogue_is_an_instantiation_of_its_own(release):
    """split_gather_kernel<NSUB, RG, TT, H16, ADD = true> exists for radius 3 only; the instantiations without it are still there."""
    names = [_kernel_name(s) for s in release if "split_gather_kernel" in s]
    add = [n for n in names if re.search(r"split_gather_kernel<\d+, \d+, (true|false), (true|false), true>", n)]
    plain = [n for n in names if re.search(r"split_gather_kernel<\d+, \d+, (true|false), (true|false), false>", n)]
    assert add and all("dau::s3::" in n for n in add), add
    for ns in ("s2", "s3", "s4"):
        assert [n for n in plain if "dau::%s::" % ns in n], ns
    assert len([n for n in plain if "dau::s3::" in n]) == len(add)


def test_release_library_reads_no_ring_knob():
    blob = open(LIB, "rb").read()
    assert b"DAU_RING" not in blob
    assert b"DAU_RING_LIMIT_PERMILLE" in open(LIB.replace("libdau_conv_hip.so", "libdau_conv_hip_tuning.so"), "rb").read()
