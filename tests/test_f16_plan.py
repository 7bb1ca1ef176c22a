"""CPU: float16 activation I/O (DAU_FLAG_IO_F16) at plan creation, which needs no device.  An f16 plan must be the fp32 plan of
the same desc in everything but its loads and stores: the same buckets, windows, tilings, batch slabs and dense members (the
split gather radii and the split gather-dot), so every dau_conv_plan_info field is equal, and it needs no more workspace."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dau_conv.h")

I = 1 << 0          # DAU_FLAG_USE_INTERPOLATION


def test_flag_value_in_python_and_header():
    from dau_conv import _capi
    assert _capi.FLAG_IO_F16 == 1 << 11
    m = re.search(r"DAU_FLAG_IO_F16\s*=\s*1\s*<<\s*(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == 11
    assert _capi.lib.dau_conv_abi_version() == 4          # additive: the ABI version stays


def test_plan_io_dtype_is_float16():
    import torch
    from dau_conv import _capi
    assert _capi.Plan(2, 4, 8, 2, 16, 16, flags=I | _capi.FLAG_IO_F16).io_dtype == torch.float16


@pytest.mark.parametrize("extra, why", [
    ("FLAG_IO_BF16", "two storage formats"),
    ("FLAG_DENSE_BF16", "the bf16-product dense form"),
    ("FLAG_DENSE_WGRAD_NEVER", "a qualifier of the bf16 dense form"),
    ("FLAG_DENSE_WGRAD_ALWAYS", "a qualifier of the bf16 dense form"),
])
def test_rejected_combinations(extra, why):
    from dau_conv import _capi
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_IO_F16"):
        _capi.Plan(2, 8, 8, 4, 16, 16, flags=I | _capi.FLAG_IO_F16 | getattr(_capi, extra))


def test_needs_the_tiled_kernels():
    from dau_conv import _capi
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_IO_F16 needs the tiled kernels"):
        _capi.Plan(2, 4, 8, 2, 16, 16, flags=I | _capi.FLAG_IO_F16, algo=_capi.ALGO_DIRECT)
    # a shape the tiled kernels refuse (17 units per channel pair under a kernel larger than 17: no gather-dot tiling), where an
    # fp32 plan falls back to the direct kernels
    fp32 = _capi.Plan(2, 2, 2, 18, 16, 16, max_kernel_size=65, flags=I)
    assert _capi.ALGO_DIRECT in (fp32.info["algo_forward"], fp32.info["algo_backward"])
    with pytest.raises(_capi.InvalidArgumentError, match="DAU_FLAG_IO_F16 needs the tiled kernels"):
        _capi.Plan(2, 2, 2, 18, 16, 16, max_kernel_size=65, flags=I | _capi.FLAG_IO_F16)


# (N, S, F, G, H, W, max_kernel_size, extra flags)
DESCS = [
    (2, 256, 256, 4, 56, 56, 9, ()),                          # north-star shape: split gather radii 2-4 and the split gather-dot
    (2, 96, 256, 4, 27, 27, 9, ()),                           # C1
    (2, 64, 64, 1, 32, 32, 9, ()),                            # G = 1: no dense member
    (2, 128, 128, 2, 28, 28, 9, ()),                          # G = 2: radius 2 only
    (2, 256, 256, 3, 28, 28, 9, ()),                          # G = 3: blocks of four 3/4 full: split gather-dot
    (2, 256, 256, 6, 56, 56, 9, ()),                          # G = 6
    (2, 32, 48, 4, 40, 72, 17, ()),                           # bucket 8
    (4, 16, 24, 4, 33, 20, 65, ()),                           # bucket 32: offset windows, seven bucket sets
    (2, 256, 256, 4, 56, 56, 9, ("FLAG_NO_DENSE_SPLIT",)),
    (2, 256, 256, 4, 56, 56, 65, ("FLAG_STATIC_BUCKET",)),
    (2, 7, 5, 1, 16, 16, 9, ("FLAG_DENSE_SPLIT_F16",)),
    (2, 8, 16, 4, 24, 24, 9, ("FLAG_UNIT_TESTING",)),
]


@pytest.mark.parametrize("desc", DESCS, ids=lambda d: "%dx%d->%d_G%d_%dx%d_k%d%s" % (d[1], d[4], d[2], d[3], d[5], d[4], d[6], "".join("_" + f[5:] for f in d[7])))
def test_f16_plan_equals_the_fp32_plan(desc):
    from dau_conv import _capi
    N, S, F, G, H, W, k, extra = desc
    flags = I
    for f in extra:
        flags |= getattr(_capi, f)
    p32 = _capi.Plan(N, S, F, G, H, W, max_kernel_size=k, sigma_hint=0.5, flags=flags)
    p16 = _capi.Plan(N, S, F, G, H, W, max_kernel_size=k, sigma_hint=0.5, flags=flags | _capi.FLAG_IO_F16)
    assert p16.info == p32.info
    assert p32.info["algo_forward"] == _capi.ALGO_TILED and p32.info["algo_backward"] == _capi.ALGO_TILED
    for which in (_capi.PASS_FORWARD, _capi.PASS_BACKWARD):
        assert p16.workspace_bytes(which) <= p32.workspace_bytes(which)
        assert p16.workspace_bytes(which) == p32.workspace_bytes(which)      # the same members (the split gather-dot included)


def test_the_descs_cover_the_dense_members():
    """the parametrised comparison above sees plans with and without the split gather radii (and a split gather-dot)"""
    from dau_conv import _capi
    infos = [_capi.Plan(N, S, F, G, H, W, max_kernel_size=k, sigma_hint=0.5, flags=I | _capi.FLAG_IO_F16).info
             for N, S, F, G, H, W, k, extra in DESCS if not extra]
    splits = {i["gather_dense_split"] for i in infos}
    assert 0b11100 in splits and 0 in splits and 0b00100 in splits
    assert any(i["dot_windows"] > 1 for i in infos)
