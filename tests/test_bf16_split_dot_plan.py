"""CPU: bfloat16 plans (DAU_FLAG_IO_BF16) hold the split gather-dot (k_split_dot.hip) under exactly the fp32 rule, in its
one-limb-error form: the staged error ES1 is half of the fp32 plan's ES, everything else of the member's workspace is equal.
Plan creation needs no device.  The geometry of sd_geom is mirrored here.

A plan's workspace is the maximum over its members, so the member shows in it only where it is the largest: it is at
(128, 256, 256, 4, 56, 56) and at (64, 256, 256, 3, 28, 28), and it is not at (2, 256, 256, 3, 28, 28), where the exact
gather-dot's own staging is larger in the fp32 plan too (its default and NO_DENSE_SPLIT workspaces are equal).  That shape keeps
the two relations in the form that can hold there (not smaller than NO_DENSE_SPLIT, not larger than fp32); the batch of 64 of
the same layer carries the strict ones."""
import pytest

I = 1 << 0          # DAU_FLAG_USE_INTERPOLATION


def _es_limb_bytes(N, S, F, G, H, W):
    """one limb of the staged error window: octs * nfb * EYs * EXs * 256 bytes (sd_geom, split_dot_configure's region width)"""
    best, best_cost = 0, None
    for rw in (12, 10):
        wq = -(-(W + 1) // rw) * rw
        cost = wq * (rw + 2) * (60 // rw)
        if best_cost is None or cost < best_cost:
            best, best_cost = rw, cost
    hq = -(-(H + 1) // 4) * 4
    wq = -(-(W + 1) // best) * best
    return -(-N // 8) * -(-F // 16) * (hq + 8) * (wq + 8) * 256


def _bwd(shape, flags, **kw):
    from dau_conv import _capi
    return _capi.Plan(*shape, max_kernel_size=kw.pop("k", 9), sigma_hint=0.5, flags=flags, **kw).workspace_bytes(_capi.PASS_BACKWARD)


@pytest.mark.parametrize("shape", [(128, 256, 256, 4, 56, 56), (64, 256, 256, 3, 28, 28)], ids=lambda s: "N%d_G%d_%dx%d" % (s[0], s[3], s[4], s[5]))
def test_bf16_plan_holds_the_member_with_a_one_limb_error(shape):
    from dau_conv import _capi
    bf16 = _bwd(shape, I | _capi.FLAG_IO_BF16)
    exact = _bwd(shape, I | _capi.FLAG_IO_BF16 | _capi.FLAG_NO_DENSE_SPLIT)
    fp32 = _bwd(shape, I)
    limb = _es_limb_bytes(*shape)
    print("%s: bf16 %d, bf16 NO_DENSE_SPLIT %d, fp32 %d, one limb of ES %d" % (shape, bf16, exact, fp32, limb))
    assert bf16 > exact
    assert bf16 < fp32
    assert abs((fp32 - bf16) - limb) <= 256, (fp32 - bf16, limb)         # the layout rounds each part up to 256 bytes


def test_bf16_plan_of_a_small_batch_is_bounded_by_its_neighbours():
    """the issue's second shape: the exact gather-dot's staging is the plan's largest member here, with and without the split"""
    from dau_conv import _capi
    shape = (2, 256, 256, 3, 28, 28)
    bf16 = _bwd(shape, I | _capi.FLAG_IO_BF16)
    assert _bwd(shape, I | _capi.FLAG_IO_BF16 | _capi.FLAG_NO_DENSE_SPLIT) <= bf16 <= _bwd(shape, I)
    assert _bwd(shape, I) == _bwd(shape, I | _capi.FLAG_NO_DENSE_SPLIT)   # (why no strict relation can hold here)


@pytest.mark.parametrize("name, shape, extra, interp", [
    ("G1", (128, 256, 256, 1, 56, 56), (), True),
    ("G2", (128, 256, 256, 2, 56, 56), (), True),
    ("G5", (128, 256, 256, 5, 56, 56), (), True),
    ("single-dim", (128, 256, 256, 4, 56, 56), ("FLAG_SINGLE_DIM_KERNEL",), True),
    ("no-interpolation", (128, 256, 256, 4, 56, 56), (), False),
    ("dense-bf16", (128, 256, 256, 4, 56, 56), ("FLAG_DENSE_BF16",), True),
])
def test_no_member_where_the_fp32_plan_has_none(name, shape, extra, interp):
    from dau_conv import _capi
    flags = (I if interp else 0) | _capi.FLAG_IO_BF16
    for f in extra:
        flags |= getattr(_capi, f)
    assert _bwd(shape, flags) == _bwd(shape, flags | _capi.FLAG_NO_DENSE_SPLIT)
    if "FLAG_DENSE_BF16" not in extra:                  # (DENSE_BF16 needs IO_BF16: there is no fp32 plan of that desc)
        # the fp32 plan of the same desc has no split gather-dot either
        f32 = flags & ~_capi.FLAG_IO_BF16
        assert _bwd(shape, f32) == _bwd(shape, f32 | _capi.FLAG_NO_DENSE_SPLIT)


def test_forced_split_gives_one_unit_the_member():
    from dau_conv import _capi
    shape = (128, 256, 256, 1, 56, 56)
    forced = _bwd(shape, I | _capi.FLAG_IO_BF16 | _capi.FLAG_DENSE_SPLIT_F16)
    assert forced > _bwd(shape, I | _capi.FLAG_IO_BF16)
    fp32 = _bwd(shape, I | _capi.FLAG_DENSE_SPLIT_F16)
    assert abs((fp32 - forced) - _es_limb_bytes(*shape)) <= 256


# the parent commit's values: nothing but the backward workspace of a bf16 plan changes
PARENT = {
    (128, 256, 256, 4, 56, 56): (727720192, {
        'offset_bucket': 4, 'blur_support': 7, 'algo_forward': 2, 'algo_backward': 2, 'drop_last_col': 0, 'drop_last_row': 0,
        'gather_patch': 56, 'gather_stack': 1, 'dot_windows': 1, 'gather_windows': 1, 'bucket_sets': 1, 'gather_dense_bf16': 0,
        'batch_slab_gather': 128, 'batch_slab_dot': 128, 'dot_region': 808, 'gather_fblock': 4, 'gather_variant': 0,
        'dense_bf16_radius3': 0, 'gather_dense_split': 28}),
    (2, 256, 256, 3, 28, 28): (31990016, {
        'offset_bucket': 4, 'blur_support': 7, 'algo_forward': 2, 'algo_backward': 2, 'drop_last_col': 0, 'drop_last_row': 0,
        'gather_patch': 16, 'gather_stack': 1, 'dot_windows': 1, 'gather_windows': 1, 'bucket_sets': 1, 'gather_dense_bf16': 0,
        'batch_slab_gather': 2, 'batch_slab_dot': 2, 'dot_region': 1404, 'gather_fblock': 4, 'gather_variant': 3,
        'dense_bf16_radius3': 0, 'gather_dense_split': 12}),
}


@pytest.mark.parametrize("shape", sorted(PARENT), ids=lambda s: "N%d_G%d" % (s[0], s[3]))
def test_forward_workspace_and_info_are_the_parents(shape):
    from dau_conv import _capi
    fwd, info = PARENT[shape]
    p = _capi.Plan(*shape, max_kernel_size=9, sigma_hint=0.5, flags=I | _capi.FLAG_IO_BF16)
    assert p.workspace_bytes(_capi.PASS_FORWARD) == fwd
    assert p.info == info
    assert _capi.lib.dau_conv_abi_version() == 4
