"""GPU: the staging of the two-limb f16 dense gather-sum (k_dense_split.hip).  NCHW plans write the staged limb planes with
split_stage_walk_kernel -- a wave walks down the rows of (image, group of 8 channels, tile of staged columns), the filtered rows in
a register ring, the zero border out of the same masked code path -- instead of split_stage_kernel, whose workgroups load, filter
and store one band in three phases.  Both passes run the sums in the same order, so y and dx must be BIT-IDENTICAL (0 differing
words) to the build that keeps split_stage_kernel for every plan (libdau_conv_hip_split_stage_ref.so of `make tuning`:
-DDAU_SPLIT_STAGE_REF).  NHWC plans keep the old kernel in both builds (the fallback case).

Cases, the smallest at which each part can go wrong: ragged channel groups in both directions on an odd map with one partial column
tile; a 90-wide map (two column tiles); the flagship geometry at depth 16 (several bands of rows); 27x27 and 28x28 (tiles of at
most 32 columns: each half wave takes four channels; tall tiles and the block of four rows downstream); prefilter supports 5, 7, 9
and 11; offsets within 2, 3 and 3.99 (the three radii's members); f16 and bf16 activations; an activation base that is 4-byte
but not 16-byte aligned; an Inf and a NaN; a workspace full of 0xFF bytes (every staged byte that is read is written by the call);
a pass cut into batch slabs; the radius-3 + ring member, whose ring pass reads the staged planes too."""
import os

import numpy as np
import pytest

from util import make_inputs, variant_capi, variant_lib

pytestmark = pytest.mark.gpu

RAGGED = (3, 9, 5, 3, 13, 11)
FLAGSHIP16 = (2, 16, 16, 4, 56, 56)


def _partner():
    if not os.path.exists(variant_lib("split_stage_ref")):
        pytest.skip("libraries not built")
    return variant_capi("split_stage_ref")


def _inputs(seed, shape, radius=3.0):
    N, S, F, G, H, W = shape
    x, dy, w, mu1, mu2 = make_inputs(seed, N, S, F, G, H, W, 9, radius)
    c = min(radius, 3.99)
    mu1.flat[0] = c; mu2.flat[0] = -c; mu1.flat[1] = -c; mu2.flat[1] = c      # the call belongs to that radius' member
    return x, dy, w, mu1, mu2


def _gather(capi, tensors, sigma=0.5, extra=(), support=7, fill=None, budget=None, offset=0, ring=False):
    """y and dx (numpy, the activations' bits) of one forward and one dx-only backward call.  extra: names of plan flags; fill:
    byte both workspaces hold before; budget: DAU_WORKSPACE_BUDGET_GB at plan creation; offset: elements the activations' bases
    lie behind a 16-byte boundary"""
    import torch
    x, dy, w, mu1, mu2 = tensors
    N, S, H, W = x.shape
    G, F = w.shape[2:]
    flags = capi.FLAG_USE_INTERPOLATION | capi.FLAG_DENSE_SPLIT_F16 | sum(getattr(capi, f) for f in extra)
    old = os.environ.get("DAU_WORKSPACE_BUDGET_GB")
    if budget is not None:
        os.environ["DAU_WORKSPACE_BUDGET_GB"] = budget
    try:
        plan = capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=sigma, flags=flags)
    finally:
        if budget is not None:
            if old is None:
                del os.environ["DAU_WORKSPACE_BUDGET_GB"]
            else:
                os.environ["DAU_WORKSPACE_BUDGET_GB"] = old
    assert plan.info["blur_support"] == support, plan.info
    assert plan.info["gather_dense_split"] == (0b111100 if ring else 0b11100), plan.info
    if budget is not None:
        assert plan.info["batch_slab_gather"] < N, plan.info
    dtype = torch.float16 if "FLAG_IO_F16" in extra else torch.bfloat16 if "FLAG_IO_BF16" in extra else torch.float32
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def act(a):
        t = dev(a).to(dtype)
        if "FLAG_IO_NHWC" in extra:
            return t.contiguous(memory_format=torch.channels_last)
        if not offset:
            return t.contiguous()
        buf = torch.empty(t.numel() + 64, dtype=dtype, device="cuda")
        first = (-buf.data_ptr() % 16) // buf.element_size() + offset
        view = buf[first:first + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 != 0 and view.data_ptr() % 4 == 0
        return view
    sg = torch.full((1, S, G, F), float(sigma), device="cuda")
    if fill is not None:
        for p in (capi.PASS_FORWARD, capi.PASS_BACKWARD):
            plan._workspace(p, torch.device("cuda", torch.cuda.current_device())).fill_(fill)
    xd, dyd, wd, m1, m2 = act(x), act(dy), dev(w), dev(mu1), dev(mu2)
    y = plan.forward(xd, wd, m1, m2, sg)
    plan.check_status()
    if ring:
        assert plan.outlier_status() == (1, True)
    dx = plan.backward(xd, dyd, wd, m1, m2, sg, need_mask=capi.NEED_DX)[0]
    plan.check_status()
    torch.cuda.synchronize()
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    return {k: v.contiguous().view(bits).cpu().numpy() for k, v in (("y", y), ("dx", dx))}, \
           {k: v.float().cpu().numpy() for k, v in (("y", y), ("dx", dx))}


def _assert_same_bits(name, new, ref):
    for key in ("y", "dx"):
        differ = int((new[key] != ref[key]).sum())
        print("%s/%s: %d of %d words differ" % (name, key, differ, new[key].size))
        assert new[key].shape == ref[key].shape and differ == 0, "%s/%s: %d words differ" % (name, key, differ)


CASES = [
    # name, (N, S, F, G, H, W), sigma, prefilter support, offset radius, extra plan flags
    ("ragged", RAGGED, 0.5, 7, 3.0, ()),
    ("two-column-tiles", (2, 8, 16, 2, 6, 90), 0.5, 7, 3.0, ()),
    ("flagship-geometry", FLAGSHIP16, 0.5, 7, 3.0, ()),
    ("27x27", (2, 16, 16, 2, 27, 27), 0.5, 7, 3.0, ()),
    ("28x28", (2, 16, 16, 2, 28, 28), 0.5, 7, 3.0, ()),
    ("support-5", RAGGED, 0.4, 5, 3.0, ()),
    ("support-9", RAGGED, 0.8, 9, 3.0, ()),
    ("support-11", RAGGED, 1.0, 11, 3.0, ()),
    ("support-5-28x28", (2, 16, 16, 2, 28, 28), 0.4, 5, 3.0, ()),
    ("support-11-flagship-geometry", FLAGSHIP16, 1.0, 11, 3.0, ()),
    ("radius-2", RAGGED, 0.5, 7, 2.0, ()),
    ("radius-4", RAGGED, 0.5, 7, 3.99, ()),
    ("radius-2-28x28", (2, 16, 16, 2, 28, 28), 0.5, 7, 2.0, ()),
    ("radius-4-flagship-geometry", FLAGSHIP16, 0.5, 7, 3.99, ()),
    ("f16-io", RAGGED, 0.5, 7, 3.0, ("FLAG_IO_F16",)),
    ("bf16-io", RAGGED, 0.5, 7, 3.0, ("FLAG_IO_BF16",)),
    ("f16-io-28x28", (2, 16, 16, 2, 28, 28), 0.5, 7, 3.0, ("FLAG_IO_F16",)),
    ("nhwc-fallback", RAGGED, 0.5, 7, 3.0, ("FLAG_IO_NHWC",)),
]


@pytest.mark.parametrize("name,shape,sigma,support,radius,extra", CASES, ids=[c[0] for c in CASES])
def test_the_walking_staging_is_bit_identical_to_the_banded_one(name, shape, sigma, support, radius, extra):
    from dau_conv import _capi
    partner = _partner()
    tensors = _inputs(1701 + support + int(radius * 100), shape, radius)
    new, val = _gather(_capi, tensors, sigma, extra, support)
    ref, _ = _gather(partner, tensors, sigma, extra, support)
    for key in ("y", "dx"):
        assert np.all(np.isfinite(val[key])) and np.abs(val[key]).max() > 0, key
    _assert_same_bits(name, new, ref)


@pytest.mark.parametrize("io", [(), ("FLAG_IO_F16",)], ids=["f32", "f16"])
def test_an_activation_base_that_is_not_16_byte_aligned(io):
    """x and dy begin 4 bytes behind a 16-byte boundary (rows of 11 elements: no row is aligned either)"""
    from dau_conv import _capi
    partner = _partner()
    tensors = _inputs(1711, RAGGED)
    offset = 2 if io else 1
    new, val = _gather(_capi, tensors, extra=io, offset=offset)
    ref, _ = _gather(partner, tensors, extra=io, offset=offset)
    aligned, _ = _gather(_capi, tensors, extra=io)
    assert np.all(np.isfinite(val["y"])) and np.all(np.isfinite(val["dx"]))
    _assert_same_bits("unaligned", new, ref)
    _assert_same_bits("unaligned-vs-aligned", new, aligned)


def test_an_inf_and_a_nan():
    """an Inf in image 0 and a NaN in image 2 of x and of dy, near a corner and at the last column: every word, the non-finite
    ones included, is the banded kernel's; image 1 stays finite"""
    from dau_conv import _capi
    partner = _partner()
    x, dy, w, mu1, mu2 = _inputs(1721, RAGGED)
    x[0, 3, 1, 0] = np.inf; dy[0, 2, 1, 0] = np.inf
    x[2, 8, 12, 10] = np.nan; dy[2, 4, 12, 10] = np.nan
    new, val = _gather(_capi, (x, dy, w, mu1, mu2))
    ref, _ = _gather(partner, (x, dy, w, mu1, mu2))
    _assert_same_bits("non-finite", new, ref)
    for key in ("y", "dx"):
        assert np.all(np.isfinite(val[key][1])), key
        assert not np.all(np.isfinite(val[key][0])) and not np.all(np.isfinite(val[key][2])), key


@pytest.mark.parametrize("shape", [RAGGED, (2, 16, 16, 2, 28, 28)], ids=["ragged", "28x28"])
def test_every_staged_byte_that_is_read_is_written(shape):
    """both workspaces full of 0xFF bytes before the calls against zeroed ones: the zero border around the maps, the rows and
    columns that pad the planes to whole tiles and the absent channels of the ragged last group are stores of the walking kernel"""
    from dau_conv import _capi
    tensors = _inputs(1731, shape)
    poisoned, val = _gather(_capi, tensors, fill=0xFF)
    zeroed, _ = _gather(_capi, tensors, fill=0)
    for key in ("y", "dx"):
        assert np.all(np.isfinite(val[key])), key
    _assert_same_bits("poisoned-workspace", poisoned, zeroed)


def test_a_pass_cut_into_batch_slabs():
    from dau_conv import _capi
    partner = _partner()
    shape = (4, 16, 32, 4, 24, 24)
    tensors = _inputs(1741, shape)
    new, _ = _gather(_capi, tensors, budget="0.0005")
    ref, _ = _gather(partner, tensors, budget="0.0005")
    whole, _ = _gather(_capi, tensors)
    _assert_same_bits("slabbed", new, ref)
    _assert_same_bits("slabbed-vs-whole", new, whole)


def test_the_ring_member_reads_the_same_staged_planes():
    """dense_outliers: offsets within 3 and one unit at 3.5 -- the radius-3 GEMM and the ring pass both read the staged planes"""
    from dau_conv import _capi
    partner = _partner()
    shape = (4, 16, 32, 4, 24, 24)
    x, dy, w, mu1, mu2 = _inputs(1751, shape)
    mu1.flat[3] = 3.5
    new, val = _gather(_capi, (x, dy, w, mu1, mu2), extra=("FLAG_DENSE_SPLIT_OUTLIERS",), ring=True)
    ref, _ = _gather(partner, (x, dy, w, mu1, mu2), extra=("FLAG_DENSE_SPLIT_OUTLIERS",), ring=True)
    assert np.all(np.isfinite(val["y"])) and np.all(np.isfinite(val["dx"]))
    _assert_same_bits("ring", new, ref)
