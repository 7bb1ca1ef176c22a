"""GPU: the error staging of the two-limb f16 gather-dot as a walking kernel (sd_stage_e_kernel, k_split_dot.hip).  A wave owns
(octet, block of 16 channels, tile of 16 window columns, band of window rows) and walks down the rows with the next row's loads in
flight, instead of one workgroup per window row whose load, LDS and store phases follow each other.  ES must be byte for byte what
the earlier kernels wrote, so the four parameter gradients of the shipped build must be BIT-IDENTICAL (0 differing words) to the
build that keeps the oldest staging (libdau_conv_hip_stage_ref.so of `make tuning`: -DDAU_SD_STAGE_REF, one thread per position),
and within the fp32 bar of the oracle.

Cases: the shapes of test_gpu_split_dot_stage_fused.py -- a ragged octet with a ragged channel block (region width 12), region
width 10, a 27x27 map, N = 11 with F = 40, a 90-wide map (104 window columns: seven column tiles, the last one of eight columns),
float16 activation I/O and the unit_testing edge rule (the dropped row and column).  Bands: the tuning build with
DAU_SD_STAGE_E_RB = 1, 3 and the whole window height (24 rows) against its default rule (bands of 4 rows at that size), so that
a band starts and another ends inside the 5-row halo.  An Inf in one plane of dy leaves the other output channels their bits; a
workspace full of 0xFF bytes gives the bits of a zeroed one (the halo, the absent images of the octet and the absent channels of
the block are stores of the kernel, not leftovers)."""
import numpy as np
import pytest

from oracle import dau_oracle as orc
from util import assert_parity, make_inputs, region_width, tuning_capi, variant_capi

pytestmark = pytest.mark.gpu

PARAMS = ("dw", "dmu1", "dmu2", "dsigma")
FIRST = (5, 20, 24, 3, 13, 22)


def _gradients(capi, tensors, extra=0, half=False, fill=None):
    import torch
    x, dy, w, mu1, mu2 = tensors
    N, S, H, W = x.shape
    G, F = w.shape[2:]
    plan = capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=0.5,
                     flags=capi.FLAG_USE_INTERPOLATION | capi.FLAG_DENSE_SPLIT_F16 | extra)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    act = lambda a: dev(a).half() if half else dev(a)
    sg = torch.full((1, S, G, F), 0.5, device="cuda")
    if fill is not None:
        plan._workspace(capi.PASS_BACKWARD, torch.device("cuda", torch.cuda.current_device())).fill_(fill)
    need = capi.NEED_DW | capi.NEED_DMU1 | capi.NEED_DMU2 | capi.NEED_DSIGMA
    g = plan.backward(act(x), act(dy), dev(w), dev(mu1), dev(mu2), sg, need_mask=need)
    plan.check_status()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in zip(("dx",) + PARAMS, g) if k in PARAMS}


def _inputs(seed, shape):
    N, S, F, G, H, W = shape
    x, dy, w, mu1, mu2 = make_inputs(seed, N, S, F, G, H, W, 9, 3.0)
    mu1.flat[0] = 3.0; mu2.flat[0] = -3.0; mu1.flat[1] = -3.0; mu2.flat[1] = 3.0
    return x, dy, w, mu1, mu2


def _assert_same_bits(name, new, ref, pick=lambda a: a):
    for key in PARAMS:
        a, b = np.ascontiguousarray(pick(new[key])), np.ascontiguousarray(pick(ref[key]))
        differ = int((a.view(np.uint32) != b.view(np.uint32)).sum())
        print("%s/%s: %d of %d words differ" % (name, key, differ, a.size))
        assert differ == 0, "%s/%s: %d words differ" % (name, key, differ)


CASES = [
    # name, (N, S, F, G, H, W), region width, extra plan flags (names of _capi), float16 activations
    ("ragged", FIRST, 12, (), False),
    ("width-10", (9, 16, 32, 2, 11, 27), 10, (), False),
    ("27x27", (6, 12, 16, 4, 27, 27), 10, (), False),
    ("ragged-N-F", (11, 8, 40, 2, 9, 14), 10, (), False),
    ("seven-column-tiles", (2, 4, 16, 2, 6, 90), 12, (), False),
    ("f16-io", FIRST, 12, ("FLAG_IO_F16",), True),
    ("edge-rule", FIRST, 12, ("FLAG_UNIT_TESTING",), False),
]


@pytest.mark.parametrize("name,shape,rw,flag_names,half", CASES, ids=[c[0] for c in CASES])
def test_walking_staging_is_bit_identical_to_the_oldest_staging(name, shape, rw, flag_names, half):
    from dau_conv import _capi
    assert region_width(shape[5]) == rw
    x, dy, w, mu1, mu2 = _inputs(1801 + rw, shape)
    if half:                                       # the oracle sees the values the kernels see
        x, dy = x.astype(np.float16).astype(np.float32), dy.astype(np.float16).astype(np.float32)
    ref_capi = variant_capi("stage_ref")
    tensors = (x, dy, w, mu1, mu2)
    new = _gradients(_capi, tensors, sum(getattr(_capi, f) for f in flag_names), half)
    ref = _gradients(ref_capi, tensors, sum(getattr(ref_capi, f) for f in flag_names), half)
    want = orc.backward(x, dy, w, mu1, mu2, 0.5, need=PARAMS, unit_testing="FLAG_UNIT_TESTING" in flag_names)
    _assert_same_bits(name, new, ref)
    for key in PARAMS:
        assert_parity(new[key], want[key], "stage-e-walk/" + name + "/" + key)


@pytest.fixture(scope="module")
def first_default():
    """the tuning build under its default band rule on the first shape (13 rows: a window of 24 rows in bands of 4)"""
    tensors = _inputs(1821, FIRST)
    return tensors, _gradients(tuning_capi(), tensors)


@pytest.mark.parametrize("rb", (1, 3, 24))
def test_band_length_does_not_change_a_bit(rb, first_default, monkeypatch):
    """bands of 1 and 3 window rows and one band of the whole height (13 + 1 rows padded to 16, plus the halo of 2 x 4): bands that
    start and end inside the halo, inside the image and on the padding below it"""
    tensors, default = first_default
    monkeypatch.setenv("DAU_SD_STAGE_E_RB", str(rb))
    got = _gradients(tuning_capi(), tensors)
    _assert_same_bits("rb-%d" % rb, got, default)


def test_the_tuning_build_is_the_release_on_the_first_shape(first_default):
    """(what the band cases compare with is what ships)"""
    from dau_conv import _capi
    tensors, default = first_default
    _assert_same_bits("release", _gradients(_capi, tensors), default)


def test_an_inf_in_one_plane_of_dy_leaves_the_other_output_channels_bit_identical():
    """the scale of a channel comes from its finite values; the Inf's own channel is the reference's too, word for word"""
    from dau_conv import _capi
    x, dy, w, mu1, mu2 = _inputs(1811, FIRST)
    clean = _gradients(_capi, (x, dy, w, mu1, mu2))
    dy = dy.copy()
    dy[1, 5, 3, 3] = np.inf
    new = _gradients(_capi, (x, dy, w, mu1, mu2))
    ref = _gradients(variant_capi("stage_ref"), (x, dy, w, mu1, mu2))
    _assert_same_bits("inf", new, ref)
    fs = [f for f in range(FIRST[2]) if f != 5]
    _assert_same_bits("inf-others", new, clean, pick=lambda a: a[..., fs])
    for key in PARAMS:
        assert np.all(np.isfinite(new[key][..., fs])), key
    assert not np.all(np.isfinite(new["dw"][..., 5]))


def test_every_staged_byte_the_main_kernel_reads_is_written():
    """the workspace full of 0xFF bytes before the call against a zeroed one"""
    from dau_conv import _capi
    tensors = _inputs(1831, FIRST)
    poisoned = _gradients(_capi, tensors, fill=0xFF)
    zeroed = _gradients(_capi, tensors, fill=0)
    for key in PARAMS:
        assert np.all(np.isfinite(poisoned[key])), key
    _assert_same_bits("poisoned-workspace", poisoned, zeroed)
