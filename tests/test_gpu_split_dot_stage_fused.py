"""GPU: the staging of the two-limb f16 gather-dot (k_split_dot.hip).  max |Xk| per (input channel, kind) is taken inside
blur4_pack_kernel (per wave, one atomicMax per kind) instead of by a pass of its own over XK, and sd_stage_e_kernel writes ES
through an LDS transpose (loads along x, stores as whole runs) instead of one thread per 512-byte position.  A maximum does not
depend on the order it is taken in and the staged bytes are the same, so the four parameter gradients of the shipped build must be
BIT-IDENTICAL (0 differing words) to the build that keeps the earlier staging (libdau_conv_hip_stage_ref.so of `make tuning`:
-DDAU_SD_STAGE_REF), and both within the fp32 bar of the oracle.  Cases: the two shapes of test_gpu_split_dot_staging.py (region
widths 12 and 10), a 27x27 map (several windows per workgroup in blur4_pack), N not a multiple of 8 with F not a multiple of 16,
a map wider than one column tile of the new sd_stage_e_kernel, float16 activation I/O, the unit_testing edge rule, and an Inf in
one input channel of x and one output channel of dy (the maxima are taken over finite values only: every other channel pair
keeps its bits)."""
import numpy as np
import pytest

from oracle import dau_oracle as orc
from util import assert_parity, make_inputs, region_width, variant_capi

pytestmark = pytest.mark.gpu

PARAMS = ("dw", "dmu1", "dmu2", "dsigma")


def _gradients(capi, x, dy, w, mu1, mu2, extra=0, half=False):
    import torch
    N, S, H, W = x.shape
    G, F = w.shape[2:]
    plan = capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=0.5,
                     flags=capi.FLAG_USE_INTERPOLATION | capi.FLAG_DENSE_SPLIT_F16 | extra)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    act = lambda a: dev(a).half() if half else dev(a)
    sg = torch.full((1, S, G, F), 0.5, device="cuda")
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


def _compare(name, new, ref, want, pick=lambda a: a):
    for key in PARAMS:
        a, b = np.ascontiguousarray(pick(new[key])), np.ascontiguousarray(pick(ref[key]))
        differ = int((a.view(np.uint32) != b.view(np.uint32)).sum())
        print("%s/%s: %d of %d words differ from the earlier staging" % (name, key, differ, a.size))
        assert differ == 0, "%s/%s: %d words differ" % (name, key, differ)
        assert_parity(a, pick(want[key]), name + "/" + key)


CASES = [
    # name, (N, S, F, G, H, W), region width, extra plan flags (names of _capi), float16 activations
    ("ragged", (5, 20, 24, 3, 13, 22), 12, (), False),
    ("width-10", (9, 16, 32, 2, 11, 27), 10, (), False),
    ("27x27", (6, 12, 16, 4, 27, 27), 10, (), False),
    ("ragged-N-F", (11, 8, 40, 2, 9, 14), 10, (), False),
    ("two-column-tiles", (2, 4, 16, 2, 6, 90), 12, (), False),
    ("f16-io", (5, 20, 24, 3, 13, 22), 12, ("FLAG_IO_F16",), True),
    ("edge-rule", (5, 20, 24, 3, 13, 22), 12, ("FLAG_UNIT_TESTING",), False),
]


@pytest.mark.parametrize("name,shape,rw,flag_names,half", CASES, ids=[c[0] for c in CASES])
def test_fused_staging_is_bit_identical_to_the_earlier_staging(name, shape, rw, flag_names, half):
    from dau_conv import _capi
    assert region_width(shape[5]) == rw
    x, dy, w, mu1, mu2 = _inputs(801 + rw, shape)
    if half:                                       # the oracle sees the values the kernels see
        x, dy = x.astype(np.float16).astype(np.float32), dy.astype(np.float16).astype(np.float32)
    ref_capi = variant_capi("stage_ref")
    new = _gradients(_capi, x, dy, w, mu1, mu2, sum(getattr(_capi, f) for f in flag_names), half)
    ref = _gradients(ref_capi, x, dy, w, mu1, mu2, sum(getattr(ref_capi, f) for f in flag_names), half)
    want = orc.backward(x, dy, w, mu1, mu2, 0.5, need=PARAMS, unit_testing="FLAG_UNIT_TESTING" in flag_names)
    _compare(name, new, ref, want)


def test_an_inf_leaves_the_other_channel_pairs_bit_identical():
    """Inf in input channel 3 of x (its Xk planes hold Inf and NaN) and in output channel 5 of dy: the finite-only maxima keep
    the scales, and with them the bits, of every unit whose input channel is not 3 and whose output channel is not 5"""
    from dau_conv import _capi
    shape = (5, 20, 24, 3, 13, 22)
    x, dy, w, mu1, mu2 = _inputs(811, shape)
    x[2, 3, 6, 9] = np.inf
    dy[1, 5, 3, 3] = np.inf
    new = _gradients(_capi, x, dy, w, mu1, mu2)
    ref = _gradients(variant_capi("stage_ref"), x, dy, w, mu1, mu2)
    with np.errstate(invalid="ignore", over="ignore"):
        want = orc.backward(x, dy, w, mu1, mu2, 0.5, need=PARAMS)
    ss = [s for s in range(shape[1]) if s != 3]
    fs = [f for f in range(shape[2]) if f != 5]
    _compare("inf", new, ref, want, pick=lambda a: a[:, ss][..., fs])
