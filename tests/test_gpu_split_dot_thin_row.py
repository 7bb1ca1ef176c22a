"""GPU: thin items of the two-limb f16 gather-dot (k_split_dot.hip, sd_dot_body).  Where (H + 1) % 4 == 1 -- every map whose height
is a multiple of four -- the last region of a column strip holds ONE real row of the K space, and that item takes the row's columns
four at a time as the K groups of an MFMA: ceil(RW / 4) = 3 K steps instead of RW.  Everything goes through the C ABI and is held to
the project's bar against the CPU oracle (util.assert_parity: 1e-4 relative + 1e-6 of the max-norm) on the four parameter gradients:
  * shapes with one full region plus the thin one (RW = 12), the masked third K step of RW = 10, two regions of 10 (columns 10 and
    11 of the first belong to the second) and two regions of 12; ragged S, F and partial image octets; offsets up to +-3.99 with
    units at the extremes (+-3.99 and +-4: the edge rows and columns of the error window);
  * isolating inputs: x non-zero only in its last row (all of it goes through the thin items) or only in its first row -- a thin row
    that is lost, shifted or counted twice fails by orders of magnitude;
  * a bfloat16 plan (the one-limb kernel) and an NHWC plan;
  * against libdau_conv_hip_no_thin.so (`make tuning`, -DDAU_SD_NO_THIN: every item full): bit-identical where no strip ends in a
    single row (H = 7, H = 6), within the bar of each other where one does (the last row's products are grouped otherwise inside
    an MFMA, and products that are exactly zero are dropped);
  * CPU: the K steps per strip the plan reports (dau_conv_split_dot_geometry)."""
import functools

import numpy as np
import pytest

from oracle import dau_oracle as orc
from util import assert_parity, make_inputs, margins, parity_error, region_width, tuning_capi, variant_capi

PARAMS = ("dw", "dmu1", "dmu2", "dsigma")

# name -> ((N, S, F, G, H, W), region width, regions per strip)
SHAPES = {
    "h4_w11_rw12": ((3, 3, 5, 4, 4, 11), 12, 2),          # one full region plus the thin one; one region column
    "h8_w9_rw10": ((8, 18, 20, 4, 8, 9), 10, 3),          # the masked third K step
    "h12_w19_rw10x2": ((9, 3, 20, 4, 12, 19), 10, 4),     # two region columns of 10: columns 10, 11 of the first are the second's
    "h16_w23_rw12x2": ((3, 18, 5, 4, 16, 23), 12, 5),     # two region columns of 12
}


def _flags(capi, extra=0):
    return capi.FLAG_USE_INTERPOLATION | capi.FLAG_DENSE_SPLIT_F16 | extra


@functools.lru_cache(maxsize=None)
def _case(name, only_row=None):
    """inputs (offsets up to +-3.99, the first units at the window's extremes) and the oracle's gradients, computed once"""
    (N, S, F, G, H, W), rw, _ = SHAPES[name]
    x, dy, w, mu1, mu2 = make_inputs(4100 + H + W, N, S, F, G, H, W, 9, 3.99)
    for i, (a, b) in enumerate(((3.99, -3.99), (-3.99, 3.99), (4.0, 4.0), (-4.0, -4.0), (-4.0, 4.0), (3.99, 3.99))):
        mu1.flat[i] = a; mu2.flat[i] = b
    if only_row is not None:
        keep = x[:, :, only_row].copy()
        x[:] = 0.0
        x[:, :, only_row] = keep
    want = orc.backward(x, dy, w, mu1, mu2, 0.5, need=PARAMS)
    for a in (x, dy, w, mu1, mu2) + tuple(want[k] for k in PARAMS):
        a.setflags(write=False)
    return (x, dy, w, mu1, mu2), want


def _gradients(capi, inputs, extra=0, dtype=None):
    import torch
    x, dy, w, mu1, mu2 = inputs
    N, S, H, W = x.shape
    G, F = w.shape[2:]
    plan = capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=0.5, flags=_flags(capi, extra))
    fmt = torch.channels_last if plan.io_layout == "NHWC" else torch.contiguous_format
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()             # (a copy: the shared cases are read-only)
    act = lambda a: dev(a).to(dtype or torch.float32).contiguous(memory_format=fmt)
    sg = torch.full((1, S, G, F), 0.5, device="cuda")
    need = capi.NEED_DW | capi.NEED_DMU1 | capi.NEED_DMU2 | capi.NEED_DSIGMA
    g = plan.backward(act(x), act(dy), dev(w), dev(mu1), dev(mu2), sg, need_mask=need)
    plan.check_status()
    torch.cuda.synchronize()
    return plan, {k: v.cpu().numpy() for k, v in zip(("dx",) + PARAMS, g) if k in PARAMS}


def _check(name, got, want):
    print("%s: max|got - want| / max|want| = %s" % (name, {k: "%.2e" % v for k, v in margins(got, {k: want[k] for k in PARAMS}).items()}))
    for key in PARAMS:
        assert_parity(got[key], want[key], name + "/" + key)


def _thin_geometry(plan, rw, regions):
    assert plan.split_dot_geometry() == (rw, regions, (regions - 1) * rw + 3)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_thin_row_shapes_meet_the_oracle(name):
    shape, rw, regions = SHAPES[name]
    assert region_width(shape[5]) == rw
    inputs, want = _case(name)
    plan, got = _gradients(tuning_capi(), inputs)
    _thin_geometry(plan, rw, regions)
    _check(name, got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("row", [-1, 0], ids=["last-row", "first-row"])
@pytest.mark.parametrize("name", ["h8_w9_rw10", "h12_w19_rw10x2", "h16_w23_rw12x2"])
def test_x_in_one_row_only(name, row):
    """x non-zero only in its last row: every product that reaches the gradients belongs to the strips' thin items (K row t = H)
    or to the d = 1 corner of row t = H - 1; only in its first row: the thin items contribute nothing."""
    inputs, want = _case(name, only_row=row)
    assert all(np.abs(want[k]).max() > 0 for k in ("dw", "dmu1", "dmu2"))
    _, got = _gradients(tuning_capi(), inputs)
    _check("%s/row%d" % (name, row), got, want)


@pytest.mark.gpu
def test_bf16_plan_takes_the_thin_item_of_the_one_limb_kernel():
    import torch
    capi = tuning_capi()
    (x, dy, w, mu1, mu2), _ = _case("h8_w9_rw10")
    rnd = lambda a: torch.from_numpy(np.array(a)).to(torch.bfloat16).float().numpy()
    xb, dyb = rnd(x), rnd(dy)
    want = orc.backward(xb, dyb, w, mu1, mu2, 0.5, need=PARAMS)
    plan, got = _gradients(capi, (xb, dyb, w, mu1, mu2), extra=capi.FLAG_IO_BF16, dtype=torch.bfloat16)
    _thin_geometry(plan, 10, 3)
    _check("bf16", got, want)


@pytest.mark.gpu
def test_nhwc_plan_takes_the_thin_item():
    capi = tuning_capi()
    inputs, want = _case("h8_w9_rw10")
    plan, got = _gradients(capi, inputs, extra=capi.FLAG_IO_NHWC)
    assert plan.io_layout == "NHWC"
    _thin_geometry(plan, 10, 3)
    _check("nhwc", got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("H, W", [(7, 11), (6, 9)], ids=["h7_rw12", "h6_rw10"])
def test_shapes_without_a_thin_row_are_bit_identical_to_the_no_thin_build(H, W):
    N, S, F, G = 9, 18, 20, 4
    x, dy, w, mu1, mu2 = make_inputs(4200 + H, N, S, F, G, H, W, 9, 3.99)
    mu1.flat[0] = 3.99; mu2.flat[0] = -3.99; mu1.flat[1] = -4.0; mu2.flat[1] = 4.0
    plan, got = _gradients(tuning_capi(), (x, dy, w, mu1, mu2))
    ref_plan, ref = _gradients(variant_capi("no_thin"), (x, dy, w, mu1, mu2))
    rw, regions = region_width(W), -(-(H + 1) // 4)
    assert plan.split_dot_geometry() == ref_plan.split_dot_geometry() == (rw, regions, regions * rw)
    for key in PARAMS:
        differ = int((got[key].view(np.uint32) != ref[key].view(np.uint32)).sum())
        print("H%d/%s: %d of %d values differ from the no_thin build" % (H, key, differ, got[key].size))
        assert differ == 0, (key, differ)
    want = orc.backward(x, dy, w, mu1, mu2, 0.5, need=PARAMS)
    _check("H%d/no_thin" % H, ref, want)                      # the reference itself is right


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["h8_w9_rw10", "h16_w23_rw12x2"])
def test_thin_shapes_stay_within_the_bar_of_the_no_thin_build(name):
    shape, rw, regions = SHAPES[name]
    inputs, want = _case(name)
    _, got = _gradients(tuning_capi(), inputs)
    ref_plan, ref = _gradients(variant_capi("no_thin"), inputs)
    assert ref_plan.split_dot_geometry() == (rw, regions, regions * rw)
    _check(name + "/no_thin", ref, want)
    for key in PARAMS:
        differ = int((got[key].view(np.uint32) != ref[key].view(np.uint32)).sum())
        viol = parity_error(got[key], ref[key])
        print("%s/%s: %d of %d values differ from the no_thin build, bar violated by %.3e (<= 0: within)" % (name, key, differ, got[key].size, viol))
        assert viol <= 0, (key, viol)


def test_k_steps_per_strip():
    """CPU (plan creation needs no device): 14 full items and a thin one per strip at the north-star shape, 171 K steps instead of
    180; a map without a single-row last region keeps RW steps per item; the release library and the no_thin build."""
    from dau_conv import _capi
    I = _capi.FLAG_USE_INTERPOLATION
    geo = lambda capi, *shape, flags=I | _capi.FLAG_DENSE_SPLIT_F16: capi.Plan(*shape, max_kernel_size=9, sigma_hint=0.5, flags=flags).split_dot_geometry()
    assert geo(_capi, 128, 256, 256, 4, 56, 56, flags=I) == (12, 15, 14 * 12 + 3)          # the default plan
    assert geo(_capi, 128, 256, 256, 4, 56, 56, flags=I | _capi.FLAG_IO_BF16) == (12, 15, 14 * 12 + 3)
    assert geo(_capi, 32, 512, 512, 4, 28, 28) == (10, 8, 7 * 10 + 3)            # C3
    assert geo(_capi, 32, 96, 256, 4, 27, 27) == (10, 7, 7 * 10)                 # C1: (H + 1) % 4 == 0
    assert geo(_capi, 2, 16, 32, 4, 13, 22) == (12, 4, 4 * 12)                   # two real rows in the last region
    assert geo(_capi, 2, 16, 32, 4, 14, 22) == (12, 4, 4 * 12)                   # three
    assert geo(_capi, 2, 16, 32, 4, 56, 56, flags=I | _capi.FLAG_NO_DENSE_SPLIT) == (0, 0, 0)
    no_thin = variant_capi("no_thin")
    assert geo(no_thin, 128, 256, 256, 4, 56, 56, flags=I) == (12, 15, 15 * 12)
