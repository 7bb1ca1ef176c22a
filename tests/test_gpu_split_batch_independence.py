"""GPU: the two-limb f16 dense gather-sum members (k_dense_split.hip, radii 2 / 3 / 4, and the radius-3 + ring member of
k_dense_ring.hip) scale every IMAGE by its own power of two, taken from the image's largest finite |value|: y[n] and dx[n] are a
function of image n and the parameters alone.  What this file pins down:
  1. an image's bits do not change with its batch-mates (fp32, bf16 and f16 activations);
  2. every image of a batch whose magnitudes differ by 2^20 (2^27) meets the fp32 bar against the oracle, each judged against its
     OWN max-norm (util.assert_parity defaults: 1e-4 relative + 1e-6 of the max-norm; margins via util.record_margins);
  3. a non-finite element (or an image without a finite value) stays inside its image, and inside it reaches only the outputs whose
     taps touch it.  In the dense form an output multiplies EVERY tap of its (2R+1)^2 kernel with the blurred input, taps of weight
     zero included (0 * Inf = NaN), so the footprint of an element is the box of half-width (prefilter radius + R) around it;
  4. a pass cut into batch slabs (DAU_WORKSPACE_BUDGET_GB) gives the bits of the whole-batch pass;
  5. the maxima do not depend on the load path (vector loads from an image's first aligned address, scalar head and tail).
Replaces the same reference code as the exact gather (dau_conv_forward_core.hpp:804-1605)."""
import numpy as np
import pytest
import torch

from oracle import dau_oracle as orc
from util import assert_parity, make_inputs, record_margins

pytestmark = pytest.mark.gpu

BAR = "1e-4 rel + 1e-6 of the image's own max-norm (fp32 bar; per-image limb scales)"
SHAPES = [
    dict(N=4, S=16, F=32, G=4, H=24, W=24),
    dict(N=3, S=7, F=5, G=2, H=9, W=6),           # tiny and ragged: image bases 7 * 9 * 6 elements apart (misaligned), a single tile
    dict(N=2, S=16, F=16, G=2, H=12, W=14),       # 8 + 4 rows
]
RADII = [2, 3, 4]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
KR = 3                                             # prefilter radius at sigma 0.5 (7 taps)
_ids = dict(ids=lambda s: "%dx%dx%d" % (s["N"], s["H"], s["W"]))


def _dims(shape):
    return tuple(shape[q] for q in ("N", "S", "F", "G", "H", "W"))


def _plan(shape, io="f32", ring=False):
    from dau_conv import _capi
    flags = _capi.FLAG_USE_INTERPOLATION | _capi.FLAG_DENSE_SPLIT_F16
    flags |= {"f32": 0, "bf16": _capi.FLAG_IO_BF16, "f16": _capi.FLAG_IO_F16}[io]
    if ring:
        flags |= _capi.FLAG_DENSE_SPLIT_OUTLIERS
    plan = _capi.Plan(*_dims(shape), max_kernel_size=9, sigma_hint=0.5, flags=flags)
    assert plan.info["gather_dense_split"] == (0b111100 if ring else 0b11100)
    return plan


def _inputs(seed, shape, radius, ring=False):
    """x ~ U[0,1), dy ~ N(0,1), offsets within +-radius with a corner offset planted (the call belongs to that radius' member);
    ring: offsets within +-3 and one unit at 3.5 (the radius-3 + ring member's call)"""
    N, S, F, G, H, W = _dims(shape)
    r = 3.0 if ring else float(radius)
    x, dy, w, mu1, mu2 = make_inputs(seed, N, S, F, G, H, W, 9, r)
    c = min(r, 3.99)
    mu1.flat[0] = c; mu2.flat[0] = -c; mu1.flat[1] = -c; mu2.flat[1] = c
    if ring:
        mu1.flat[3] = 3.5
    else:
        assert max(np.abs(mu1).max(), np.abs(mu2).max()) > radius - 1
    return x, dy, w, mu1, mu2


def _gather(plan, x, dy, w, mu1, mu2, io="f32", ring=False):
    """the two gather-sum passes -> dict(y, dx) as CPU tensors of the plan's activation type"""
    from dau_conv import _capi
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    S, G, F = w.shape[1:]
    sg = torch.full((1, S, G, F), 0.5, device="cuda")
    xd, dyd = dev(x).to(DTYPES[io]), dev(dy).to(DTYPES[io])
    wd, m1, m2 = dev(w), dev(mu1), dev(mu2)
    y = plan.forward(xd, wd, m1, m2, sg)
    plan.check_status()
    if ring:
        assert plan.outlier_status() == (1, True)
    dx = plan.backward(xd, dyd, wd, m1, m2, sg, need_mask=_capi.NEED_DX)[0]
    plan.check_status()
    if ring:
        assert plan.outlier_status() == (1, True)
    return dict(y=y.cpu(), dx=dx.cpu())


def _same_bits(a, b):
    view = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def _f32(t):
    return t.float().numpy()


def _mixed_batch(seed, shape, radius, io, exp=20, ring=False):
    """call A: a batch of one magnitude; call B: image 0 kept, the others replaced by other data `2^exp` times as large (f16
    activations: image 0 below 2^-6, the others up to 2^14)"""
    x, dy, w, mu1, mu2 = _inputs(seed, shape, radius, ring)
    x2, dy2 = make_inputs(seed + 500, *_dims(shape), 9, 3.0)[:2]
    if io == "f16":
        small_x, big_x, small_dy, big_dy = 2.0 ** -6, 2.0 ** 14, 2.0 ** -9, 2.0 ** 11      # |dy| < 8
    else:
        small_x = small_dy = 1.0
        big_x = big_dy = 2.0 ** exp
    xa, dya = x * np.float32(small_x), dy * np.float32(small_dy)
    xb, dyb = xa.copy(), dya.copy()
    xb[1:] = x2[1:] * np.float32(big_x)
    dyb[1:] = dy2[1:] * np.float32(big_dy)
    return (xa, dya), (xb, dyb), (w, mu1, mu2)


# ---------------------------------------------------------------------------------------------- 1. bitwise batch invariance
@pytest.mark.parametrize("io", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_an_images_bits_do_not_depend_on_its_batch_mates(shape, radius, io):
    a, b, par = _mixed_batch(61 + radius, shape, radius, io)
    plan = _plan(shape, io)
    ga, gb = _gather(plan, *a, *par, io=io), _gather(plan, *b, *par, io=io)
    for key in ("y", "dx"):
        assert torch.isfinite(ga[key][0]).all() and ga[key][0].abs().max() > 0, key
        assert _same_bits(ga[key][0], gb[key][0]), "%s[0] changes with the other images of the batch" % key


# ---------------------------------------------------------------------------------------------- 2. per-image parity
@pytest.mark.parametrize("exp", [20, 27])
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_every_image_meets_the_bar_against_its_own_max_norm(shape, radius, exp):
    _, (x, dy), (w, mu1, mu2) = _mixed_batch(61 + radius, shape, radius, "f32", exp)
    got = {k: _f32(v) for k, v in _gather(_plan(shape), x, dy, w, mu1, mu2).items()}
    want = dict(y=orc.forward(x, w, mu1, mu2, 0.5), dx=orc.backward(x, dy, w, mu1, mu2, 0.5, need=("dx",))["dx"])
    name = "per-image/r%d/%dx%dx%d/2^%d" % (radius, shape["N"], shape["H"], shape["W"], exp)
    small = record_margins(name + "/image0", {k: got[k][0] for k in want}, {k: want[k][0] for k in want}, BAR)
    big = record_margins(name + "/others", {k: got[k][1:] for k in want}, {k: want[k][1:] for k in want}, BAR)
    print(name, "margins image 0", small, "others", big)
    for key in ("y", "dx"):
        for n in range(shape["N"]):
            assert_parity(got[key][n], want[key][n], "%s/%s[%d]" % (name, key, n))


# ---------------------------------------------------------------------------------------------- 3. non-finite isolation
NONFINITE_SHAPES = [dict(N=2, S=16, F=32, G=4, H=24, W=24), dict(N=2, S=7, F=5, G=2, H=9, W=6)]


def _outside_box(H, W, py, px, half):
    yy, xx = np.mgrid[0:H, 0:W]
    return (np.abs(yy - py) > half) | (np.abs(xx - px) > half)


def _check_isolation(shape, radius, bad, scale, ring=False):
    N, S, F, G, H, W = _dims(shape)
    x, dy, w, mu1, mu2 = _inputs(71 + radius, shape, radius, ring)
    x[0] *= np.float32(scale)
    dy[0] *= np.float32(scale)
    py, px = 3, min(5, W - 1)
    x[1, S // 2, py, px] = bad
    dy[1, F // 2, py, px] = bad
    got = {k: _f32(v) for k, v in _gather(_plan(shape, ring=ring), x, dy, w, mu1, mu2, ring=ring).items()}
    # image 0: finite and at the bar against the oracle run on image 0 ALONE
    want = dict(y=orc.forward(x[:1], w, mu1, mu2, 0.5), dx=orc.backward(x[:1], dy[:1], w, mu1, mu2, 0.5, need=("dx",))["dx"])
    for key in ("y", "dx"):
        assert_parity(got[key][0], want[key][0], "nonfinite/%s[0]" % key)
    # image 1: the element reaches the outputs within (prefilter radius + the member's tap radius) of it, and no other
    outside = _outside_box(H, W, py, px, KR + (4 if ring else radius))
    for key in ("y", "dx"):
        assert not np.isfinite(got[key][1][:, py, px]).all(), "%s[1]: the element did not propagate" % key
        assert np.isfinite(got[key][1][:, outside]).all(), "%s[1] is non-finite outside the element's footprint" % key


@pytest.mark.parametrize("scale", [1e6, 1e-9])
@pytest.mark.parametrize("bad", [np.inf, np.nan, -np.inf], ids=["inf", "nan", "-inf"])
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", NONFINITE_SHAPES, **_ids)
def test_a_non_finite_element_stays_in_its_image(shape, radius, bad, scale):
    _check_isolation(shape, radius, np.float32(bad), scale)


@pytest.mark.parametrize("radius", RADII)
def test_a_nan_weight_stays_in_its_channel(radius):
    """One NaN weight (s0, g0, f0): y keeps every output channel but f0, dx every input channel but s0, finite and at the bar (the
    weight bound G * max|w| of the dense taps' scale is taken over the finite units)."""
    shape = NONFINITE_SHAPES[0]
    N, S, F, G, H, W = _dims(shape)
    x, dy, w, mu1, mu2 = _inputs(81 + radius, shape, radius)
    s0, g0, f0 = 5, 1, 9
    wn = w.copy()
    wn[0, s0, g0, f0] = np.nan
    got = {k: _f32(v) for k, v in _gather(_plan(shape), x, dy, wn, mu1, mu2).items()}
    want = dict(y=orc.forward(x, w, mu1, mu2, 0.5), dx=orc.backward(x, dy, w, mu1, mu2, 0.5, need=("dx",))["dx"])
    keep_f, keep_s = np.arange(F) != f0, np.arange(S) != s0
    assert np.isnan(got["y"][:, f0]).any() and np.isnan(got["dx"][:, s0]).any()
    assert_parity(got["y"][:, keep_f], want["y"][:, keep_f], "nan-weight/y")
    assert_parity(got["dx"][:, keep_s], want["dx"][:, keep_s], "nan-weight/dx")


# ---------------------------------------------------------------------------------------------- 4. slab invariance
@pytest.mark.parametrize("radius", RADII)
def test_a_slabbed_pass_gives_the_bits_of_the_whole_batch(radius, monkeypatch):
    shape = SHAPES[0]
    monkeypatch.setenv("DAU_WORKSPACE_BUDGET_GB", "0.0005")
    slabbed = _plan(shape)
    monkeypatch.delenv("DAU_WORKSPACE_BUDGET_GB")
    whole = _plan(shape)
    assert slabbed.info["batch_slab_gather"] < shape["N"] and whole.info["batch_slab_gather"] == shape["N"], (slabbed.info, whole.info)
    x, dy, w, mu1, mu2 = _inputs(91 + radius, shape, radius)
    first = slabbed.info["batch_slab_gather"]                  # the images of the first slab are 2^20 below the others
    x[:first] *= np.float32(2.0 ** -20)
    dy[:first] *= np.float32(2.0 ** -20)
    a, b = _gather(slabbed, x, dy, w, mu1, mu2), _gather(whole, x, dy, w, mu1, mu2)
    for key in ("y", "dx"):
        assert _same_bits(a[key], b[key]), key


# ---------------------------------------------------------------------------------------------- 5. the radius-3 + ring member
RING_SHAPES = [SHAPES[0], SHAPES[2]]                           # (the ragged shape's 70 units leave the member no outlier unit: 1 %)


@pytest.mark.parametrize("io", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", RING_SHAPES, **_ids)
def test_ring_member_bits_do_not_depend_on_batch_mates(shape, io):
    a, b, par = _mixed_batch(101, shape, 3, io, ring=True)
    plan = _plan(shape, io, ring=True)
    ga, gb = _gather(plan, *a, *par, io=io, ring=True), _gather(plan, *b, *par, io=io, ring=True)
    for key in ("y", "dx"):
        assert torch.isfinite(ga[key][0]).all() and ga[key][0].abs().max() > 0, key
        assert _same_bits(ga[key][0], gb[key][0]), "%s[0] changes with the other images of the batch" % key


@pytest.mark.parametrize("scale", [1e6, 1e-9])
@pytest.mark.parametrize("bad", [np.inf, np.nan, -np.inf], ids=["inf", "nan", "-inf"])
def test_ring_member_keeps_a_non_finite_element_in_its_image(bad, scale):
    _check_isolation(NONFINITE_SHAPES[0], 3, np.float32(bad), scale, ring=True)


# ---------------------------------------------------------------------------------------------- 6. degenerate images
@pytest.mark.parametrize("radius", RADII)
def test_zero_and_all_inf_images_leave_the_others_alone(radius):
    shape = SHAPES[0]
    x, dy, w, mu1, mu2 = _inputs(111 + radius, shape, radius)
    plan = _plan(shape)
    base = _gather(plan, x, dy, w, mu1, mu2)
    xd, dyd = x.copy(), dy.copy()
    xd[1] = 0.0; dyd[1] = 0.0
    xd[2] = np.inf; dyd[2] = np.inf
    got = _gather(plan, xd, dyd, w, mu1, mu2)
    for key in ("y", "dx"):
        for n in (0, 3):
            assert _same_bits(got[key][n], base[key][n]), (key, n)
        assert not got[key][1].any(), key                      # the zero image: scale 1, zeros
        assert not torch.isfinite(got[key][2]).any(), key      # every output of the all-Inf image has the image's taps in reach


# ---------------------------------------------------------------------------------------------- the maxima's load paths
@pytest.mark.parametrize("io", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]], **_ids)
def test_results_do_not_depend_on_the_base_alignment(shape, io):
    """The same batch at bases 0 .. 7 elements past an aligned address: the maxima run through other head / vector / tail splits
    (and the staging kernel through its scalar loads); every image's y and dx keep their bits."""
    from dau_conv import _capi
    N, S, F, G, H, W = _dims(shape)
    (_, _), (x, dy), (w, mu1, mu2) = _mixed_batch(121, shape, 3, io)
    plan = _plan(shape, io)
    dev = lambda a: torch.from_numpy(a).cuda()
    sg = torch.full((1, S, G, F), 0.5, device="cuda")
    wd, m1, m2 = dev(w), dev(mu1), dev(mu2)
    first = None
    for shift in (0, 1, 2, 3, 5):
        def place(a):
            buf = torch.zeros(a.size + 8, dtype=DTYPES[io], device="cuda")
            view = buf[shift:shift + a.size].view(a.shape)
            view.copy_(dev(a))
            return view
        xd, dyd = place(x), place(dy)
        assert xd.data_ptr() % 16 == (shift * xd.element_size()) % 16 or shift == 0
        y = plan.forward(xd, wd, m1, m2, sg)
        dx = plan.backward(xd, dyd, wd, m1, m2, sg, need_mask=_capi.NEED_DX)[0]
        plan.check_status()
        out = dict(y=y.cpu(), dx=dx.cpu())
        if first is None:
            first = out
        for key in ("y", "dx"):
            assert torch.isfinite(out[key]).all(), (key, shift)
            assert _same_bits(out[key], first[key]), (key, shift)
