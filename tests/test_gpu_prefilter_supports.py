"""GPU: every prefilter support through every member, layout and storage format.  sigma reaches the kernels only through the
support k = 2*ceil(5*sigma)+1 of the prefilter (3 .. 17 taps), and nearly every staging kernel is specialised on it at compile time
(blur_pack_kernel<K>, blur4_pack_kernel<K>, split_stage_kernel<K, act>, sd_xk_walk_kernel<K>, dense_stage_rows_kernel<K>,
wg_filter_kernel<K>), with a generic form or no member at all behind the widest ones.  The rest of the suite is deep at sigma 0.5
(7 taps) and thin elsewhere; this module runs one sigma per support

  1. through every member pinned by flags, fp32 NCHW, against the oracle at the project's bar (util.assert_parity at its defaults:
     1e-4 relative + 1e-6 of the max-norm; bf16-dense plans at the bars of test_gpu_dense_bf16.py / the dense sweep of test_gpu_fuzz.py),
  2. through the identities of include/dau_conv.h: NHWC plan = NCHW plan bit for bit, f16 plan = the fp32 plan on the widened input,
     bf16 I/O against the oracle at the storage bar of test_gpu_bf16.py,
  3. with a sigma tensor that differs from the plan's hint (same support), and one whose elements beyond the first are NaN,
  4. through a DAUConv2d layer whose trainable sigma crosses supports under channels_last float32 / float16 activations.

Coverage, support x member x layout x storage format -> test (7 taps is also what the rest of the suite runs):

  member                          supports          layout, format                  test
  exact gather-sum / gather-dot   3 .. 17           NCHW f32                        test_exact_kernels (A, C, D, E)
    blur_pack in row bands        13, 15, 17        NCHW f32                        test_exact_kernels_blur_pack_in_row_bands
                                  3, 5, 9, 11, 17   NCHW = NHWC x f32, f16, bf16    test_nhwc_plan_...[exact_A, exact_C]
                                  3,5,9,11,13,17    NCHW f16 = f32                 test_f16_plan_...[exact]            (7: test_gpu_f16.py)
                                  3, 9, 11, 17      NCHW bf16                       test_bf16_io_against_the_oracle[exact]
  split radii 2 / 3 / 4 and the   3 .. 11           NCHW f32                        test_split_members (A, B, D x 2.0, 3.0, 3.99)
  split gather-dot                3, 5, 9, 11       NCHW = NHWC x f32, f16, bf16    test_nhwc_plan_...[split_A_m3, split_B_m4, default_P]
                                  3, 5, 9, 11       NCHW f16 = f32                  test_f16_plan_...[split]
                                  3, 9, 11          NCHW bf16                       test_bf16_io_against_the_oracle[split]
    no split stage                13, 15, 17        gather_dense_split == 0         test_split_members, test_f16_plan_...[split], test_bf16_io_...[split-17]:
                                                                                    y, dx are the exact plan's bits; the split gather-dot still runs
  radius 3 + ring                 3, 5, 9, 11       NCHW f32                        test_ring_member
                                  3, 5, 9, 11       NCHW = NHWC x f32, f16, bf16    test_nhwc_plan_...[outliers_B]      (13 ..: no radius-3 member, as above)
  bf16 dense gather and wgrad     3, 5, 9, 11, 17   NCHW bf16                       test_bf16_dense_gather_and_wgrad    (plan creation refuses NHWC and
                                                                                    other formats with DAU_FLAG_DENSE_BF16; 13, 15: the generic path of 11, 17)
  direct kernels                  3 .. 17           NCHW f32                        test_direct_kernels                 (plan creation refuses 16-bit / NHWC I/O)
  sigma tensor != hint            7                 NCHW f32, NHWC f16              test_sigma_tensor_differs_from_the_hint (exact, split, direct)
  element 0 of sigma              7, 9              NCHW f32, bf16                  test_only_element_zero_of_sigma_is_read (exact, split, bf16 dense)
  layer, trainable sigma          7, 9, 11          NHWC f32, f16                   test_layer_with_a_trainable_sigma_crossing_supports

Every test asserts plan.info["blur_support"] (and the info fields that tell which member a call takes) before it runs anything.
tests/conftest.py forces DAU_FLAG_NO_DENSE_SPLIT only for the modules it lists; this one is not among them: every plan states its flags.
The oracle itself is pinned at these supports by tests/test_oracle_supports.py."""
import functools
import importlib

import numpy as np
import pytest
import torch

from oracle import dau_oracle as orc
from util import assert_parity, bits as _bits, make_inputs, record_margins

pytestmark = pytest.mark.gpu

# one sigma per support, away from the float32 rounding boundaries of 5*sigma (tests/test_oracle_supports.py checks the map on the CPU)
SIGMA = {3: 0.19, 5: 0.35, 7: 0.5, 9: 0.75, 11: 0.95, 13: 1.15, 15: 1.35, 17: 1.55}
SUPPORTS = sorted(SIGMA)
NAMES = ("y", "dx", "dw", "dmu1", "dmu2", "dsigma")
I, BF16, DENSE_BF16, WGRAD_ALWAYS, SPLIT, NO_SPLIT, F16, OUTLIERS, NHWC = 1 << 0, 1 << 4, 1 << 6, 1 << 8, 1 << 9, 1 << 10, 1 << 11, 1 << 12, 1 << 13
IO = {"f32": (0, torch.float32), "f16": (F16, torch.float16), "bf16": (BF16, torch.bfloat16)}
ALGO_DIRECT, ALGO_TILED = 1, 2
FP32_BAR = "1e-4 rel + 1e-6 max-norm (fp32 bar)"

# name -> ((N, S, F, G, H, W), max_kernel_size): the smallest shapes that still contain the seams
SHAPES = {
    # H = 21: at least two stage bands of the split members at every support (stage_plan: 18 / 16 / 14 / 12 / 10 rows per band for
    # 3 / 5 / 7 / 9 / 11 taps); W = 70: two 64-column segments, the halo across the seam; S = 7: element loads
    "A": ((2, 7, 5, 2, 21, 70), 9),
    "B": ((2, 16, 40, 4, 28, 28), 9),         # 16-byte paths, tall tiles, G = 4 for the split gather-dot
    "C": ((2, 5, 8, 2, 40, 72), 17),          # offsets up to 7: bucket 8
    "D": ((2, 4, 8, 2, 5, 4), 9),             # the image smaller than the support in both directions
    "E": ((2, 3, 4, 2, 1, 9), 9),             # one row
    "P": ((2, 128, 128, 4, 16, 16), 9),       # the shape whose DEFAULT plan holds the split members and the split gather-dot
    # exact kernels, 13 / 15 / 17 taps: blur_pack in row bands.  Derived from blur_pack_lds_bytes (k_gather_mfma.hip): only the
    # 56 x 56 patches (kVariants row 0 under kernel 9: 65 staged rows and columns, a 9-column strip) have a window that passes the
    # 80 KiB at which blur_pack_bands starts cutting: ((wh+k-1)(ww+k-1) + (wh+k-1) ww + 9 * 65) * 8 bytes with wh = min(65, H),
    # ww = min(65, W).  A 56 x 112 map (two such patches; wh = 56, ww = 65) gives 78600 bytes at 11 taps (one band) and
    # 81928 / 85320 / 88776 at 13 / 15 / 17 (two).  make_geometry prices the rounds of workgroups, so the forward pass takes those
    # patches only from N/2 * F = 512 workgroups on: 4 images, 256 output channels; the two input channels keep the oracle at 0.4 s.
    # (The input-gradient pass of this shape, 2 output channels, takes small patches.)  _blur_pack_bands below redoes the sum.
    "T": ((4, 2, 256, 1, 56, 112), 9),
}


@functools.lru_cache(maxsize=None)
def _inputs(shape, m, rounding="f32", outlier=False):
    """(x, dy, w, mu1, mu2), read-only, shared by every test of that (shape, offset range, storage format).  The corner units are
    pinned as test_split_gather_against_oracle does: the corners of the (2r+1)^2 kernel, 3.99 being the layer's clip of radius 4."""
    (N, S, F, G, H, W), ks = SHAPES[shape]
    x, dy, w, mu1, mu2 = make_inputs(500 + sum(ord(c) for c in shape) + int(10 * m), N, S, F, G, H, W, ks, m)
    c = min(m, ks // 2 - 0.01)
    mu1.flat[0] = c; mu2.flat[0] = -c; mu1.flat[1] = -c; mu2.flat[1] = c
    if outlier:
        mu1.flat[5] = 3.5                     # one unit beyond +-3: the radius-3 + ring member's call
    if rounding != "f32":                     # what a 16-bit plan reads: the oracle gets these values, widened
        dt = {"f16": torch.float16, "bf16": torch.bfloat16}[rounding]
        x, dy = (torch.from_numpy(a).to(dt).float().numpy() for a in (x, dy))
    for a in (x, dy, w, mu1, mu2):
        a.setflags(write=False)
    return x, dy, w, mu1, mu2


@functools.lru_cache(maxsize=None)
def _oracle(shape, m, sigma, rounding="f32", outlier=False, k=0):
    """the six tensors of the oracle, computed once per case and left unchanged"""
    x, dy, w, mu1, mu2 = _inputs(shape, m, rounding, outlier)
    want = orc.backward(x, dy, w, mu1, mu2, sigma, k=k)
    want["y"] = orc.forward(x, w, mu1, mu2, sigma, k=k)
    for a in want.values():
        a.setflags(write=False)
    return want


def _plan(shape, k, flags, sigma_hint=None, **kw):
    from dau_conv import _capi
    dims, ks = SHAPES[shape]
    plan = _capi.Plan(*dims, max_kernel_size=ks, sigma_hint=SIGMA[k] if sigma_hint is None else sigma_hint, flags=flags, **kw)
    assert plan.info["blur_support"] == k, plan.info
    return plan


def _sigma_tensor(data, sigma):
    S, G, F = data[2].shape[1:]
    return torch.full((1, S, G, F), float(sigma), device="cuda")


def _run(plan, data, sigma, outliers=False):
    """forward + backward, status checked after each; x, dy in the plan's storage format and layout -> (y, dx, dw, dmu1, dmu2, dsigma)"""
    x, dy, w, mu1, mu2 = data
    fmt = torch.channels_last if plan.io_layout == "NHWC" else torch.contiguous_format
    xd, dyd = (torch.tensor(a, device="cuda").to(plan.io_dtype).contiguous(memory_format=fmt) for a in (x, dy))
    wd, m1, m2 = (torch.tensor(a, device="cuda") for a in (w, mu1, mu2))
    sg = sigma if torch.is_tensor(sigma) else _sigma_tensor(data, sigma)
    y = plan.forward(xd, wd, m1, m2, sg)
    plan.check_status()
    if outliers:
        assert plan.outlier_status() == (1, True), "the radius-3 + ring member did not run the forward pass"
    grads = plan.backward(xd, dyd, wd, m1, m2, sg)
    plan.check_status()
    if outliers:
        assert plan.outlier_status() == (1, True), "the radius-3 + ring member did not run the input-gradient pass"
    assert y.dtype == plan.io_dtype and grads[0].dtype == plan.io_dtype and grads[1].dtype == torch.float32
    return (y,) + tuple(grads)


def _np(out):
    """-> {name: float32 numpy array in logical [N, C, H, W] order}"""
    return {n: t.float().contiguous().cpu().numpy() for n, t in zip(NAMES, out)}


def _same_bits(got, ref, what):
    for g, r, n in zip(got, ref, NAMES):
        assert g.shape == r.shape and g.dtype == r.dtype, n
        differ = int((_bits(g) != _bits(r)).sum())
        assert differ == 0, "%s: %s: %d of %d values differ" % (what, n, differ, r.numel())
        assert torch.isfinite(g.float()).all(), n


def _check_fp32(got, want, name, bar=FP32_BAR):
    m = record_margins(name, got, {n: want[n] for n in NAMES}, bar)
    print(name, {n: "%.2e" % v for n, v in m.items()})
    for n in NAMES:
        assert_parity(got[n], want[n], name + "/" + n)


def _check_storage(got, want, name, rel, floor):
    """y and dx stored in 16 bits: the storage bar; the parameter gradients are fp32 arithmetic on the same inputs: the fp32 bar"""
    m = record_margins(name, got, {n: want[n] for n in NAMES}, "y, dx: %g rel + %g max-norm (16-bit storage); parameter gradients: %s" % (rel, floor, FP32_BAR))
    print(name, {n: "%.2e" % v for n, v in m.items()})
    for n in ("y", "dx"):
        assert_parity(got[n], want[n], name + "/" + n, rel=rel, floor=floor)
    for n in NAMES[2:]:
        assert_parity(got[n], want[n], name + "/" + n)


def _assert_exact_tiled(info):
    """the plan holds the exact tiled kernels and no dense member: what runs is what the test names"""
    assert info["gather_dense_split"] == 0 and info["gather_dense_bf16"] == 0, info
    assert info["algo_forward"] == ALGO_TILED and info["algo_backward"] == ALGO_TILED, info


def _offsets_of(shape):
    return 7.0 if shape == "C" else 3.99


# ---- 1. every support, every member, fp32 NCHW, against the oracle ---------------------------------------------------------------
@pytest.mark.parametrize("shape", ["A", "C", "D", "E"])
@pytest.mark.parametrize("k", SUPPORTS)
def test_exact_kernels(k, shape):
    """blur_pack_kernel<5 / 7 / 9 / 0> and blur4_pack_kernel<5 / 7 / 9 / 0> in front of the exact gather-sum and gather-dot"""
    plan = _plan(shape, k, I | NO_SPLIT)
    _assert_exact_tiled(plan.info)
    if shape == "C":
        assert plan.info["offset_bucket"] == 8
    m = _offsets_of(shape)
    got = _np(_run(plan, _inputs(shape, m), SIGMA[k]))
    _check_fp32(got, _oracle(shape, m, SIGMA[k]), "supports/exact/k%d/%s" % (k, shape))


def _blur_pack_bands(H, W, k, rows=65, cols=65, strip_cols=9):
    """blur_pack_bands of k_gather_mfma.hip for the 56 x 56 patches of kernel 9 (kVariants row 0)"""
    def lds_bytes(band_rows):
        r = band_rows if 0 < band_rows < rows else rows
        wh, ww = min(r, H), min(cols, W)
        return ((wh + k - 1) * (ww + k - 1) + (wh + k - 1) * ww + strip_cols * (r | 1)) * 8
    bands = 1
    while bands < 8 and lds_bytes(-(-rows // bands)) > 80 * 1024:
        bands += 1
    return bands


@pytest.mark.parametrize("k", [13, 15, 17])
def test_exact_kernels_blur_pack_in_row_bands(k):
    """the generic blur_pack_kernel<0> with its window cut into row bands: every band re-reads its halo of k - 1 rows"""
    plan = _plan("T", k, I | NO_SPLIT)
    _assert_exact_tiled(plan.info)
    assert plan.info["gather_variant"] == 0 and plan.info["gather_patch"] == 56, plan.info       # what _blur_pack_bands assumes
    H, W = SHAPES["T"][0][4:]
    assert _blur_pack_bands(H, W, k) == 2 and _blur_pack_bands(H, W, 11) == 1
    got = _np(_run(plan, _inputs("T", 3.99), SIGMA[k]))
    _check_fp32(got, _oracle("T", 3.99, SIGMA[k]), "supports/exact-bands/k%d/T" % k)


@pytest.mark.parametrize("m", [2.0, 3.0, 3.99])
@pytest.mark.parametrize("shape", ["A", "B", "D"])
@pytest.mark.parametrize("k", SUPPORTS)
def test_split_members(k, shape, m):
    """split_stage_kernel<3 / 5 / 7 / 9 / 11> in front of the two-limb f16 GEMM of each radius; the parameter gradients through the
    split gather-dot (sd_xk_walk_kernel<5 / 7 / 9>, or the blur4_pack + sd_stage_x chain).  13 taps and more have no split stage:
    the plan must then LACK the split gather-sum members (not hold wrong ones), and its gather-sum passes are the exact kernels'."""
    plan = _plan(shape, k, I | SPLIT)
    assert plan.info["gather_dense_split"] == (0b11100 if k <= 11 else 0), plan.info
    assert plan.info["algo_forward"] == ALGO_TILED and plan.info["algo_backward"] == ALGO_TILED
    data = _inputs(shape, m)
    assert max(np.abs(data[3]).max(), np.abs(data[4]).max()) > m - 1           # this call belongs to the member of THIS radius
    out = _run(plan, data, SIGMA[k])
    _check_fp32(_np(out), _oracle(shape, m, SIGMA[k]), "supports/split/k%d/%s/m%g" % (k, shape, m))
    if k >= 13:
        # no split stage for this support (stage_for): y and dx are the bits of the plan that never had the members ...
        exact = _run(_plan(shape, k, I | NO_SPLIT), data, SIGMA[k])
        _same_bits(out[:2], exact[:2], "gather-sum passes without a split stage")
        # ... while split_dot_configure still takes the plan (blur4_pack_fits holds for these maps; every support other than 5 / 7 / 9
        # stages through blur4_pack + sd_stage_x): the parameter gradients come from the two-limb gather-dot, another arithmetic
        # inside the same bar
        assert any(not torch.equal(_bits(a), _bits(b)) for a, b in zip(out[2:], exact[2:])), "the split gather-dot did not run"


@pytest.mark.parametrize("k", [3, 5, 9, 11])
def test_ring_member(k):
    """k_dense_ring.hip reads what the radius-3 split stage wrote: one unit at 3.5 among offsets within +-3"""
    plan = _plan("B", k, I | SPLIT | OUTLIERS)
    assert plan.info["gather_dense_split"] == 0b111100, plan.info
    got = _np(_run(plan, _inputs("B", 3.0, outlier=True), SIGMA[k], outliers=True))
    _check_fp32(got, _oracle("B", 3.0, SIGMA[k], outlier=True), "supports/ring/k%d/B" % k)


@pytest.mark.parametrize("shape", ["A", "B"])
@pytest.mark.parametrize("k", [3, 5, 9, 11, 17])
def test_bf16_dense_gather_and_wgrad(k, shape):
    """dense_stage_rows_kernel<3 / 5 / 9> and the fused wg_filter_kernel<3 / 5 / 9>; 11 and 17 taps take the generic staging path and
    blur4_pack.  Offsets within +-4, the oracle on the bf16-rounded inputs.  Bars: B at test_gpu_dense_bf16.py's (2e-2 relative +
    4e-3 of the max-norm for y and dx, 1e-2 for the dense parameter gradients: test_dense_forms_under_other_prefilter_supports); A
    has few channels (S = 7, F = 5: an output is a small sum of comparatively large terms), the case for which the dense sweep of
    test_gpu_fuzz.py sets the floor to 1e-2 of the max-norm for every tensor."""
    plan = _plan(shape, k, I | BF16 | DENSE_BF16 | WGRAD_ALWAYS)
    assert plan.info["gather_dense_bf16"] == 2 and plan.info["gather_dense_split"] == 0, plan.info
    got = _np(_run(plan, _inputs(shape, 3.99, "bf16"), SIGMA[k]))
    want = _oracle(shape, 3.99, SIGMA[k], "bf16")
    floor_act = 1e-2 if shape == "A" else 4e-3
    name = "supports/dense-bf16/k%d/%s" % (k, shape)
    m = record_margins(name, got, {n: want[n] for n in NAMES}, "2e-2 rel + %g max-norm (y, dx), + 1e-2 (dense parameter gradients)" % floor_act)
    print(name, {n: "%.2e" % v for n, v in m.items()})
    for n in ("y", "dx"):
        assert_parity(got[n], want[n], name + "/" + n, rel=2e-2, floor=floor_act)
    for n in NAMES[2:]:
        assert_parity(got[n], want[n], name + "/" + n, rel=2e-2, floor=1e-2)


@pytest.mark.parametrize("shape", ["D", "E"])
@pytest.mark.parametrize("k", SUPPORTS)
def test_direct_kernels(k, shape):
    from dau_conv import _capi
    plan = _plan(shape, k, I, algo=_capi.ALGO_DIRECT)
    assert plan.info["algo_forward"] == ALGO_DIRECT and plan.info["algo_backward"] == ALGO_DIRECT, plan.info
    assert plan.info["gather_dense_split"] == 0 and plan.info["gather_dense_bf16"] == 0
    got = _np(_run(plan, _inputs(shape, 3.99), SIGMA[k]))
    _check_fp32(got, _oracle(shape, 3.99, SIGMA[k]), "supports/direct/k%d/%s" % (k, shape))


# ---- 2. identities across layout and storage -------------------------------------------------------------------------------------
# name -> (flags, shape, offsets within, one unit at 3.5); test_nhwc_call_returns_the_bits_of_the_nchw_call's rows, with a sigma
LAYOUT_ROWS = {
    "exact_A": (NO_SPLIT, "A", 3.99, False),
    "exact_C": (NO_SPLIT, "C", 7.0, False),
    "split_A_m3": (SPLIT, "A", 3.0, False),
    "split_B_m4": (SPLIT, "B", 3.99, False),
    "outliers_B": (SPLIT | OUTLIERS, "B", 3.0, True),
    "default_P": (0, "P", 3.0, False),
}
# 17 taps: the exact rows only (no split member to compare)
LAYOUT_CASES = [(k, row) for k in (3, 5, 9, 11, 17) for row in LAYOUT_ROWS if k != 17 or row.startswith("exact")]


@pytest.mark.parametrize("io", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("k, row", LAYOUT_CASES, ids=["k%d-%s" % c for c in LAYOUT_CASES])
def test_nhwc_plan_returns_the_bits_of_the_nchw_plan(k, row, io):
    """blur_pack_kernel<K | NHWC>, blur4_pack_nhwc_kernel<K>, split_stage_kernel<K | NHWC, act>: other addresses, the same sums"""
    flags, shape, m, outlier = LAYOUT_ROWS[row]
    nchw = _plan(shape, k, I | flags | IO[io][0])
    nhwc = _plan(shape, k, I | flags | IO[io][0] | NHWC)
    assert nhwc.info == nchw.info and nhwc.io_layout == "NHWC" and nchw.io_layout == "NCHW"
    if flags & NO_SPLIT:
        _assert_exact_tiled(nhwc.info)
    elif flags & OUTLIERS:
        assert nhwc.info["gather_dense_split"] == 0b111100
    else:
        assert nhwc.info["gather_dense_split"] == 0b11100           # forced, or the default plan of shape P
    data = _inputs(shape, m, io, outlier)
    want = _run(nchw, data, SIGMA[k], outliers=outlier)
    got = _run(nhwc, data, SIGMA[k], outliers=outlier)
    for t in got[:2]:
        assert t.is_contiguous(memory_format=torch.channels_last) and t.dtype == IO[io][1]
    _same_bits(got, want, "NHWC plan against the NCHW plan")


@pytest.mark.parametrize("shape, m", [("A", 3.0), ("B", 3.99)], ids=["A", "B"])
@pytest.mark.parametrize("members", [SPLIT, NO_SPLIT], ids=["split", "exact"])
@pytest.mark.parametrize("k", [3, 5, 9, 11, 13, 17])
def test_f16_plan_is_the_fp32_plan_on_the_widened_input(k, members, shape, m):
    """single-pass plans: y and dx are torch.half() of the fp32 plan's, the parameter gradients its bits"""
    p16 = _plan(shape, k, I | members | F16)
    p32 = _plan(shape, k, I | members)
    assert p16.info == p32.info and p16.info["gather_windows"] == 1
    assert p16.info["gather_dense_split"] == (0b11100 if members == SPLIT and k <= 11 else 0), p16.info
    data = _inputs(shape, m, "f16")
    got = _run(p16, data, SIGMA[k])
    ref = _run(p32, data, SIGMA[k])
    _same_bits(got, (ref[0].half(), ref[1].half()) + ref[2:], "f16 plan against the fp32 plan on the widened input")


@pytest.mark.parametrize("members", [SPLIT, NO_SPLIT], ids=["split", "exact"])
@pytest.mark.parametrize("k", [3, 9, 11, 17])
def test_bf16_io_against_the_oracle(k, members):
    """bf16 activations through the exact and the split members (fp32 arithmetic on the widened input): y and dx at the storage bar
    of test_gpu_bf16.py, the parameter gradients at the fp32 bar"""
    plan = _plan("A", k, I | members | BF16)
    assert plan.info["gather_dense_split"] == (0b11100 if members == SPLIT and k <= 11 else 0) and plan.info["gather_dense_bf16"] == 0
    assert plan.info["algo_forward"] == ALGO_TILED and plan.info["algo_backward"] == ALGO_TILED
    got = _np(_run(plan, _inputs("A", 3.99, "bf16"), SIGMA[k]))
    _check_storage(got, _oracle("A", 3.99, SIGMA[k], "bf16"), "supports/bf16-io/%s/k%d/A" % ("split" if members == SPLIT else "exact", k),
                   rel=2e-2, floor=4e-3)


# ---- 3. sigma semantics at the plan level ------------------------------------------------------------------------------------------
def _semantics_plan(kind, k, hint):
    """-> (plan, offsets within, storage format of the inputs)"""
    from dau_conv import _capi
    if kind == "exact":
        plan = _plan("A", k, I | NO_SPLIT, sigma_hint=hint)
        _assert_exact_tiled(plan.info)
        return plan, 3.99, "f32"
    if kind == "split":
        plan = _plan("A", k, I | SPLIT, sigma_hint=hint)
        assert plan.info["gather_dense_split"] == 0b11100
        return plan, 3.0, "f32"
    if kind == "nhwc_f16":
        plan = _plan("A", k, I | SPLIT | F16 | NHWC, sigma_hint=hint)
        assert plan.info["gather_dense_split"] == 0b11100 and plan.io_layout == "NHWC"
        return plan, 3.0, "f16"
    if kind == "dense_bf16":
        plan = _plan("A", k, I | BF16 | DENSE_BF16 | WGRAD_ALWAYS, sigma_hint=hint)
        assert plan.info["gather_dense_bf16"] == 2
        return plan, 3.99, "bf16"
    assert kind == "direct"
    plan = _plan("A", k, I, sigma_hint=hint, algo=_capi.ALGO_DIRECT)
    assert plan.info["algo_forward"] == ALGO_DIRECT and plan.info["algo_backward"] == ALGO_DIRECT
    return plan, 3.99, "f32"


@pytest.mark.parametrize("kind", ["exact", "split", "nhwc_f16", "direct"])
def test_sigma_tensor_differs_from_the_hint(kind):
    """include/dau_conv.h: all a plan keeps of sigma_hint is the support; "the taps themselves are computed from the device tensor each
    call".  A plan made for 0.5 called with 0.42, then 0.58 (both 7 taps; 0.6f * 5 is avoided on purpose), then 0.42 again: each call
    matches the oracle at ITS sigma on a 7 x 7 support, and the third returns the bits of the first -- nothing is kept of a call."""
    plan, m, rounding = _semantics_plan(kind, 7, 0.5)
    for s in (0.42, 0.58):
        assert orc.filter_support(s) == 7
    data = _inputs("A", m, rounding)
    first = None
    for step, s in enumerate((0.42, 0.58, 0.42)):
        out = _run(plan, data, s)
        if step == 2:
            _same_bits(out, first, "sigma 0.42 after a call with 0.58")
            break
        first = first or out
        want = _oracle("A", m, s, rounding, k=7)
        name = "supports/sigma-tensor/%s/sigma%g" % (kind, s)
        if rounding == "f16":
            _check_storage(_np(out), want, name, rel=2e-3, floor=1e-3)       # test_gpu_f16.py's storage bar
        else:
            _check_fp32(_np(out), want, name)
    # and the two sigmas are told apart by the bar: the call at 0.58 does not pass as one at 0.42
    y42, y58 = (_oracle("A", m, s, rounding, k=7)["y"] for s in (0.42, 0.58))
    assert np.abs(y58 - y42).max() > 1e-2 * np.abs(y42).max()


@pytest.mark.parametrize("kind", ["exact", "split", "dense_bf16"])
@pytest.mark.parametrize("k", [7, 9])
def test_only_element_zero_of_sigma_is_read(kind, k):
    """include/dau_conv.h: "element 0 is used".  NaN in every other element: the bits of the uniform tensor."""
    plan, m, rounding = _semantics_plan(kind, k, SIGMA[k])
    data = _inputs("A", m, rounding)
    uniform = _sigma_tensor(data, SIGMA[k])
    poisoned = torch.full_like(uniform, float("nan"))
    poisoned.view(-1)[0] = uniform.view(-1)[0]
    want = _run(plan, data, uniform)
    got = _run(plan, data, poisoned)
    _same_bits(got, want, "sigma with NaN beyond element 0")


# ---- 4. layer level: a trainable sigma crossing supports under channels_last and autocast dtypes -------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_layer_with_a_trainable_sigma_crossing_supports(dtype):
    """dau_sigma_trainable=True moves sigma across support boundaries during training, and a channels_last input runs the NHWC plan
    by default: 0.5 -> 0.75 -> 0.95 -> 0.5 (7, 9, 11, 7 taps).  After every step forward and backward against the oracle at that
    sigma, sigma.grad against the float64 sum of the oracle's dsigma, and the plan cache: one plan per support visited."""
    import dau_conv
    dc = importlib.import_module("dau_conv.dau_conv")
    dc._PLANS.clear()
    torch.manual_seed(7)
    N, S, F, H, W = 2, 8, 16, 21, 70
    lr = 10.0
    layer = dau_conv.DAUConv2d(dau_sigma_trainable=True, in_channels=S, filters=F, dau_units=(2, 2), max_kernel_size=9, use_bias=False,
                               mu1_initializer=dau_conv.random_uniform_initializer(-3, 3),
                               mu2_initializer=dau_conv.random_uniform_initializer(-3, 3), mu_learning_rate_factor=lr).cuda()
    assert layer.sigma.requires_grad and tuple(layer.sigma.shape) == (1,)
    x = torch.rand(N, S, H, W, device="cuda").to(dtype).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(N, F, H, W, device="cuda").to(dtype).contiguous(memory_format=torch.channels_last)
    xn, dyn = x.float().contiguous().cpu().numpy(), dy.float().contiguous().cpu().numpy()         # the widened inputs
    lim = layer._dau_convolution_op.mean_max_allowed_offset
    w, mu1, mu2 = (t.detach().cpu().numpy() for t in (layer.dau_weights, layer.dau_mu1, layer.dau_mu2))
    mu1c, mu2c = np.clip(mu1, -lim, lim), np.clip(mu2, -lim, lim)
    inside1, inside2 = (np.abs(mu1) <= lim).astype(np.float32), (np.abs(mu2) <= lim).astype(np.float32)
    plans_of, visited = {}, []
    for step, sigma in enumerate((0.5, 0.75, 0.95, 0.5)):
        k = orc.filter_support(sigma)
        with torch.no_grad():
            layer.sigma.fill_(sigma)
        layer.zero_grad()
        xi = x.detach().requires_grad_(True)
        y = layer(xi)
        y.backward(dy)
        dau_conv.check_pending_offsets()
        assert abs(layer._sigma_host - sigma) < 1e-6, (layer._sigma_host, sigma)
        assert y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last) and not y.is_contiguous()
        assert xi.grad.dtype == dtype
        # the plan cache: one plan per support visited, all of them NHWC plans; the way back to 0.5 takes the first plan again
        if k not in visited:
            visited.append(k)
        assert sorted(p.info["blur_support"] for p in dc._PLANS.values()) == sorted(visited), (step, list(dc._PLANS))
        assert all(p.io_layout == "NHWC" and p.io_dtype == dtype for p in dc._PLANS.values())
        used = list(dc._PLANS.values())[-1]                                # (the cache keeps the plan of the last call at its end)
        assert used.info["blur_support"] == k
        assert plans_of.setdefault(k, used) is used, "sigma %g did not hit the plan of its support again" % sigma
        want = orc.backward(xn, dyn, w, mu1c, mu2c, sigma, mu_learning_rate_factor=lr)
        want["y"] = orc.forward(xn, w, mu1c, mu2c, sigma)
        got = dict(y=y.detach().float().contiguous().cpu().numpy(), dx=xi.grad.float().contiguous().cpu().numpy(),
                   dw=layer.weights.grad.cpu().numpy(), dmu1=layer.mu1.grad.cpu().numpy(), dmu2=layer.mu2.grad.cpu().numpy())
        want_g = dict(y=want["y"], dx=want["dx"], dw=want["dw"], dmu1=want["dmu1"] * inside1, dmu2=want["dmu2"] * inside2)
        tag = "supports/layer/%s/step%d-sigma%g" % ("f16" if dtype == torch.float16 else "f32", step, sigma)
        m = record_margins(tag, got, want_g, FP32_BAR if dtype == torch.float32 else "y, dx: 2e-3 rel + 1e-3 max-norm (f16 storage); parameter gradients: " + FP32_BAR)
        print(tag, {n: "%.2e" % v for n, v in m.items()})
        act_bar = {} if dtype == torch.float32 else dict(rel=2e-3, floor=1e-3)        # test_gpu_f16.py's bars for f16 activations
        for n in ("y", "dx"):
            assert_parity(got[n], want_g[n], tag + "/" + n, **act_bar)
        for n in ("dw", "dmu1", "dmu2"):
            assert_parity(got[n], want_g[n], tag + "/" + n)
        # sigma is one scalar tiled to the parameter shape: its gradient is the sum of the per-unit gradients
        ds = want["dsigma"].astype(np.float64)
        got_ds, want_ds = float(layer.sigma.grad.item()), float(ds.sum())
        print(tag, "dsigma sum: got %.7g want %.7g sum|dsigma| %.4g" % (got_ds, want_ds, np.abs(ds).sum()))
        assert abs(got_ds - want_ds) <= 1e-4 * abs(want_ds) + 1e-6 * float(np.abs(ds).sum()), (got_ds, want_ds)
    assert len(dc._PLANS) == 3 and sorted(plans_of) == [7, 9, 11]
    dc._PLANS.clear()
