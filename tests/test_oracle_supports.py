"""CPU: the C oracle at every prefilter support.  The golden vectors pin its filters at sigma 0.5 and 0.8 on a 9 x 9 support only;
the GPU tests of tests/test_gpu_prefilter_supports.py lean on it from 3 to 17 taps.  So here the yardstick is pinned first: the six
filters against a float64 numpy closed form written from the formulas (unit_normalization = true: every filter is divided by the
sum Z of the masked Gaussian, and the derivative filters have their Z-weighted mean taken out), and the zero-padded correlation
against a direct float64 one, on images smaller than the support, of one row, and with more than one row band and column segment."""
import numpy as np
import pytest

from oracle import dau_oracle as orc
from util import assert_parity

# one sigma per support 2*ceil(5*sigma)+1, away from the float32 rounding boundaries of 5*sigma
SIGMA_OF_SUPPORT = {3: 0.19, 5: 0.35, 7: 0.5, 9: 0.75, 11: 0.95, 13: 1.15, 15: 1.35, 17: 1.55}
NAMES = ("Gn", "Dw", "Dmu1", "Dmu2", "Dsigma", "Gerr")


def closed_form_filters(sigma, k, single_dim_kernel=False, forbid_positive_dim1=False):
    """The six k x k filters in float64, [row = y][column = x]; sigma as the float32 the kernels and the oracle receive."""
    s = float(np.float32(sigma))
    c = (k - 1) // 2
    v, u = (a.astype(np.float64) for a in np.mgrid[-c:c + 1, -c:c + 1])          # u along x (mu1), v along y (mu2)
    g = np.exp(-(u * u + v * v) / (2.0 * s * s))
    if single_dim_kernel:
        g[v != 0] = 0.0
    if forbid_positive_dim1:
        g[u > 0] = 0.0
    gn = g / g.sum()
    d1, d2, ds = u / s ** 2 * gn, v / s ** 2 * gn, (u * u + v * v) / s ** 3 * gn
    return dict(Gn=gn, Dw=gn, Dmu1=d1 - gn * d1.sum(), Dmu2=d2 - gn * d2.sum(), Dsigma=ds - gn * ds.sum(), Gerr=gn[::-1, ::-1])


def direct_correlation(x, filt):
    """out[y, x] = sum_ji filt[j, i] * x[y + j - c, x + i - c], zero beyond the image, in float64"""
    k = filt.shape[0]
    c = (k - 1) // 2
    H, W = x.shape[-2:]
    xp = np.zeros(x.shape[:-2] + (H + 2 * c, W + 2 * c), np.float64)
    xp[..., c:c + H, c:c + W] = x
    out = np.zeros(x.shape, np.float64)
    for j in range(k):
        for i in range(k):
            out += float(filt[j, i]) * xp[..., j:j + H, i:i + W]
    return out


def test_one_sigma_per_support():
    for k, sigma in SIGMA_OF_SUPPORT.items():
        assert orc.filter_support(sigma) == k
        # away from the boundary: a few float32 ulps of sigma either way give the same support
        for s in (np.nextafter(np.float32(sigma), np.float32(0)), np.nextafter(np.float32(sigma), np.float32(2)), sigma * 0.99, sigma * 1.01):
            assert orc.filter_support(float(s)) == k, (k, s)


@pytest.mark.parametrize("fp", [False, True], ids=["fp0", "fp1"])
@pytest.mark.parametrize("sd", [False, True], ids=["sd0", "sd1"])
@pytest.mark.parametrize("k", sorted(SIGMA_OF_SUPPORT))
def test_filters_match_the_closed_form(k, sd, fp):
    sigma = SIGMA_OF_SUPPORT[k]
    got = orc.filters(sigma, single_dim_kernel=sd, forbid_positive_dim1=fp)
    want = closed_form_filters(sigma, k, sd, fp)
    for name in NAMES:
        assert got[name].shape == (k, k)
        # the bar of test_filters_match_reference_oracle (tests/test_oracle_golden.py)
        assert_parity(got[name], want[name], "k%d sd%d fp%d %s" % (k, sd, fp, name), rel=1e-6, floor=1e-7)
    # what the formulas imply, to rounding: unit mass, derivative filters of zero mass
    assert abs(float(got["Gn"].astype(np.float64).sum()) - 1.0) < 1e-6
    for name in ("Dmu1", "Dmu2", "Dsigma"):
        assert abs(float(got[name].astype(np.float64).sum())) < 1e-6 * max(1.0, float(np.abs(want[name]).sum())), name


@pytest.mark.parametrize("H, W", [(3, 2), (1, 9), (21, 70)], ids=["3x2", "1x9", "21x70"])
@pytest.mark.parametrize("k", sorted(SIGMA_OF_SUPPORT))
def test_blur_matches_a_direct_correlation(k, H, W):
    """3 x 2 is smaller than every support but 3 in both directions, 1 x 9 is one row, 21 x 70 the map of the GPU tests.  The
    filters: Dmu1 and Dmu2 (odd in x / in y, so a flipped axis shows), Gn, and taps without any symmetry."""
    rs = np.random.RandomState(100 * k + H)
    x = rs.rand(2, 3, H, W).astype(np.float32)
    f = orc.filters(SIGMA_OF_SUPPORT[k])
    for name, filt in (("Gn", f["Gn"]), ("Dmu1", f["Dmu1"]), ("Dmu2", f["Dmu2"]), ("random", rs.randn(k, k).astype(np.float32))):
        got = orc.blur(x, filt)
        assert got.shape == x.shape and got.dtype == np.float32
        # the oracle sums in double and rounds once: half an ulp of float32 (6e-8); the bar of the filter test
        assert_parity(got, direct_correlation(x, filt), "k%d %dx%d %s" % (k, H, W, name), rel=1e-6, floor=1e-7)


@pytest.mark.parametrize("k", [3, 13, 17])
def test_forward_is_blur_then_shift_at_other_supports(k):
    """orc.forward(..., k=0) takes the support from sigma: a single unit at an integer offset gives the shifted direct correlation"""
    sigma = SIGMA_OF_SUPPORT[k]
    rs = np.random.RandomState(k)
    x = rs.rand(1, 1, 3, 9).astype(np.float32)
    w = np.ones((1, 1, 1, 1), np.float32)
    mu1, mu2 = np.full((1, 1, 1, 1), 2.0, np.float32), np.zeros((1, 1, 1, 1), np.float32)
    xb = direct_correlation(x, closed_form_filters(sigma, k)["Gn"])
    want = np.zeros_like(xb)
    want[..., :, :7] = xb[..., :, 2:]
    assert_parity(orc.forward(x, w, mu1, mu2, sigma), want, "k%d" % k, rel=1e-6, floor=1e-7)
    assert_parity(orc.forward(x, w, mu1, mu2, sigma, k=k), want, "k%d explicit" % k, rel=1e-6, floor=1e-7)
