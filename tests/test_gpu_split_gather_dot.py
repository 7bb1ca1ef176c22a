"""GPU: the parameter gradients as a two-limb f16 GEMM with the bilinear corners as rows (k_split_dot.hip, split_gather_dot_kernel).
Calls whose offsets lie within +-4 take it (DAU_FLAG_DENSE_SPLIT_F16 whatever the unit count; by default where blocks of four units
are at least 3/4 full); DAU_FLAG_NO_DENSE_SPLIT keeps the exact gather-dot.  Bar: the fp32 one (1e-4 relative + 1e-6 of the
max-norm against the oracle) for all four parameter gradients -- the member claims fp32 accuracy, so it gets no bar of its own."""
import numpy as np
import pytest
import torch

from oracle import dau_oracle as orc
from util import assert_parity, make_inputs, record_margins

pytestmark = pytest.mark.gpu

PARAMS = ("dw", "dmu1", "dmu2", "dsigma")


def _plan(N, S, F, G, H, W, flags=None, **kw):
    from dau_conv import _capi
    fl = _capi.FLAG_USE_INTERPOLATION | (_capi.FLAG_DENSE_SPLIT_F16 if flags is None else flags)
    return _capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=kw.pop("sigma_hint", 0.5), flags=fl, **kw)


def _params(plan, x, dy, w, mu1, mu2, sigma=0.5, need=None):
    from dau_conv import _capi
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    S, G, F = w.shape[1:]
    sg = torch.full((1, S, G, F), float(sigma), device="cuda")
    need = need if need is not None else _capi.NEED_DW | _capi.NEED_DMU1 | _capi.NEED_DMU2 | _capi.NEED_DSIGMA
    g = plan.backward(dev(x), dev(dy), dev(w), dev(mu1), dev(mu2), sg, need_mask=need)
    plan.check_status()
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in zip(("dx",) + PARAMS, g)}


def _want(x, dy, w, mu1, mu2, sigma=0.5, **kw):
    return orc.backward(x, dy, w, mu1, mu2, sigma, need=PARAMS, **kw)


def _check(got, want, name, keys=PARAMS):
    for key in keys:
        assert_parity(got[key], want[key], name + "/" + key)
    return record_margins(name, {k: got[k] for k in keys}, {k: want[k] for k in keys},
                          "1e-4 rel + 1e-6 max-norm (fp32 bar; split-f16 gather-dot)")


def _corners(mu1, mu2, c):
    mu1.flat[0] = c; mu2.flat[0] = -c; mu1.flat[1] = -c; mu2.flat[1] = c


@pytest.mark.parametrize("G", [1, 2, 3, 4, 5, 6])
def test_split_gather_dot_unit_counts(G):
    N, S, F, H, W = 3, 20, 36, 13, 17                # ragged batch, channel blocks, regions
    x, dy, w, mu1, mu2 = make_inputs(70 + G, N, S, F, G, H, W, 9, 3.0)
    _corners(mu1, mu2, 3.0)
    _check(_params(_plan(N, S, F, G, H, W), x, dy, w, mu1, mu2), _want(x, dy, w, mu1, mu2), "sdot/G%d" % G)


@pytest.mark.parametrize("m", [0.4, 2.0, 3.0, 3.99])
def test_split_gather_dot_offset_ranges(m):
    """one member for every call within +-4, the layer's clip included (the window's halo is radius 4)"""
    N, S, F, G, H, W = 2, 16, 32, 4, 28, 28
    x, dy, w, mu1, mu2 = make_inputs(81, N, S, F, G, H, W, 9, m)
    _corners(mu1, mu2, m)
    _check(_params(_plan(N, S, F, G, H, W), x, dy, w, mu1, mu2), _want(x, dy, w, mu1, mu2), "sdot/m%.2f" % m)


def test_split_gather_dot_without_dsigma_and_edge_rule():
    """kinds = 3 (no dsigma requested), unit_testing edge rule, one ignored unit, sigma 0.8"""
    from dau_conv import _capi
    N, S, F, G, H, W = 2, 12, 20, 4, 32, 32
    x, dy, w, mu1, mu2 = make_inputs(5, N, S, F, G, H, W, 9, 3.5, ignore=1)
    plan = _plan(N, S, F, G, H, W, flags=_capi.FLAG_DENSE_SPLIT_F16 | _capi.FLAG_UNIT_TESTING, number_units_ignore=1, sigma_hint=0.8)
    got = _params(plan, x, dy, w, mu1, mu2, sigma=0.8, need=_capi.NEED_DW | _capi.NEED_DMU1 | _capi.NEED_DMU2)
    want = _want(x, dy, w, mu1, mu2, sigma=0.8, ignore=1, unit_testing=True)
    _check(got, want, "sdot/kinds3", keys=("dw", "dmu1", "dmu2"))


def test_split_gather_dot_wide_dynamic_range():
    """activations and errors spanning 2^20 across channels: the per-channel power-of-two scales keep every channel's bits"""
    N, S, F, G, H, W = 2, 16, 32, 4, 20, 20
    x, dy, w, mu1, mu2 = make_inputs(9, N, S, F, G, H, W, 9, 3.0)
    x *= (2.0 ** np.linspace(-10, 10, S)).astype(np.float32)[None, :, None, None]
    dy *= (2.0 ** np.linspace(10, -10, F)).astype(np.float32)[None, :, None, None]
    got = _params(_plan(N, S, F, G, H, W), x, dy, w, mu1, mu2)
    want = _want(x, dy, w, mu1, mu2)
    # each output channel against its own max-norm (the range spans 2^40 over the tensor)
    for f in range(F):
        for key in PARAMS:
            assert_parity(got[key][..., f], want[key][..., f], "sdot/range/%s/f%d" % (key, f))


def test_split_gather_dot_inf_beside_finite_channels():
    N, S, F, G, H, W = 2, 16, 32, 4, 16, 16
    x, dy, w, mu1, mu2 = make_inputs(11, N, S, F, G, H, W, 9, 3.0)
    dy[1, 5, 3, 3] = np.inf
    got = _params(_plan(N, S, F, G, H, W), x, dy, w, mu1, mu2)
    want = _want(x, dy, w, mu1, mu2)
    keep = [f for f in range(F) if f != 5]
    for key in PARAMS:
        assert_parity(got[key][..., keep], want[key][..., keep], "sdot/inf/" + key)


def test_split_gather_dot_agrees_with_the_exact_kernel():
    from dau_conv import _capi
    N, S, F, G, H, W = 4, 32, 48, 4, 24, 24
    x, dy, w, mu1, mu2 = make_inputs(13, N, S, F, G, H, W, 9, 3.5)
    split = _params(_plan(N, S, F, G, H, W), x, dy, w, mu1, mu2)
    exact = _params(_plan(N, S, F, G, H, W, flags=_capi.FLAG_NO_DENSE_SPLIT), x, dy, w, mu1, mu2)
    for key in PARAMS:
        assert_parity(split[key], exact[key], "sdot-vs-exact/" + key)


def test_split_gather_dot_scale_invariance():
    """power-of-two scaling of the inputs scales the gradients bit-exactly (the scales are exact)"""
    N, S, F, G, H, W = 2, 16, 16, 4, 16, 16
    x, dy, w, mu1, mu2 = make_inputs(17, N, S, F, G, H, W, 9, 3.0)
    plan = _plan(N, S, F, G, H, W)
    a = _params(plan, x, dy, w, mu1, mu2)
    b = _params(plan, x * np.float32(2.0 ** -12), dy * np.float32(2.0 ** 7), w, mu1, mu2)
    np.testing.assert_array_equal(b["dw"], a["dw"] * np.float32(2.0 ** -5))


@pytest.mark.parametrize("cfg", [
    # name, (N, S, F, G, H, W), offsets within: full depth (every input channel, every position of the batch slice), DEFAULT plans
    ("ns-depth N=8 S=F=256 56x56 G=4 r3", (8, 256, 256, 4, 56, 56), 3.0),
    ("ns-depth N=8 S=F=256 56x56 G=4 r4", (8, 256, 256, 4, 56, 56), 3.99),
    ("c3-depth N=8 S=F=512 28x28 G=4 r3", (8, 512, 512, 4, 28, 28), 3.0),
    ("c1 N=64 96->256 27x27 G=4 r3", (64, 96, 256, 4, 27, 27), 3.0),
])
def test_split_gather_dot_at_baseline_depth(cfg):
    from dau_conv import _capi
    name, (N, S, F, G, H, W), m = cfg
    x, dy, w, mu1, mu2 = make_inputs(2025, N, S, F, G, H, W, 9, m)
    plan = _capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=0.5)
    got = _params(plan, x, dy, w, mu1, mu2)
    # the oracle on a slice of output channels (the gradients of a unit depend on its own output channel only)
    fs = slice(0, 8)
    want = _want(x, dy[:, fs], w[..., fs], mu1[..., fs], mu2[..., fs])
    mg = _check({k: got[k][..., fs] for k in PARAMS}, want, "sdot/" + name)
    print("margins", name, mg)
