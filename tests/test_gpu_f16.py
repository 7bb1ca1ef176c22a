"""GPU: float16 activations at the plan level (DAU_FLAG_IO_F16).  x, dy go in as float16, y and dx come back as float16,
parameters and their gradients stay fp32.  An f16 plan runs the members of the fp32 plan of the same desc with the same fp32
arithmetic on the widened input, so (a) against the oracle fed the f16 values widened to fp32 the only loss is the final
rounding of y / dx (half an ulp of binary16, 2^-11, once per offset-window pass), and (b) for single-pass plans y and dx are
bit for bit torch.half() of what the fp32 plan computes from the widened input, and the parameter gradients are bit-identical."""
import numpy as np
import pytest
import torch

from oracle import dau_oracle as orc
from util import assert_parity

pytestmark = pytest.mark.gpu

I = 1 << 0          # DAU_FLAG_USE_INTERPOLATION


def _inputs(seed, N, S, F, G, H, W, k, m, x_scale=1.0):
    rs = np.random.RandomState(seed)
    x16 = torch.from_numpy((rs.rand(N, S, H, W) * x_scale).astype(np.float32)).half()
    dy16 = torch.from_numpy(rs.randn(N, F, H, W).astype(np.float32)).half()
    w = (rs.randn(1, S, G, F) * 0.1).astype(np.float32)
    lim = k // 2 - 0.01
    mu1 = np.clip(rs.uniform(-m, m, (1, S, G, F)), -lim, lim).astype(np.float32)
    mu2 = np.clip(rs.uniform(-m, m, (1, S, G, F)), -lim, lim).astype(np.float32)
    return x16, dy16, w, mu1, mu2


def _run(plan, x, dy, w, mu1, mu2):
    dev = lambda a: torch.from_numpy(a).cuda()
    S, G, F = w.shape[1:]
    sigma = torch.full((1, S, G, F), 0.5, device="cuda")
    y = plan.forward(x.cuda(), dev(w), dev(mu1), dev(mu2), sigma)
    grads = plan.backward(x.cuda(), dy.cuda(), dev(w), dev(mu1), dev(mu2), sigma)
    plan.check_status()
    return (y,) + tuple(grads)


SHAPES = [
    dict(N=3, S=6, F=40, G=4, H=56, W=56, k=9, m=3),
    dict(N=4, S=8, F=16, G=6, H=28, W=28, k=9, m=3),          # stacked planes, two gather-dot passes
    dict(N=2, S=5, F=8, G=2, H=40, W=72, k=17, m=7),
    dict(N=2, S=3, F=8, G=3, H=33, W=20, k=65, m=20),         # bucket 32: gather-dot offset windows
    dict(N=2, S=128, F=128, G=4, H=16, W=16, k=9, m=3),       # default plan: split gather radii 2-4 and the split gather-dot
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "S%d_F%d_G%d_%dx%d_k%d_m%d" % tuple(s[q] for q in "SFGHWkm"))
def test_f16_io_against_oracle(shape):
    from dau_conv import _capi
    N, S, F, G, H, W, k, m = (shape[q] for q in ("N", "S", "F", "G", "H", "W", "k", "m"))
    x16, dy16, w, mu1, mu2 = _inputs(7, N, S, F, G, H, W, k, m)
    plan = _capi.Plan(N, S, F, G, H, W, max_kernel_size=k, sigma_hint=0.5, flags=I | _capi.FLAG_IO_F16)
    if S == 128:
        assert plan.info["gather_dense_split"] == 0b11100
    y, dx, dw, dmu1, dmu2, dsigma = _run(plan, x16, dy16, w, mu1, mu2)
    assert y.dtype == torch.float16 and dx.dtype == torch.float16 and dw.dtype == torch.float32
    x32, dy32 = x16.float().numpy(), dy16.float().numpy()          # what the kernels actually read
    want_y = orc.forward(x32, w, mu1, mu2, 0.5)
    want = orc.backward(x32, dy32, w, mu1, mu2, 0.5)
    assert_parity(y.float().cpu().numpy(), want_y, "y", rel=2e-3, floor=1e-3)
    assert_parity(dx.float().cpu().numpy(), want["dx"], "dx", rel=2e-3, floor=1e-3)
    for got, key in ((dw, "dw"), (dmu1, "dmu1"), (dmu2, "dmu2"), (dsigma, "dsigma")):
        assert_parity(got.cpu().numpy(), want[key], key)


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("shape, extra, want_split", [
    (dict(N=2, S=128, F=128, G=4, H=16, W=16, k=9, m=3), 0, 0b11100),            # split gather + split gather-dot
    (dict(N=2, S=128, F=128, G=4, H=16, W=16, k=9, m=3), 1 << 10, 0),            # DAU_FLAG_NO_DENSE_SPLIT: the exact kernels
    (dict(N=4, S=8, F=16, G=6, H=28, W=28, k=9, m=3), 0, None),
    (dict(N=2, S=5, F=8, G=2, H=40, W=72, k=17, m=7), 0, None),                 # bucket 8
], ids=["split", "exact", "stacked", "bucket8"])
def test_f16_plan_is_the_fp32_plan_on_the_widened_input(shape, extra, want_split):
    from dau_conv import _capi
    N, S, F, G, H, W, k, m = (shape[q] for q in ("N", "S", "F", "G", "H", "W", "k", "m"))
    x16, dy16, w, mu1, mu2 = _inputs(11, N, S, F, G, H, W, k, m)
    p16 = _capi.Plan(N, S, F, G, H, W, max_kernel_size=k, sigma_hint=0.5, flags=I | extra | _capi.FLAG_IO_F16)
    p32 = _capi.Plan(N, S, F, G, H, W, max_kernel_size=k, sigma_hint=0.5, flags=I | extra)
    assert p16.info == p32.info and p16.info["gather_windows"] == 1
    if want_split is not None:
        assert p16.info["gather_dense_split"] == want_split
    got = _run(p16, x16, dy16, w, mu1, mu2)
    ref = _run(p32, x16.float(), dy16.float(), w, mu1, mu2)
    assert torch.equal(_bits(got[0]), _bits(ref[0].half())), "y"
    assert torch.equal(_bits(got[1]), _bits(ref[1].half())), "dx"
    for g, r, name in zip(got[2:], ref[2:], ("dw", "dmu1", "dmu2", "dsigma")):
        assert torch.equal(g.view(torch.int32), r.view(torch.int32)), name


def _one_unit_plan(flags=0, S=1, F=2, H=16, W=16):
    from dau_conv import _capi
    return _capi.Plan(1, S, F, 1, H, W, flags=I | _capi.FLAG_IO_F16 | flags), _capi.Plan(1, S, F, 1, H, W, flags=I | flags)


def _fwd(plan, x, wvals):
    S, F = x.shape[1], len(wvals)
    w = torch.tensor(wvals, dtype=torch.float32, device="cuda").reshape(1, 1, 1, F).expand(1, S, 1, F).contiguous()
    z = torch.zeros(1, S, 1, F, device="cuda")
    return plan.forward(x, w, z, z.clone(), torch.full((1, S, 1, F), 0.5, device="cuda"))


def test_f16_store_keeps_a_nan_a_nan():
    p16, _ = _one_unit_plan(H=8, W=8)
    x = torch.ones(1, 1, 8, 8, device="cuda")
    x[0, 0, 3, 3] = float("nan")
    y = _fwd(p16, x.half(), [1.0, -1.0])
    assert torch.isnan(y[0, 0, 3, 3]) and torch.isnan(y[0, 1, 3, 3])
    assert torch.isfinite(y[0, 0, 7, 7]) and torch.isfinite(y[0, 1, 7, 7])     # beyond the 7 x 7 prefilter around the NaN


def test_f16_store_overflows_to_inf():
    p16, p32 = _one_unit_plan()
    x = torch.full((1, 1, 16, 16), 60000.0, device="cuda").half()             # representable; y = +-2 x in the interior
    y = _fwd(p16, x, [2.0, -2.0])
    assert torch.isposinf(y[0, 0, 3:-3, 3:-3]).all() and torch.isneginf(y[0, 1, 3:-3, 3:-3]).all()
    ref = _fwd(p32, x.float(), [2.0, -2.0])
    assert torch.equal(_bits(y), _bits(ref.half()))            # the border (finite, some above 65504 in fp32) as torch.half()


def test_f16_store_keeps_subnormals():
    p16, p32 = _one_unit_plan(S=4, F=8, H=24, W=24)
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(1, 4, 24, 24, generator=g) * 3e-5).half().cuda()          # mostly f16 subnormals (< 2^-14)
    wv = [0.5, 1.0, -0.25, 2.0, 0.125, -1.0, 0.75, 1.5]
    y = _fwd(p16, x, wv)
    ref = _fwd(p32, x.float(), wv)
    assert torch.equal(_bits(y), _bits(ref.half()))
    a = y.float().abs()
    assert ((a > 0) & (a < 2.0 ** -14)).sum() > 100             # subnormal outputs are there, not flushed to zero


def test_f16_window_pass_plan():
    """k = 65 with offsets up to +-20 at a size where the gather runs in offset windows: every window pass re-reads the f16
    output, adds and rounds again"""
    from dau_conv import _capi
    N, S, F, G, H, W, k, m = 2, 2, 20, 9, 37, 100, 65, 20
    x16, dy16, w, mu1, mu2 = _inputs(13, N, S, F, G, H, W, k, m)
    plan = _capi.Plan(N, S, F, G, H, W, max_kernel_size=k, sigma_hint=0.5, flags=I | _capi.FLAG_IO_F16)
    assert plan.info["gather_windows"] == 4
    y, dx, dw, dmu1, dmu2, dsigma = _run(plan, x16, dy16, w, mu1, mu2)
    x32, dy32 = x16.float().numpy(), dy16.float().numpy()
    want_y = orc.forward(x32, w, mu1, mu2, 0.5)
    want = orc.backward(x32, dy32, w, mu1, mu2, 0.5)
    assert_parity(y.float().cpu().numpy(), want_y, "y", rel=2e-3, floor=1e-3)
    assert_parity(dx.float().cpu().numpy(), want["dx"], "dx", rel=2e-3, floor=1e-3)
    for got, key in ((dw, "dw"), (dmu1, "dmu1"), (dmu2, "dmu2"), (dsigma, "dsigma")):
        assert_parity(got.cpu().numpy(), want[key], key)
